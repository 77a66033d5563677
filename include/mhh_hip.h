/*
 * mhh_hip.h -- C ABI of the MI355X-native RHS + pressure hot path (libmhh_hip.so).
 *
 * Drop-in boundary for the reference's Advec / Diff / Pres / Boundary_cyclic operators
 * (adconnolly/microhh). The reference has no FFI; its GPU seam is the set of member
 * functions that the .cu files re-define under USECUDA. Every entry point below names the
 * reference member function / kernel it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the adaptor TU a MicroHH maintainer would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = default stream). Nothing here synchronises the device unless stated.
 *   - all field pointers are DEVICE pointers, layout identical to the reference's host layout:
 *     ijk = i + j*icells + k*ijcells, i fastest, ghost cells included (include/grid.h:70-80).
 *   - element type is selected by mhh_grid.dtype (MHH_F64 = reference default build,
 *     MHH_F32 = reference -DUSESP build). Scalars cross the ABI as double and are narrowed
 *     exactly where the reference narrows them.
 *   - return value: 0 = ok, otherwise an MHH_E* code; mhh_last_error() gives the text. The C++
 *     adaptor turns non-zero into std::runtime_error like the reference host code does
 *     (include/tools.h:49-56, src/pres.cu:185-186).
 *   - buffers are owned by the caller (Field3d::init_device, src/field3d.cu:32-47); kernels
 *     borrow and never retain pointers. Not re-entrant per plan object.
 */
#ifndef MHH_HIP_H
#define MHH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MHH_F64 0
#define MHH_F32 1

#define MHH_OK        0
#define MHH_EINVAL    1   /* bad argument / unsupported combination */
#define MHH_EHIP      2   /* HIP runtime error */
#define MHH_EFFT      3   /* rocFFT error (reference: runtime_error("FFT error")) */
#define MHH_ENOMEM    4

/* Boundary_cyclic Edge (include/boundary_cyclic.h:33) */
#define MHH_EDGE_EW   0
#define MHH_EDGE_NS   1
#define MHH_EDGE_BOTH 2

/* advection schemes (src/advec.cxx:55-83 swadvec) */
#define MHH_ADVEC_2    2
#define MHH_ADVEC_2I5  25
#define MHH_ADVEC_4M   41   /* 4th-order kinetic-energy-conserving form (src/advec_4m.cxx); per-field entry points only */
#define MHH_ADVEC_2I53 253  /* advec_2i5 with 4th/3rd instead of 6th/5th order vertically (src/advec_2i53.cxx); per-field entry points only */
#define MHH_ADVEC_2I62 262  /* 6th-order interpolation horizontally, 2nd order vertically (src/advec_2i62.cxx); per-field entry points only */
#define MHH_ADVEC_2I4  24   /* 2nd-order fluxes with 4th-order interpolation (src/advec_2i4.cxx); per-field entry points only */
#define MHH_ADVEC_4    4
/* diffusion schemes (src/diff.cxx:57-85 swdiff) */
#define MHH_DIFF_2     2
#define MHH_DIFF_4     4
#define MHH_DIFF_SMAG2 22

/* Mirror of Grid_data<TF> (include/grid.h:49-135) reduced to what the hot path reads.
 * Metric arrays are device pointers of kcells elements of the grid's dtype. */
typedef struct mhh_grid
{
    int itot, jtot, ktot;
    int imax, jmax, kmax;          /* per-rank interior; == itot,jtot,ktot on one GPU   */
    int igc, jgc, kgc;
    int icells, jcells, ijcells, kcells;
    int istart, jstart, kstart;
    int iend, jend, kend;
    int dtype;                     /* MHH_F64 | MHH_F32                                  */
    int npx, npy;                  /* slab decomposition: npx must be 1                   */
    int mpicoordx, mpicoordy;      /* rank coordinates (include/master.h:34-53)           */
    long long ncells;
    double xsize, ysize, zsize;
    double dx, dy;
    const void* z;
    const void* zh;
    const void* dz;
    const void* dzh;
    const void* dzi;
    const void* dzhi;
    const void* dzi4;
    const void* dzhi4;
} mhh_grid;

#define MHH_MAX_SCALARS 8

/* Mirror of the slice of Fields<TF> the operators touch (include/fields.h:132-161):
 * mp (u,v,w), mt (ut,vt,wt), sp/st (scalars and their tendencies), sd["evisc"], sd["p"],
 * rhoref/rhorefh, and the 2-D surface arrays consumed by diff_smag2. NULL where unused. */
typedef struct mhh_fields
{
    void* u;  void* v;  void* w;
    void* ut; void* vt; void* wt;
    int   nscalars;
    void* s [MHH_MAX_SCALARS];
    void* st[MHH_MAX_SCALARS];
    double svisc[MHH_MAX_SCALARS];   /* Field3d::visc of each scalar                      */
    void* evisc;
    void* p;
    const void* rhoref;              /* [kcells] */
    const void* rhorefh;             /* [kcells] */
    double visc;                     /* Fields::visc                                       */
    /* surface model inputs (Boundary_surface outputs; NULL => resolved walls, "default"). const is the operators' view of
     * them: mhh_boundary_surface_exec and the mhh_surface_* stages WRITE the bottom fluxes and dudz, dvdz, dbdz. */
    const void* u_fluxbot; const void* u_fluxtop;
    const void* v_fluxbot; const void* v_fluxtop;
    const void* s_fluxbot[MHH_MAX_SCALARS]; const void* s_fluxtop[MHH_MAX_SCALARS];
    const void* dudz; const void* dvdz; const void* dbdz;   /* boundary.get_dudz() etc.    */
    const void* z0m;
    int   s_fluxlimit[MHH_MAX_SCALARS];   /* scalar is in advec.fluxlimit_list (src/advec_2i5.cxx:39,921) */
} mhh_fields;

const char* mhh_last_error(void);
int mhh_version(void);
/* Block the host until everything queued on `stream` has finished (NULL = default stream): what the reference's
 * cudaDeviceSynchronize() at the end of every exec does before Stats reads the tendencies (src/advec_2.cu:219). */
int mhh_synchronize(void* stream);

/* ---- Boundary_cyclic -------------------------------------------------------------------
 * replaces Boundary_cyclic<TF>::exec_g / exec (src/boundary_cyclic.cu:91-127,
 * src/boundary_cyclic.cxx:370-443) and exec_2d(_g) (:445-500). jtot==1 replicates row. */
int mhh_boundary_cyclic   (const mhh_grid* g, void* data, int edge, void* stream);
int mhh_boundary_cyclic_2d(const mhh_grid* g, void* data, void* stream);
/* Boundary_cyclic::exec(unsigned int*, Edge) / exec_2d(unsigned int*) (src/boundary_cyclic.cxx:510-660): the same fills for
 * 32-bit integer fields (the immersed-boundary / land-surface index masks), whatever the grid's dtype                    */
int mhh_boundary_cyclic_u32(const mhh_grid* g, void* data /* unsigned int [ncells] */, int edge, void* stream);
int mhh_boundary_cyclic_2d_u32(const mhh_grid* g, void* data /* unsigned int [ijcells] */, void* stream);
/* several fields in one launch (Boundary::set_prognostic_cyclic_bcs, src/boundary.cxx:447-458) */
int mhh_boundary_cyclic_n (const mhh_grid* g, void* const* data, int nfields, int edge, void* stream);

/* ---- Advection (kernel granularity of the reference) -----------------------------------
 * scheme 2  : src/advec_2.cxx:81-202   (advec_u/v/w/s),  GPU src/advec_2.cu:38-117
 * scheme 25 : src/advec_2i5.cxx:151-728,                 GPU src/advec_2i5.cu:41-510
 * scheme 4  : src/advec_4.cxx:88-486,                    GPU src/advec_4.cu:37-442
 * scheme 24 : src/advec_2i4.cxx:101-640 (advec_u/v/w/s), calc_cfl :51-99
 * scheme 262: src/advec_2i62.cxx:105-310,                calc_cfl :58-105
 * scheme 253: src/advec_2i53.cxx:120-700,                calc_cfl :55-118
 * scheme 41 : src/advec_4m.cxx:90-478,                   calc_cfl :51-88
 * Each call adds the advective tendency of one field (read-modify-write of the tendency). */
int mhh_advec_u(const mhh_grid* g, int scheme, void* ut, const void* u, const void* v, const void* w,
                const void* rhoref, const void* rhorefh, void* stream);
int mhh_advec_v(const mhh_grid* g, int scheme, void* vt, const void* u, const void* v, const void* w,
                const void* rhoref, const void* rhorefh, void* stream);
int mhh_advec_w(const mhh_grid* g, int scheme, void* wt, const void* u, const void* v, const void* w,
                const void* rhoref, const void* rhorefh, void* stream);
int mhh_advec_s(const mhh_grid* g, int scheme, void* st, const void* s, const void* u, const void* v, const void* w,
                const void* rhoref, const void* rhorefh, void* stream);
/* Koren-limited scalar advection, Advec_monotonic::advec_s_lim (include/advec_monotonic.h:79-180),
 * used by Advec_2i5::exec for the scalars in fluxlimit_list (src/advec_2i5.cxx:1030). */
int mhh_advec_s_lim(const mhh_grid* g, void* st, const void* s, const void* u, const void* v, const void* w,
                    const void* rhoref, const void* rhorefh, void* stream);
/* Advec::exec (src/advec_2.cxx:297-335, advec_2i5.cxx:977-1044, advec_4.cxx:592-650) */
int mhh_advec_exec(const mhh_grid* g, int scheme, const mhh_fields* f, void* stream);
/* calc_cfl + Master::max + *dt  (src/advec_2.cxx:51-78, advec_2i5.cxx:60-148, advec_4.cxx:51-86);
 * *cfl_out is a host double; the call synchronises `stream`. `work` = device scratch of
 * mhh_reduce_work_bytes() bytes. */
int mhh_advec_cfl(const mhh_grid* g, int scheme, const void* u, const void* v, const void* w,
                  double dt, void* work, double* cfl_out, void* stream);
unsigned long long mhh_reduce_work_bytes(void);

/* ---- Diffusion ---------------------------------------------------------------------------
 * diff_2: src/diff_2.cxx:39-86 (diff_c, diff_w)   GPU src/diff_2.cu:34-90
 * diff_4: src/diff_4.cxx:41-173                   GPU src/diff_4.cu:37-160          */
int mhh_diff_c(const mhh_grid* g, int order, void* at, const void* a, double visc, void* stream);
int mhh_diff_w(const mhh_grid* g, int order, void* wt, const void* w, double visc, void* stream);

/* diff_smag2 (src/diff_smag2.cxx; parity target is the CPU path, NOT src/diff_smag2.cu, see
 * DESIGN.md). surface_model = 1 <=> boundary.get_switch() != "default".                  */
int mhh_smag2_strain2(const mhh_grid* g, int surface_model, void* strain2,
                      const void* u, const void* v, const void* w,
                      const void* dudz, const void* dvdz, void* stream);                 /* :47-155  */
/* mlen0[kcells] = cs*pow(dx*dy*dz[k],1/3) is a per-level table computed on the HOST with the C library's pow
 * (mhh_smag2_mlen0_host; `g` then carries HOST metric pointers) and uploaded by the caller -- what
 * Diff_smag2::prepare_device does in the reference's GPU path (src/diff_smag2.cu:521-542).               */
int mhh_smag2_mlen0_host(const mhh_grid* g_host, double cs, void* mlen0_host_out);
/* mlen2[kcells]: the squared mixing length of calc_evisc / calc_evisc_neutral (src/diff_smag2.cxx:273-276,325-328:
 * wall-damped with kappa*(z+z0m) under a surface model, mlen0^2 otherwise) for a HORIZONTALLY UNIFORM roughness length
 * z0m, evaluated on the host with the same IEEE operations as the kernels (same bits). Optional: passed as
 * mhh_diff_params::mlen2 it replaces three divisions and a square root per cell of exec_viscosity by a table look-up.
 * `g_host` carries HOST metric pointers (z); valid while z0m stays uniform and unchanged. */
int mhh_smag2_mlen2_host(const mhh_grid* g_host, int surface_model, int neutral, const void* mlen0_host, double z0m, void* mlen2_host_out);
int mhh_smag2_evisc(const mhh_grid* g, int surface_model, void* evisc, const void* N2,
                    const void* bgradbot, const void* z0m, const void* mlen0, double tPr, void* stream); /* :254-367 incl. cyclic fill */
int mhh_smag2_evisc_neutral(const mhh_grid* g, int surface_model, void* evisc,
                    const void* u, const void* v, const void* z0m,
                    const void* mlen0, double visc, void* stream);                       /* :157-252 incl. cyclic fill */
int mhh_smag2_diff_u(const mhh_grid* g, int surface_model, void* ut, const void* u, const void* v, const void* w,
                     const void* evisc, const void* fluxbot, const void* fluxtop,
                     const void* rhoref, const void* rhorefh, double visc, void* stream); /* :369-468 */
int mhh_smag2_diff_v(const mhh_grid* g, int surface_model, void* vt, const void* u, const void* v, const void* w,
                     const void* evisc, const void* fluxbot, const void* fluxtop,
                     const void* rhoref, const void* rhorefh, double visc, void* stream); /* :470-571 */
int mhh_smag2_diff_w(const mhh_grid* g, void* wt, const void* u, const void* v, const void* w,
                     const void* evisc, const void* rhoref, const void* rhorefh, double visc, void* stream); /* :573-617 */
int mhh_smag2_diff_c(const mhh_grid* g, int surface_model, void* at, const void* a,
                     const void* evisc, const void* fluxbot, const void* fluxtop,
                     const void* rhoref, const void* rhorefh, double tPr, double visc, void* stream); /* :619-709 */
int mhh_smag2_dnmul(const mhh_grid* g, const void* evisc, double tPr, void* work,
                    double* dnmul_out, void* stream);                                      /* :711-736 + master.max */
/* Thermo_dry calc_N2 hook (src/thermo_dry.cxx:66-78): input of calc_evisc */
int mhh_calc_N2(const mhh_grid* g, void* N2, const void* th, const void* thref, double grav, void* stream);

/* Diff::exec_viscosity / Diff::exec (src/diff_smag2.cxx:1046-1188, :939-1043; diff_2.cxx:150-180;
 * diff_4.cxx:262-300). For smag2, N2 (3-D) must be supplied unless `th_for_N2` >= 0, in which case
 * N2 is evaluated inline from scalar th_for_N2 with thref/grav (fusion of thermo.get_thermo_field). */
typedef struct mhh_diff_params
{
    double cs, tPr;          /* [diff] cs, tPr  (src/diff_smag2.cxx:853-855)              */
    int    surface_model;    /* boundary switch != "default"                               */
    int    neutral;          /* thermo switch == "0"                                       */
    const void* N2;          /* 3-D buoyancy frequency, or NULL with th_for_N2 >= 0        */
    int    th_for_N2;
    const void* thref;       /* [kcells]                                                   */
    double grav;
    const void* mlen0;       /* [kcells] device table from mhh_smag2_mlen0_host            */
    /* dry buoyancy folded into mhh_rhs_exec (Thermo_dry::exec precedes Advec::exec in Model::exec,
     * src/model.cxx:365,388): wt += grav/threfh[k]*(th_h - threfh[k]) for scalar th_for_N2, first. */
    int    buoyancy;         /* 0 = off, 2 / 4 = interpolation order (swspatialorder)      */
    const void* threfh;      /* [kcells]                                                   */
    /* slab decomposition (npy > 1): also evaluate evisc on the ghost rows jstart-1 and jend from the
     * u, v, w (, th) halos instead of exchanging it -- the same operands as on the neighbour, hence
     * the same bits; the diffusion kernels read evisc one row beyond the slab only. Needs jgc >= 2 and
     * the 2-D surface inputs valid on those rows.                                                      */
    int    evisc_ghost_rows;
    const void* mlen2;       /* [kcells] optional device table from mhh_smag2_mlen2_host (uniform z0m), or NULL */
    /* which thermodynamics th_for_N2 belongs to. 0 = Thermo_dry (the meaning above). 1 = Thermo_buoy (src/thermo_buoy.cxx):
     * th_for_N2 names the buoyancy scalar b; the inline N2 of exec_viscosity is 0.5*(b[k+1]-b[k-1])*dzi[k] + bg_n2 (calc_N2,
     * :49-61; thref and grav unused), and the folded buoyancy is b at the w level (calc_buoyancy_tend_2nd / _4th, :94-109,
     * :167-184; threfh unused). With alpha != 0 or bg_n2 != 0 the slope / stratified form (:111-165, :186-250) applies: the
     * fused passes then run mhh_thermo_buoy_tend first and fold nothing. Zero-initialised: Thermo_dry, as before.          */
    int    buoyancy_kind;
    double bg_n2;            /* [thermo] N2: background stratification (bs.n2)                       */
    double alpha;            /* [thermo] alpha: slope angle in radians (bs.alpha)                    */
    double utrans;           /* grid.utrans: Galilean transformation velocity                        */
} mhh_diff_params;
int mhh_diff_exec_viscosity(const mhh_grid* g, int scheme, const mhh_fields* f, const mhh_diff_params* p, void* stream);
/* exec_viscosity over the rows [j0, j1) of [jstart-1, jend+1) only (the wall mirror and the east-west wrap still cover
 * all rows): lets the slab driver evaluate the rows that need no north-south halo while the halos travel. */
int mhh_diff_exec_viscosity_rows(const mhh_grid* g, int scheme, const mhh_fields* f, const mhh_diff_params* p,
                                 int j0, int j1, void* stream);
int mhh_diff_exec_viscosity_rows2(const mhh_grid* g, int scheme, const mhh_fields* f, const mhh_diff_params* p, int j0, int j1, int j2, int j3, void* stream);
/* diagnostic: launches of the k-marching form of exec_viscosity so far (it needs 16-byte aligned rows; other layouts
 * take the one-thread-per-cell kernel, same bits) */
unsigned long long mhh_stat_visc_march_launches(void);
unsigned long long mhh_stat_rhs44_march_launches(void);   /* same for the k-marching form of (advec_4, diff_4) in mhh_rhs_exec */
/* same for the scalar pass of the k-marching (advec_2i5, diff_smag2) kernel: one per launch, a launch takes a batch of scalars
 * 1, 2, ... (mhh_rhs_exec, mhh_rhs_exec_rows(2), mhh_advec_exec, mhh_diff_exec; MHH_SCALAR_IMPL=cell: the per-field kernels) */
unsigned long long mhh_stat_scalar_march_launches(void);
/* same for the scalar pass of the k-marching (advec_4, diff_4) kernel: one per launch, a launch takes a batch of scalars 0, 1, ...
 * (mhh_rhs_exec, mhh_advec_exec, mhh_diff_exec where the 4th-order marching kernel takes u, v, w, under MHH_SCALAR_IMPL=march; the default is the per-field kernels) */
unsigned long long mhh_stat_scalar4_march_launches(void);
/* diagnostic: the copy form the LAST launch of a k-marching kernel took (kernel: 0 = the fused 2i5 + smag2 kernel, 1 = its scalar
 * pass, 2 = the advec_4 + diff_4 kernel, 3 = exec_viscosity, 4 = the scalar pass of the advec_4 + diff_4 kernel). *piece_bytes: 16 or 4 bytes per LDS-DMA piece (0: never launched);
 * *hx: cells the tile of the fields starts west of a block's first cell; *ex: the same for the evisc tile (0: the launch copies
 * none); *cells_per_lane: 2 for the packed fp32 form. 16-byte pieces are taken only with istart - hx on a piece of the row. */
int mhh_stat_march_form(int kernel, int* piece_bytes, int* hx, int* ex, int* cells_per_lane);
/* self test of a device primitive of exec_viscosity: the square root for arguments known to be >= 2^-767 (csrc/gfx950_prims.h,
 * sqrt_in_range) against the compiler's sqrt on n arguments drawn from `seed`; *mismatches (host memory) must come back 0 */
int mhh_selftest_sqrt_in_range(unsigned long long n, unsigned long long seed, unsigned long long* mismatches, void* stream);
int mhh_diff_exec(const mhh_grid* g, int scheme, const mhh_fields* f, const mhh_diff_params* p, void* stream);

/* Thermo_dry::exec buoyancy tendency, calc_buoyancy_tend_2nd / _4th (src/thermo_dry.cxx:165-197,
 * GPU src/thermo_dry.cu): wt[k] += grav/threfh[k]*(interp(th) - threfh[k]) for k in (kstart, kend). */
int mhh_thermo_dry_buoyancy_tend(const mhh_grid* g, int order, void* wt, const void* th, const void* threfh,
                                 double grav, void* stream);

/* Thermo_buoy::exec (src/thermo_buoy.cxx:347-395) in ONE launch, all fields through `f`; b = f->s[b_index], its tendency
 * f->st[b_index]. alpha == 0 and n2 == 0: the flat form, wt += interp(b) at the w level (k in (kstart, kend)); otherwise
 * the slope / stratified form: ut += sin(alpha)*interp_x(b), wt += cos(alpha)*interp(b),
 * bt -= n2*(sin(alpha)*(interp(u) + utrans) + cos(alpha)*interp(w)). order 2 | 4 (grid.swspatialorder) selects interp2 /
 * interp4c; order 4 needs kgc >= 2 and, for the slope form, igc >= 2. sin and cos are taken on the host in the grid's dtype
 * (std::sin / std::cos of TF(alpha)), as the reference does. swbaroclinic is not covered.                              */
int mhh_thermo_buoy_tend(const mhh_grid* g, int order, const mhh_fields* f, int b_index, double alpha, double n2,
                         double utrans, void* stream);
/* Thermo_buoy::get_thermo_field("N2") (calc_N2, src/thermo_buoy.cxx:49-61): N2 = 0.5*(b[k+1]-b[k-1])*dzi[k] + bg_n2, interior */
int mhh_thermo_buoy_N2(const mhh_grid* g, void* N2, const void* b, double bg_n2, void* stream);

/* ---- Fused RHS: advec.exec + diff.exec in one pass over the tendencies ------------------
 * Same arithmetic, same order of accumulation into each tendency as calling
 * mhh_advec_exec then mhh_diff_exec (bit-identical results), one read of every input
 * and one read-modify-write of every tendency for the pairs (2,2) (25,22) (4,4); any other
 * pair of valid schemes runs as the two operator calls.                                   */
int mhh_rhs_exec(const mhh_grid* g, int advec_scheme, int diff_scheme, const mhh_fields* f,
                 const mhh_diff_params* p, void* stream);
/* p->buoyancy with p->buoyancy_kind == 1 (Thermo_buoy): the flat form is folded into the w equation of the (2,2) and (2i5,smag2)
 * passes (b = scalar 0 in the marching one; another index, or a flux-limited b, runs mhh_thermo_buoy_tend first) and of the
 * (4,4) pass (with p->buoyancy == 4, in both its forms); every other pair runs mhh_thermo_buoy_tend first. The slope / stratified
 * form is never folded: mhh_thermo_buoy_tend, then the pass without buoyancy, issued only once the call's inputs have passed their
 * checks. Same bits as mhh_thermo_buoy_tend followed by the unfused calls in every case.                              */

/* the (advec_2i5, diff_smag2) pass over the rows [j0, j1) of the interior only; u, v, w and up to MHH_MAX_SCALARS
 * unlimited scalars (scalar 0 in the fused marching kernel, the others in its scalar pass over the same rows; buoyancy only
 * as the 2nd-order form folded with scalar 0: Thermo_dry, or Thermo_buoy's flat form); same bits as the whole-slab call on those rows */
int mhh_rhs_exec_rows(const mhh_grid* g, int advec_scheme, int diff_scheme, const mhh_fields* f,
                      const mhh_diff_params* p, int j0, int j1, void* stream);
/* the same over TWO disjoint, ordered row ranges in one launch (a slab's two edge strips once its north-south halos are in) */
int mhh_rhs_exec_rows2(const mhh_grid* g, int advec_scheme, int diff_scheme, const mhh_fields* f, const mhh_diff_params* p, int j0, int j1, int j2, int j3, void* stream);

/* ---- Pressure ----------------------------------------------------------------------------
 * Plan object = Pres_2 / Pres_4 private state: bmati/bmatj, a/c (m1..m7), rocFFT plans,
 * work buffers (Pres_2::init/set_values/prepare_device: src/pres_2.cxx:107-153,
 * src/pres_2.cu:217-240; pres_4.cxx:179-252).  rhoref/rhorefh/dz/dzhi(/dzi4/dzhi4) are read at
 * creation through HOST pointers (set_values runs on the host in the reference too).       */
typedef struct mhh_pres_plan mhh_pres_plan;
int  mhh_pres_plan_create(const mhh_grid* g, int order /*2|4*/,
                          const void* host_dz, const void* host_dzhi,
                          const void* host_dzi4, const void* host_dzhi4,
                          const void* host_rhoref, const void* host_rhorefh,
                          mhh_pres_plan** out);
void mhh_pres_plan_destroy(mhh_pres_plan* plan);
/* Pres::exec(dt): input -> solve -> output (src/pres_2.cxx:66-94, pres_4.cxx:64-140) */
int mhh_pres_exec(mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, double dt, void* stream);
/* Power-of-two itot, jtot: three kernels that do the transforms in LDS (pres_2: csrc/pres_lds.h, pres_4: csrc/pres_lds4.h) instead
 * of the seven passes of the staged form. mhh_pres_exec takes this form from 2^24 cells on (where it is faster on MI355X:
 * profiles/r3_pres_forms.md); MHH_PRES_LDS=1 / 0 selects it wherever the plan has it / never. The stages one by one, for tests:
 * 1 = Pres::input + transform along x (src/pres_2.cxx:156-196, src/pres_4.cxx:256-317, src/fft.cxx:451-497), 2 = transforms along y
 * around the k sweeps (Thomas, src/pres_2.cxx:202-263; the factored 7-band system, src/pres_4.cxx:358-470, 574-730), 3 = transform
 * back along x + p with its ghost cells + Pres::output (src/pres_2.cxx:333-387; src/pres_4.cxx:481-571). pres_2 with itot <= 256:
 * stage 2 runs two blocks per column (a twisted factorisation: bottom-up and top-down eliminations that meet half way; MHH_PRES_Y_TWISTED=0 / 1). */
int   mhh_pres_lds_stage(mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, double dt, int stage, void* stream);
int   mhh_pres_plan_has_lds_form(const mhh_pres_plan* plan);
int   mhh_pres_exec_form(const mhh_pres_plan* plan);   /* what mhh_pres_exec will run: 0 = staged (rocFFT), 1 = transforms in LDS */
void* mhh_pres_plan_spectral(mhh_pres_plan* plan);   /* device array between the stages: S[k][kx][j], complex */
/* stages, exposed for the slab-decomposed driver and for parity tests */
int mhh_pres_input (mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, double dt, void* p_packed, void* stream); /* pres_2.cxx:156-196, pres_4.cxx:256-317 */
int mhh_pres_solve (mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, void* p_packed, void* stream);            /* pres_2.cxx:267-362, pres_4.cxx:320-529 */
int mhh_pres_output(mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, void* stream);                            /* pres_2.cxx:365-387, pres_4.cxx:533-571 */
/* Pres::check_divergence (src/pres_2.cxx:391-422, pres_4.cxx:733-767); synchronises stream */
int mhh_pres_check_divergence(const mhh_grid* g, int order, const mhh_fields* f, void* work, double* div_out, void* stream);

/* plan-free forms of the pointwise stages (used by the slab driver; with npy > 1 the north-south halo of vt
 * is the caller's exchange, the east-west wrap of ut stays local) */
int mhh_pres_input_packed(const mhh_grid* g, int order, const mhh_fields* f, double dt, void* p_packed, void* stream);
int mhh_pres_output_order(const mhh_grid* g, int order, const mhh_fields* f, void* stream);

/* ---- Slab decomposition in y over the GPUs of one node (npx = 1, npy = N; the reference has no multi-GPU
 * mode, its CPU-MPI path is the model: src/boundary_cyclic.cxx:116-176, src/transpose.cxx:170-219,
 * src/fft.cxx:451-583, src/pres_2.cxx:297-299). The library packs/unpacks; the HOST issues the exchanges
 * (ring send/recv for halos, all-to-all for the x<->y transpose) with RCCL through torch.distributed.
 * With npy > 1, mhh_boundary_cyclic* only accept MHH_EDGE_EW and the operators that end in a cyclic fill
 * (exec_viscosity, evisc) do the east-west wrap only.                                                     */
/* halo buffers: [field][k][jgc][icells]; send_south = southernmost interior rows (-> south neighbour's north
 * ghosts), send_north = northernmost interior rows (-> north neighbour's south ghosts)                     */
unsigned long long mhh_halo_buffer_elems(const mhh_grid* g, int nfields);
int mhh_halo_pack_ns  (const mhh_grid* g, void* const* fields, int nfields, void* send_south, void* send_north, void* stream);
int mhh_halo_unpack_ns(const mhh_grid* g, void* const* fields, int nfields, const void* recv_from_south, const void* recv_from_north, void* stream);
/* partial exchange: rows_south rows travel south, rows_north rows travel north (0..jgc each), buffers
 * [field][k][rows][icells]. pres_2 input reads vt[j+1] only (src/pres_2.cxx:181,193): rows_south = 1, rows_north = 0;
 * pres_2 output reads p[j-1] only (:383-385): rows_south = 0, rows_north = 1. On unpack, recv_from_south holds the
 * rows_north rows the south neighbour sent north, recv_from_north the rows_south rows the north neighbour sent south. */
int mhh_halo_pack_rows  (const mhh_grid* g, void* const* fields, int nfields, int rows_south, int rows_north,
                         void* send_south, void* send_north, void* stream);
int mhh_halo_unpack_rows(const mhh_grid* g, void* const* fields, int nfields, int rows_south, int rows_north,
                         const void* recv_from_south, const void* recv_from_north, void* stream);
/* pres_2 (and pres_4, below) split at the transposes, in nchunks slices of k (mhh_pres_slab_set_chunks, ktot % nchunks == 0; a new
 * plan has ONE slice = all levels), so that the host can overlap the all-to-all of slice c with the transforms of slice c+1 (the
 * reference's FFT::exec_forward transposes and transforms plane batches in turn as well, src/fft.cxx:451-583). The two all-to-all
 * buffers hold mhh_pres_slab_xbuf_elems() COMPLEX elements each, laid out [slice][peer][k in slice][jl][kxl]: slice c is the
 * equal-split all-to-all of elements [c*n, (c+1)*n), n = mhh_pres_slab_xbuf_elems() / nchunks. Call order per solve (order 2):
 *   north-south halo of vt (rows_south = 1 is all the input reads);  mhh_pres_input_packed(g, 2) into mhh_pres_slab_packed;
 *   for c: fwd_x_pack_chunk(c) -> all-to-all(c);  for c: fwd_y_chunk(c);  solve_y;
 *   for c: bwd_y_chunk(c) -> all-to-all(c);       for c: bwd_x_chunk(c);
 *   unpack_output_slab; halo of p (rows_north = 1); output_south_row     -- or: unpack_slab; halo of p; mhh_pres_output_order(g, 2).
 * unpack_output_slab applies Pres_2::output (src/pres_2.cxx:365-387) in the unpack kernel for everything but vt on the
 * southernmost row (its p[j-1] lives on the south neighbour): same bits as the second ending, one pass over p, ut, vt, wt less. */
typedef struct mhh_pres_slab_plan mhh_pres_slab_plan;
int  mhh_pres_slab_plan_create(const mhh_grid* g, const void* host_dz, const void* host_dzhi,
                               const void* host_rhoref, const void* host_rhorefh, mhh_pres_slab_plan** out);
void mhh_pres_slab_plan_destroy(mhh_pres_slab_plan* plan);
unsigned long long mhh_pres_slab_xbuf_elems(const mhh_pres_slab_plan* plan);
void* mhh_pres_slab_packed(mhh_pres_slab_plan* plan);   /* plan-owned packed-divergence buffer (imax*jmax*kmax) */
int mhh_pres_slab_set_chunks(mhh_pres_slab_plan* plan, int nchunks);          /* rebuilds the plan's transforms for ktot / nchunks levels */
int mhh_pres_slab_chunks(const mhh_pres_slab_plan* plan);
int mhh_pres_fwd_x_pack_chunk(mhh_pres_slab_plan* plan, const mhh_grid* g, void* p_packed, void* sendbuf, int c, void* stream);
int mhh_pres_fwd_y_chunk     (mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, int c, void* stream);
int mhh_pres_solve_y         (mhh_pres_slab_plan* plan, const mhh_grid* g, void* stream);
int mhh_pres_bwd_y_chunk     (mhh_pres_slab_plan* plan, const mhh_grid* g, void* sendbuf, int c, void* stream);
int mhh_pres_bwd_x_chunk     (mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, int c, void* stream);
int mhh_pres_unpack_output_slab(mhh_pres_slab_plan* plan, const mhh_grid* g, const mhh_fields* f, void* stream);
int mhh_pres_output_south_row (const mhh_grid* g, const mhh_fields* f, void* stream);
/* The same calls on slice 0 of a ONE-slice plan, joined per side of the transposes: fwd_x_pack = fwd_x_pack_chunk(0);
 * fwd_y_solve_bwd_y = fwd_y_chunk(0), solve_y, bwd_y_chunk(0); bwd_x_unpack = bwd_x_chunk(0), unpack_slab; bwd_x_unpack_output =
 * bwd_x_chunk(0), unpack_output_slab. On a plan with more than one slice they return MHH_EINVAL (the message names
 * mhh_pres_slab_set_chunks(plan, 1)): its transforms and buffer layout are those of the slices. */
int mhh_pres_fwd_x_pack       (mhh_pres_slab_plan* plan, const mhh_grid* g, void* p_packed, void* sendbuf, void* stream);
int mhh_pres_fwd_y_solve_bwd_y(mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, void* sendbuf, void* stream);
int mhh_pres_bwd_x_unpack     (mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, const mhh_fields* f, void* stream);
int mhh_pres_bwd_x_unpack_output(mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, const mhh_fields* f, void* stream);
/* pres_4 on the slab (src/pres_4.cxx:64-140; the reference's MPI decomposition swaps the mode indices after the x/y transpose as
 * Pres_2 does, src/pres_4.cxx:327-470). mhh_pres_slab_plan_create_order is the slab counterpart of mhh_pres_plan_create
 * (Pres_4::set_values, src/pres_4.cxx:179-252, from the HOST metrics dzi4 / dzhi4; order 2 reads dz, dzhi, rhoref, rhorefh and gives
 * the plan of mhh_pres_slab_plan_create). Order 4 needs jgc >= 2, kgc >= 2, igc >= 2, kmax >= 4 and a 3-D grid (jtot > 1). Its plan
 * keeps the LU factors of the 7-band system of every column of the rank (src/pres_4.cxx:358-470, 574-730): 7*(kmax+4)*nxb*jtot
 * values, nxb = ceil((itot/2+1)/npy). Call order per solve (order 4):
 *   north-south halo of vt, rows_south = 2, rows_north = 1 (the input reads vt[j-1..j+2], src/pres_4.cxx:312-315);
 *   mhh_pres_input_packed(g, 4) into mhh_pres_slab_packed;  the chunk calls above with solve_y, then mhh_pres_unpack_slab;
 *   halo of p, rows_south = 1, rows_north = 2 (the output reads p[j-2..j+1], src/pres_4.cxx:555-569);  mhh_pres_output_order(g, 4).
 * The unpack writes p's interior rows, its x halo and the four mirrored vertical ghost levels (src/pres_4.cxx:481-528). The fused
 * Pres_2::output entry points (bwd_x_unpack_output, unpack_output_slab) and the LDS x stages (mhh_pres_slab_lds_*) refuse an order-4
 * plan, mhh_pres_slab_has_lds returns 0 for it; mhh_pres_output_south_row takes no plan and is part of the order-2 sequence only. */
int mhh_pres_slab_plan_create_order(const mhh_grid* g, int order /*2|4*/, const void* host_dz, const void* host_dzhi,
                                    const void* host_dzi4, const void* host_dzhi4, const void* host_rhoref, const void* host_rhorefh,
                                    mhh_pres_slab_plan** out);
int mhh_pres_slab_order(const mhh_pres_slab_plan* plan);
/* the unpack (either order): the packed solution of the last bwd_x_chunk into p (src/pres_2.cxx:333-362, src/pres_4.cxx:481-528) */
int mhh_pres_unpack_slab(mhh_pres_slab_plan* plan, const mhh_grid* g, const mhh_fields* f, void* stream);
/* The x stages of the slab solve with the transforms in LDS (csrc/pres_lds.h; power-of-two itot, jmax a multiple of 8;
 * mhh_pres_slab_has_lds tells): Pres_2::input + the transform along x (src/pres_2.cxx:156-196, src/fft.cxx:451-497) of k-slice c
 * written straight into segment c of the send buffer of Transpose::exec_xy (src/transpose.cxx:170-193), and the transform back
 * along x + p with its x halo + Pres_2::output (src/fft.cxx:540-583, src/pres_2.cxx:333-387) read straight from segment c of the
 * receive buffer of Transpose::exec_yx. They replace mhh_pres_input_packed + fwd_x_pack_chunk and bwd_x_chunk +
 * unpack_output_slab; the y stage, the one-row halo of p and mhh_pres_output_south_row stay.
 * Same tolerance as the staged form (different transforms, not the same bits). */
int mhh_pres_slab_has_lds(const mhh_pres_slab_plan* plan);
int mhh_pres_slab_lds_fwd(mhh_pres_slab_plan* plan, const mhh_grid* g, const mhh_fields* f, double dt, void* sendbuf, int c, void* stream);
int mhh_pres_slab_lds_bwd(mhh_pres_slab_plan* plan, const mhh_grid* g, const void* recvbuf, const mhh_fields* f, int c, void* stream);
/* the y stage of that form: the all-to-all buffers are laid out [slice][peer][k][kxl][row] (rows fastest: a column's rows from one rank
 * are one run), so the transforms along y read / write them directly (src/fft.cxx:499-538) around the Thomas sweeps (mhh_pres_solve_y).
 * Call order per solve: for c: lds_fwd(c) -> all-to-all(c);  for c: lds_fwd_y(c);  solve_y;  for c: lds_bwd_y(c) -> all-to-all(c);
 * for c: lds_bwd(c);  p halo (one row);  output_south_row. */
int mhh_pres_slab_lds_fwd_y(mhh_pres_slab_plan* plan, const mhh_grid* g, void* recvbuf, int c, void* stream);
int mhh_pres_slab_lds_bwd_y(mhh_pres_slab_plan* plan, const mhh_grid* g, void* sendbuf, int c, void* stream);

/* ---- Field3d_operators: horizontal means, deterministic ---------------------------------------------------------
 * Two kernels per call and no floating-point atomics: a 64 x 4 block sums one level's cells of a chunk of
 * mhh_field_mean_chunk_rows() rows in a fixed order into ONE double partial of scratch[field][k][chunk]; a second kernel
 * adds the partials in index order. Two calls on the same input give the same bits. `scratch` is the caller's: device
 * memory of mhh_field_mean_scratch_elems(g, nfields) DOUBLES. Up to 3 + MHH_MAX_SCALARS fields per call.               */
#define MHH_MAX_MEAN_FIELDS (3 + MHH_MAX_SCALARS)
unsigned long long mhh_field_mean_scratch_elems(const mhh_grid* g, int nfields);
int mhh_field_mean_chunk_rows(void);
/* Field3d_operators::calc_mean_profile (src/field3d_operators.cxx:45-66): for every level k in [0, kcells) the interior (i, j)
 * cells summed in double, profs[n][k] = TF(sum / (itot*jtot)). The divisor is the GLOBAL itot*jtot: a slab rank produces its
 * share and the caller sums the shares over the ranks (the reference's master.sum after the division).                    */
int mhh_field_mean_profile(const mhh_grid* g, const void* const* fields, int nfields, void* const* profs /* TF [kcells] each */,
                           void* scratch, void* stream);
/* The sum of Field3d_operators::calc_mean (src/field3d_operators.cxx:132-155): fld[ijk]*dz[k] formed in TF, accumulated in
 * double over the interior; sums[n] (DEVICE doubles) receives this rank's sum. The quotient by itot*jtot*zsize (formed in
 * TF, :152) is taken where the sum is consumed (mhh_force_params::uflux_sums), so that a slab rank can all-reduce first.  */
int mhh_field_mean_sum(const mhh_grid* g, const void* const* fields, int nfields, void* sums /* double [nfields] */,
                       void* scratch, void* stream);

/* ---- Buffer: the sponge layer (src/buffer.cxx:37-58,163-206) -----------------------------------------------------
 * at[ijk] -= sigmaz[k]*(a[ijk] - abuf[k]) for u, v, every scalar (k in [bufferkstart, kend), table sigma) and w
 * (k in [bufferkstarth, kend), half-level table sigmah). One launch over the buffer levels only. A zero-initialised
 * struct (swbuffer = 0) is a no-op.                                                                                 */
typedef struct mhh_buffer_params
{
    int swbuffer;
    int bufferkstart, bufferkstarth;         /* Buffer::create (src/buffer.cxx:107-126)                            */
    const void* sigma;                       /* [kcells] device tables from mhh_buffer_sigma_host                  */
    const void* sigmah;
    /* [kcells] device profiles per field: the fixed bufferprofs, or the mean profiles (swupdate); NULL = field left alone */
    const void* abuf_u; const void* abuf_v; const void* abuf_w;
    const void* abuf_s[MHH_MAX_SCALARS];
} mhh_buffer_params;
/* sigmaz[k] = sigma*pow((z[k]-zstart)/(zsize-zstart), beta) in the grid's dtype with the HOST C library's pow (powf in fp32,
 * as the reference calls std::pow of TF, src/buffer.cxx:48); z = zh with half_level. `g_host` carries HOST metric pointers.
 * Levels outside [kstart, kend) or below zstart get 0 (the kernels never read them).                                   */
int mhh_buffer_sigma_host(const mhh_grid* g_host, double zstart, double sigma, double beta, int half_level, void* out_host);
int mhh_buffer_exec(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, void* stream);

/* ---- Force (src/force.cxx:46-311,581-729) ------------------------------------------------------------------------
 * One launch; per field the terms apply to each cell in the reference's order -- pressure force, swls, swwls, nudging --
 * so a tendency has the bits of the separate reference loops run in sequence. Profiles are [kcells] DEVICE arrays of the
 * grid's dtype. A zero-initialised struct is a no-op. rescale_nudgeprof (scalednudgelist) edits a host profile: the
 * caller's, before the upload. w has no ls_ / nudge_ slot: the large-scale source and the nudging act on u, v and the
 * scalars only (the reference takes any prognostic name in lslist / nudgelist; w reaches this pass through the sponge
 * and through swwls = local with swwls_mom).                                                                         */
#define MHH_LSPRES_NONE  0
#define MHH_LSPRES_DPDX  1   /* add_pressure_force :47-60, ut += -dpdx                                              */
#define MHH_LSPRES_UFLUX 2   /* enforce_fixed_flux :63-74                                                           */
#define MHH_LSPRES_GEO   3   /* calc_coriolis_2nd / _4th :77-151                                                    */
#define MHH_WLS_NONE  0
#define MHH_WLS_MEAN  1      /* advec_wls_2nd_mean :203-235 (Large_scale_subsidence_type::Mean_field)               */
#define MHH_WLS_LOCAL 2      /* advec_wls_2nd_local / _local_w :237-305 (Local_field)                               */
typedef struct mhh_force_params
{
    int swlspres;
    int order;                               /* geo: 2 | 4 (grid.swspatialorder); 4 needs igc >= 2 and jgc >= 2     */
    double dpdx;
    double uflux, dt;                        /* uflux: dt is narrowed to the grid's dtype first, as the reference's const TF dt */
    const void* uflux_sums;                  /* DEVICE double[2]: GLOBAL sums of u*dz and ut*dz (mhh_field_mean_sum)  */
    double fc, utrans, vtrans;               /* geo: fc, grid.utrans, grid.vtrans                                   */
    const void* ug; const void* vg;
    int swls;                                /* calc_large_scale_source :153-169: at += ls[k] where ls_* != NULL     */
    const void* ls_u; const void* ls_v; const void* ls_s[MHH_MAX_SCALARS];
    int swwls, swwls_mom;                    /* every scalar; with swwls_mom also u, v (and w in the local form)     */
    const void* wls;
    /* horizontal mean profiles (mhh_field_mean_profile, summed over the ranks): read by swwls = mean and by the nudging */
    const void* mean_u; const void* mean_v; const void* mean_s[MHH_MAX_SCALARS];
    int swnudge;                             /* calc_nudging_tendency :171-191 where nudge_* != NULL                 */
    const void* nudge_factor;
    const void* nudge_u; const void* nudge_v; const void* nudge_s[MHH_MAX_SCALARS];
} mhh_force_params;
int mhh_force_exec(const mhh_grid* g, const mhh_fields* f, const mhh_force_params* p, void* stream);
/* buffer->exec then force->exec (src/model.cxx:395,404) as ONE read-modify-write of every tendency: the same kernel with
 * both term groups compiled in; the bits of mhh_buffer_exec followed by mhh_force_exec.                                */
int mhh_buffer_force_exec(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, const mhh_force_params* p, void* stream);

/* ---- Vertical ghost cells --------------------------------------------------------------
 * Boundary::set_ghost_cells: calc_ghost_cells_{bot,top}_{2nd,4th} (src/boundary.cxx:686-836); bc 0 = Dirichlet
 * (abot/atop), 1 = Neumann or flux (agradbot/agradtop), -1 = that side is left alone (what the reference's kernels do for
 * Ustar_type, which matches neither of their branches); 2-D arrays are [ijcells]. set_ghost_cells_w (4th order
 * only): type 0 = Normal (:874-907), 1 = Conservation (:838-871).                                              */
int mhh_boundary_ghost_cells(const mhh_grid* g, int order, void* a, int bcbot, int bctop,
                             const void* abot, const void* agradbot, const void* atop, const void* agradtop, void* stream);
int mhh_boundary_ghost_cells_w(const mhh_grid* g, void* w, int type, void* stream);

/* ---- Boundary_surface: the Monin-Obukhov surface layer (src/boundary_surface.cxx:830-983) ---------------------------
 * The device form of Boundary_surface<TF>::exec with the lookup solver (swconstantz0 = true, the default):
 *   mbcbot Dirichlet (noslip), thermo bc Flux      : stability case 2 (:94-112)
 *   mbcbot Dirichlet (noslip), thermo bc Dirichlet : stability case 3 (:113-133)
 *   mbcbot Ustar,              thermo bc Flux      : stability case 1 (:83-92), surfm's Ustar branch (:222-252)
 *   thermo_kind 0 (switch "0"), either mbcbot      : stability_neutral (:137-177)
 * Refused with MHH_EINVAL and a text that names the reason: swconstantz0 = 0 (the iterative solvers of
 * include/boundary_surface_kernels.h:287-470), swcharnock, and a grid with igc < 2 or jgc < 2 (calc_dutot reads u[i+2], v[j+2]).
 * It WRITES the 2-D arrays of mhh_fields that the operators read: u_fluxbot, v_fluxbot, s_fluxbot[n] (Dirichlet scalars), dudz,
 * dvdz, dbdz. Their `const` in mhh_fields is the operators' view; the surface layer is their producer. zsl = g->z[kstart].
 * 2-D arrays are [ijcells] of the grid's dtype unless stated. Every call only enqueues on `stream`.                          */
#define MHH_BC_DIRICHLET 0   /* Boundary_type::Dirichlet_type: the surface value is given (mbcbot = noslip)                  */
#define MHH_BC_NEUMANN   1   /* Neumann_type: surfs leaves such a scalar alone                                               */
#define MHH_BC_FLUX      2   /* Flux_type: the surface flux is given                                                         */
#define MHH_BC_USTAR     3   /* Ustar_type (momentum only): the friction velocity is given                                   */
#define MHH_THERMO_NONE  0
#define MHH_THERMO_DRY   1   /* Thermo_dry: calc_buoyancy_bot / calc_buoyancy_fluxbot / get_db_ref (src/thermo_dry.cxx:133-162,629-633) */
#define MHH_THERMO_BUOY  2   /* Thermo_buoy: plain copies, db_ref = bg_n2 (src/thermo_buoy.cxx:425-448, include/thermo_buoy.h:66)      */
#define MHH_THERMO_MOIST 3   /* Thermo_moist: calc_buoyancy_bot / calc_buoyancy_fluxbot / get_db_ref (src/thermo_moist.cxx:637-693,1713-1717) */
#define MHH_SURFACE_NZL  10000   /* nzL_lut (include/boundary.h:55) */
typedef struct mhh_surface_params
{
    int mbcbot;                              /* MHH_BC_DIRICHLET | MHH_BC_USTAR                                             */
    int thermobc;                            /* boundary type of the thermo scalar: == sbcbot[thermo_index]                 */
    int thermo_kind, thermo_index;           /* MHH_THERMO_*; the scalar that is th (dry) or b (buoy)                       */
    int swconstantz0;                        /* must be 1: the lookup solver                                                */
    int swcharnock;                          /* must be 0                                                                   */
    double thref_kstart, threfh_kstart, grav;/* Thermo_dry: bs.thref[kstart], bs.threfh[kstart], Constants::grav            */
    double bg_n2;                            /* Thermo_buoy: bs.n2, what its get_db_ref returns                             */
    const void* zL; const void* f;           /* float [MHH_SURFACE_NZL] device tables from mhh_surface_lut_host             */
    const void* z0m; const void* z0h;
    void* ustar; void* obuk;                 /* state: init_surface sets obuk = 1e-9 (dsmall), ustar = 1e-2 (:565-570)       */
    void* nobuk;                             /* int [ijcells]: the table index each column's walk starts from; 0 at first   */
    const void* ubot; const void* vbot;      /* fld_bot of u, v                                                             */
    void* ugradbot; void* vgradbot;          /* grad_bot of u, v: input of mhh_boundary_ghost_cells                         */
    void* sbot[MHH_MAX_SCALARS];             /* fld_bot per scalar: read (Dirichlet) or written (Flux)                      */
    void* sgradbot[MHH_MAX_SCALARS];         /* grad_bot per scalar                                                         */
    int   sbcbot[MHH_MAX_SCALARS];           /* sbc.at(name).bcbot                                                          */
    /* Thermo_moist (thermo_kind 3): thermo_index is thl, qt_index is qt, which must have thl's kind of bc. thvref, thvrefh are the
     * DEVICE base-state tables [kcells], read at kstart when the kernels run: the base state moves on the device every sub-step.
     * Zero-initialised: unused.                                                                                             */
    int   qt_index;
    const void* thvref; const void* thvrefh;
} mhh_surface_params;
/* prepare_lut (include/boundary_surface_kernels.h:78-133) on the HOST with the host C library, as Boundary_surface::init_solver
 * runs it (:812-826): zL_out, f_out are HOST float[MHH_SURFACE_NZL] for both dtypes, the temporaries are in the dtype. A pair
 * (mbcbot, thermobc) without a table (Ustar) leaves f_out zero.                                                            */
int mhh_surface_lut_host(double zsl, double z0m, double z0h, int mbcbot, int thermobc, int dtype, float* zL_out, float* f_out);
/* The stages one by one, so that a test can isolate them. None of them fills ghost cells.
 * dutot: calc_dutot on the interior (include/boundary_surface_kernels.h:136-180), without its exec_2d                      */
int mhh_surface_dutot(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* dutot, void* stream);
/* stability / stability_neutral (src/boundary_surface.cxx:54-177) over all cells from a filled dutot, with Thermo's
 * get_buoyancy_surf / get_buoyancy_fluxbot / get_db_ref evaluated inline: writes obuk, ustar, nobuk                        */
int mhh_surface_stability(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, const void* dutot, void* stream);
/* surfm (:180-288): u_fluxbot, v_fluxbot on the interior (without their exec_2d), ugradbot, vgradbot on all cells          */
int mhh_surface_momentum(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* stream);
/* surfs (:291-339) for scalar n, all cells                                                                                 */
int mhh_surface_scalar(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, int n, void* stream);
/* calc_duvdz_mo, calc_dbdz_mo (include/boundary_surface_kernels.h:186-243), interior; dbdz unless thermo_kind == 0         */
int mhh_surface_mo_gradients(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* stream);
/* Boundary_surface<TF>::exec (:830-983): three kernels and three 2-D cyclic fills (dutot, u_fluxbot, v_fluxbot); the bits of
 * dutot, fill, stability, momentum, scalar (each n), mo_gradients, fill, fill. `scratch` = [ijcells] of the dtype: dutot.
 * One rank only: on a slab (npy > 1) the north-south rows of dutot, u_fluxbot and v_fluxbot are the caller's exchange between
 * the stages, so the fused call returns MHH_EINVAL there and the driver calls the stages.                                  */
int mhh_boundary_surface_exec(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* scratch, void* stream);

/* ---- Thermo_moist (src/thermo_moist.cxx, include/thermo_moist_functions.h; GPU src/thermo_moist.cu) --------------------------
 * thl and qt are two scalars of the grid's dtype; pref, prefh, exnref, exnrefh, thvref, thvrefh, rhoref, rhorefh are the base-state
 * profiles, [kcells] device tables. `nonconv` is an int counter in device memory (NULL: none): where the reference throws
 * "Non-converging saturation adjustment" (niter == nitermax, thermo_moist_functions.h:277-288) the device neither traps nor prints;
 * the cell finishes with its tenth iterate and adds one to the counter. Every entry only enqueues on its stream.
 *
 * get_thermo_field("N2") needs no entry of its own: calc_N2 (src/thermo_moist.cxx:460-475) is the dry expression with thvref in the
 * place of thref, i.e. mhh_diff_params with buoyancy_kind = 0, th_for_N2 = the index of thl, thref = thvref, buoyancy = 0.
 * The warm branch of sat_adjust holds + - * /, max and fabs only and is bit-identical to the reference; the cold branch passes
 * through exp (esat_ice) and the base state through pow and exp, which differ between C libraries in the last bits.            */
#define MHH_MOIST_IMPL_MARCH 0   /* one thread per column marching up in k: four array passes                                   */
#define MHH_MOIST_IMPL_CELL  1   /* one thread per cell through the generic cell kernel: six array passes, the same bits (A/B)  */
/* sat_adjust (thermo_moist_functions.h:186-291) on n independent cells; thl, qt, p, exn and the outputs are [n] device arrays of
 * dtype MHH_F64 / MHH_F32; an output may be NULL.                                                                                */
int mhh_thermo_moist_sat_adjust(int dtype, long long n, const void* thl, const void* qt, const void* p, const void* exn,
                                void* ql, void* qi, void* t, void* qs, int* nonconv, void* stream);
/* Thermo_moist::exec at second order, calc_buoyancy_tend_2nd (src/thermo_moist.cxx:78-120; GPU calc_buoyancy_tend_2nd_g,
 * src/thermo_moist.cu): wt[k] += buoyancy(exnrefh[k], thl and qt at the w level, their ql and qi, thvrefh[k]) for k in (kstart, kend).
 * exnrefh[k] is read from the table; the reference recomputes exner(prefh[k]), the expression that filled it. Run in front of
 * mhh_rhs_exec, as thermo->exec precedes advec->exec. The levels per chunk of the marching form follow MHH_MARCH_KC_RT.          */
int mhh_thermo_moist_buoyancy_tend(const mhh_grid* g, void* wt, const void* thl, const void* qt, const void* prefh,
                                   const void* exnrefh, const void* thvrefh, int* nonconv, void* stream);
/* the same with the form named (MHH_MOIST_IMPL_*)                                                                               */
int mhh_thermo_moist_buoyancy_tend_impl(const mhh_grid* g, int impl, void* wt, const void* thl, const void* qt, const void* prefh,
                                        const void* exnrefh, const void* thvrefh, int* nonconv, void* stream);
/* Thermo_moist::get_thermo_field for "b", "ql", "qi", "T" (calc_buoyancy :123-167, calc_liquid_water :231-250, calc_ice :414-434,
 * calc_T :478-496) in one pass with one sat_adjust per cell: writes whichever of b, ql, qi, T is not NULL. ql, qi, T on the
 * interior; b on all kcells levels of the interior columns, with ql = qi = 0 outside [kstart, kend).                             */
int mhh_thermo_moist_fields(const mhh_grid* g, const void* thl, const void* qt, const void* pref, const void* exnref, const void* thvref,
                            void* b, void* ql, void* qi, void* T, int* nonconv, void* stream);
/* get_thermo_field("ql_h"): calc_liquid_water_h (:368-411), what the ql mask of Thermo_moist::get_mask (:1314-1329) thresholds on
 * the half levels. thl and qt interpolated to the half level and the per-cell saturation adjustment at prefh, exnrefh: levels
 * kstart+1 .. kend of the interior columns (kend reads the ghost level of thl and qt), zero at kstart.                            */
int mhh_thermo_moist_ql_h(const mhh_grid* g, const void* thl, const void* qt, const void* prefh, const void* exnrefh, void* ql_h,
                          int* nonconv, void* stream);
/* Thermo_moist::create_basestate (:1220-1241) on the HOST with the host's C library: calc_top_and_bot (:58-75) sets the ghost
 * entries of thl0 and qt0 (HOST [kcells], written), calc_base_state (thermo_moist_functions.h:293-349) fills the eight HOST
 * profiles (any may be NULL), and with boussinesq != 0 rhoref, rhorefh are overwritten with 1 and thvref, thvrefh with thvref0.
 * g_host carries HOST metric pointers. nonconv: HOST int, incremented.                                                          */
int mhh_thermo_moist_base_state_host(const mhh_grid* g_host, void* thl0, void* qt0, double pbot, int boussinesq, double thvref0,
                                     void* pref, void* prefh, void* rhoref, void* rhorefh, void* thvref, void* thvrefh,
                                     void* exnref, void* exnrefh, int* nonconv);
/* calc_base_state on the device from the mean profiles thlmean, qtmean ([kcells], ghost entries set), statement by statement, by
 * one lane on the stream: no synchronisation, no host memory (the reference's GPU path copies the means to the host every
 * sub-step, src/thermo_moist.cu:806-844). Any output may be NULL.                                                                */
int mhh_thermo_moist_base_state(const mhh_grid* g, const void* thlmean, const void* qtmean, double pbot,
                                void* pref, void* prefh, void* rhoref, void* rhorefh, void* thvref, void* thvrefh,
                                void* exnref, void* exnrefh, int* nonconv, void* stream);

/* ---- Microphys_2mom_warm (src/microphys_2mom_warm.cxx; Seifert & Beheng 2006, Stevens & Seifert 2008) and Limiter (src/limiter.cxx)
 * Four scalars of the grid's dtype: thl, qt, qr (rain water specific humidity) and nr (rain drop number density), with their
 * tendencies. rhoref, pref, exnref are [kcells] device tables (Thermo_moist's base state); ql is not an input: it is
 * get_thermo_field("ql_qi"), max(qt - sat_adjust(thl, qt, pref[k], exnref[k]).qs, 0), evaluated per cell, and `nonconv` counts as in
 * Thermo_moist. Column-local: nothing is read across a cell's column, so a slab rank needs no exchange. Every entry but the CFL
 * number only enqueues on its stream.                                                                                            */
#define MHH_MICRO_AUTO  1    /* autoconversion (:94-128)                                                  */
#define MHH_MICRO_ACCR  2    /* accretion (:131-158)                                                       */
#define MHH_MICRO_EVAP  4    /* evaporation (:278-318)                                                     */
#define MHH_MICRO_SCBR  8    /* selfcollection and breakup (:321-370)                                      */
#define MHH_MICRO_SEDI  16   /* sedimentation_ss08 (:373-539)                                              */
#define MHH_MICRO_CLIP  32   /* remove_negative_values on qr and nr (:51-64), interior, in place           */
#define MHH_MICRO_ALL   63
typedef struct mhh_micro_params
{
    double Nc0;        /* the fixed cloud droplet number [m-3] (micro.Nc0)                                                   */
    double dt;         /* the FULL time step, timeloop->get_dt(): sedimentation's CFL numbers and its limiter use it         */
    int processes;     /* mask of MHH_MICRO_*: all of them is Microphys_2mom_warm::exec; one process into zeroed tendencies
                          is a term of the swmicrobudget statistics (:831-925)                                                */
} mhh_micro_params;
#define MHH_MICRO_IMPL_MARCH 0   /* the local processes and the CFL numbers / slopes by one thread per column marching up in k */
#define MHH_MICRO_IMPL_CELL  1   /* the same by one thread per cell and level (three levels of w recomputed): the same bits (A/B) */
/* Microphys_2mom_warm::exec (:639-752). qr and nr are WRITTEN with MHH_MICRO_CLIP; their vertical ghost levels (kstart-1, kend) are
 * read by the slopes and must be set. Per cell the tendencies take autoconversion, accretion, evaporation, selfcollection, breakup,
 * then the sedimentation flux divergence. rr_bot: [ijcells], the surface rain rate -flux_qr[kstart] [kg m-2 s-1], written on the
 * interior with MHH_MICRO_SEDI. scratch: a HOST array of four device pointers, each to kcells * ijcells elements of the dtype
 * (sedimentation's CFL numbers and slopes of qr and nr: four tmp fields); may be NULL without MHH_MICRO_SEDI. The levels per chunk of the marching form follow MHH_MARCH_KC_RT.                             */
int mhh_micro_2mom_warm_exec(const mhh_grid* g, const mhh_micro_params* params, void* qr, void* nr, const void* thl, const void* qt,
                             void* qrt, void* nrt, void* thlt, void* qtt, void* rr_bot, const void* rhoref, const void* pref,
                             const void* exnref, void* const* scratch, int* nonconv, void* stream);
/* the same with the form named (MHH_MICRO_IMPL_*)                                                                               */
int mhh_micro_2mom_warm_exec_impl(const mhh_grid* g, int impl, const mhh_micro_params* params, void* qr, void* nr, const void* thl, const void* qt,
                                  void* qrt, void* nrt, void* thlt, void* qtt, void* rr_bot, const void* rhoref, const void* pref,
                                  const void* exnref, void* const* scratch, int* nonconv, void* stream);
/* calc_max_sedimentation_cfl (:163-234): the largest sedimentation CFL number of qr for the step dt, at least 1e-5; its velocity
 * has no density correction and is mirrored over both ghost levels. work: mhh_reduce_work_bytes() of device memory. Synchronises
 * the stream (the result is a host number), as mhh_advec_cfl does.                                                              */
int mhh_micro_2mom_warm_cfl(const mhh_grid* g, const void* qr, const void* nr, const void* rhoref, double dt, void* work, double* out, void* stream);
/* Limiter::tendency_limiter (src/limiter.cxx:54-75): at += (a + dt*at < 0) ? (-(a + dt*at) + eps)/dt : 0 on the interior, eps the
 * double epsilon narrowed to the dtype; dt is the sub-step (src/model.cxx:415).                                                  */
int mhh_limiter_exec(const mhh_grid* g, void* at, const void* a, double dt, void* stream);

/* ---- Microphys_nsw6 (src/microphys_nsw6.cxx; Tomita 2008, the single-moment six-class ice scheme; swmicro = nsw6) ----------------
 * Five scalars of the grid's dtype: thl, qt, qr (rain), qs (snow), qg (graupel), with their tendencies; no field is written.
 * rhoref, pref, exnref are [kcells] device tables (Thermo_moist's base state). Column-local: a slab rank needs no exchange. Every
 * entry but the CFL number only enqueues on its stream. params is mhh_micro_params: Nc0, dt (the FULL step) and a mask of:       */
#define MHH_NSW6_CONV   1    /* conversion (:125-650): the 25 process rates folded into 15 transfers between the six classes  */
#define MHH_NSW6_SEDI_R 2    /* sedimentation_ss08 (:686-825) of rain                                                        */
#define MHH_NSW6_SEDI_S 4    /* ... of snow                                                                                  */
#define MHH_NSW6_SEDI_G 8    /* ... of graupel                                                                               */
#define MHH_NSW6_ALL    15
/* the two forms of the powers of the slope parameters (A/B): std::pow wherever the reference has it, or none at all: b = 3 makes
 * lambda a fourth root and every other exponent a multiple of 1/8, so square roots and products do. Every std::tgamma of the file
 * and D_d (:139) are evaluated on the host in the dtype in both forms.                                                          */
#define MHH_NSW6_POW  0
#define MHH_NSW6_SQRT 1
#define MHH_NSW6_IMPL_DEFAULT MHH_NSW6_SQRT
/* Microphys_nsw6::exec (:983-1073): conversion, then the sedimentation of rain, snow and graupel. ql, qi: get_thermo_field("ql")
 * and ("qi") as the reference's function takes them, or BOTH NULL: then sat_adjust(thl, qt, pref[k], exnref[k]) runs per cell and
 * `nonconv` counts as in Thermo_moist. The vertical ghost levels (kstart-1, kend) of qr, qs, qg are read by the slopes and must be
 * set. r?_bot: [ijcells], the surface rates -flux[kstart] [kg m-2 s-1], written on the interior by the species' sedimentation.
 * scratch: a HOST array of six device pointers, each to kcells * ijcells elements of the dtype (CFL numbers and slopes: scratch[2s],
 * scratch[2s+1] of species s = 0 rain, 1 snow, 2 graupel); only those of the species in the mask are read.                        */
int mhh_micro_nsw6_exec(const mhh_grid* g, const mhh_micro_params* params, const void* qr, const void* qs, const void* qg, const void* thl,
                        const void* qt, const void* ql, const void* qi, void* qrt, void* qst, void* qgt, void* thlt, void* qtt, void* rr_bot,
                        void* rs_bot, void* rg_bot, const void* rhoref, const void* pref, const void* exnref, void* const* scratch, int* nonconv,
                        void* stream);
/* the same with the form named (MHH_NSW6_POW, MHH_NSW6_SQRT)                                                                     */
int mhh_micro_nsw6_exec_impl(const mhh_grid* g, int impl, const mhh_micro_params* params, const void* qr, const void* qs, const void* qg,
                             const void* thl, const void* qt, const void* ql, const void* qi, void* qrt, void* qst, void* qgt, void* thlt, void* qtt,
                             void* rr_bot, void* rs_bot, void* rg_bot, const void* rhoref, const void* pref, const void* exnref,
                             void* const* scratch, int* nonconv, void* stream);
/* The largest of the three calc_cfl_ss08 of get_time_limit (:1119-1177) for the step dt, at least 1e-5 (a double, :1174). work:
 * mhh_reduce_work_bytes() of device memory. Synchronises the stream (the result is a host number), as mhh_advec_cfl does.        */
int mhh_micro_nsw6_cfl(const mhh_grid* g, const void* qr, const void* qs, const void* qg, const void* rhoref, double dt, void* work, double* out,
                       void* stream);
int mhh_micro_nsw6_cfl_impl(const mhh_grid* g, int impl, const void* qr, const void* qs, const void* qg, const void* rhoref, double dt, void* work,
                            double* out, void* stream);

/* ---- Radiation_gcss (src/radiation_gcss.cxx: the GCSS long- and short-wave fluxes of DYCOMS-II, swradiation = gcss) -------------
 * The parity target is the reference's CPU path; its CUDA file (src/radiation_gcss.cu) differs from it in physics (no max(0, .),
 * dz for z[k]-z[k-1], lwp subtracted on the way up, the flux difference shifted by a level). Column-local: a slab rank exchanges
 * nothing. The fluxes need ql, thl's tendency takes their vertical difference. What looks like a slip in the reference is kept
 * (csrc/cell_ops.h names each with its line). Every entry but the zenith angle only enqueues on its stream, so a sub-step with it
 * still captures into a graph; `mu` is a HOST number fixed at capture, as dt is for the microphysics: re-capture when the sun moved. */
#define MHH_RAD_LW 1      /* the long-wave term of thlt (calc_gcss_rad_LW :203-252, the tendency :273-285)                       */
#define MHH_RAD_SW 2      /* the short-wave term (calc_gcss_rad_SW + sunray :101-200, :287-308); applied only where mu > 0.035 in the dtype */
typedef struct mhh_radiation_gcss_params
{
    double xka, fr0, fr1, div;   /* radiation.xka, fr0, fr1, div (:317-320): narrowed to the dtype on entry, the members are TF   */
    double mu;                   /* the cosine of the zenith angle, from mhh_radiation_gcss_zenith_host; narrowed likewise       */
    int parts;                   /* MHH_RAD_LW | MHH_RAD_SW: the terms thlt takes; both is Radiation_gcss::exec                    */
} mhh_radiation_gcss_params;
#define MHH_RAD_IMPL_SWEEP 0   /* one kernel, an upward and a downward sweep per column, one scratch field between them          */
#define MHH_RAD_IMPL_PLAIN 1   /* the reference's sequence: a column kernel per flux array, a cell kernel for thlt: the same bits (A/B) */
/* calc_zenith (:39-76) with the host's C library in the dtype; day_of_year as Timeloop::calc_day_of_year gives it (the day of the
 * year counted from 1, plus the fraction of the day: 2001-06-09 00:00 UTC is 160.0).                                              */
int mhh_radiation_gcss_zenith_host(int dtype, double lat, double lon, double day_of_year, double* mu);
/* Radiation_gcss::exec (:353-379: exec_gcss_rad :253-309) and get_radiation_field (:392-436) in one call.
 * thlt: the tendency of thl, interior levels kstart+1 .. kend-1 (NULL: fields only). ql: [ncells] (NULL: it is
 * get_thermo_field("ql") of thl, qt, pref, exnref, written to scratch[0]; `nonconv` counts as in Thermo_moist). lflx, sflx:
 * get_radiation_field("lflx" / "sflx"), either may be NULL; lflx is written on the interior, sflx on the interior over a zero fill
 * of all ncells, and stays all zero at night (mu <= 0.035). Both are formed whatever `parts` says. scratch: a HOST array of two
 * device pointers to ncells elements of the dtype each (two tmp fields; the reference's CPU path takes four).                      */
int mhh_radiation_gcss_exec(const mhh_grid* g, const mhh_radiation_gcss_params* params, void* thlt, const void* ql, const void* thl,
                            const void* qt, const void* rhoref, const void* pref, const void* exnref, void* lflx, void* sflx,
                            void* const* scratch, int* nonconv, void* stream);
/* the same with the form named (MHH_RAD_IMPL_*)                                                                                  */
int mhh_radiation_gcss_exec_impl(const mhh_grid* g, int impl, const mhh_radiation_gcss_params* params, void* thlt, const void* ql, const void* thl,
                                 const void* qt, const void* rhoref, const void* pref, const void* exnref, void* lflx, void* sflx,
                                 void* const* scratch, int* nonconv, void* stream);

/* ---- Stats (src/stats.cxx: the sampling of second-order cases; the parity target is the reference's CPU path) --------------------
 * Masks live in ONE unsigned int field mfield [ncells] and a 2-D mfield_bot [ijcells]; mask n (0 .. MHH_STATS_MAX_MASKS-1, in the
 * order of add_mask, :841-850) has flag = 1 << 2n on full levels and flagh = 1 << (2n+1) on half levels. Every reduction is
 * deterministic (chunk partials, then an ordered finish: no floating-point atomics) and is split into a SUMS call that leaves
 * doubles in device memory and a FINISH call that turns them into values of the grid's dtype, so that a slab rank can add sums
 * and counts over the ranks in between. Every entry only enqueues on its stream. `scratch`: device memory of
 * mhh_stats_scratch_elems(g, nmasks, njobs) DOUBLES. One vertical ghost level is required (the profiles read kend and kstart-1). */
#define MHH_STATS_MAX_MASKS 8
#define MHH_STATS_MAX_JOBS  16
#define MHH_STATS_MASK_PLUS 0   /* Stats_mask_type::Plus: a cell leaves the mask where value <= threshold                            */
#define MHH_STATS_MASK_MIN  1   /* Stats_mask_type::Min:  ... where value > threshold                                               */
#define MHH_STATS_MEAN     0    /* calc_mean (:263-287); also the mean of w under flagh and calc_tend (:1893-1919)                 */
#define MHH_STATS_MOMENT2  2    /* calc_moment (:341-365), power 2, 3, 4: needs `mean`                                             */
#define MHH_STATS_MOMENT3  3
#define MHH_STATS_MOMENT4  4
#define MHH_STATS_FRAC     5    /* calc_frac (:410-433)                                                                            */
#define MHH_STATS_GRAD     6    /* calc_grad_2nd (:2171-2195): averaged under the flag of the OTHER level (!fld.loc[2])            */
#define MHH_STATS_COUNT    7    /* calc_nmask (:224-261) over 0 .. kcells; used by mhh_stats_mask_count                            */
#define MHH_STATS_MEAN2D   8    /* calc_mean_2d (:289-306): fld is [ijcells], no mask, the value is element 0 of the profile      */
#define MHH_STATS_FLUX_W    9   /* the resolved flux (:1668-1733): advec.get_advec_flux of fld - mean[k] and w - wmean[k], evaluated on the
                                 * fly: advec_flux_u / _v / _s of advec_2 (src/advec_2.cxx:206-252) and advec_2i5 (src/advec_2i5.cxx:730-913),
                                 * advec_flux_s_lim (include/advec_monotonic.h:183); averaged under flagh; needs `mean`, `w`, `wmean`    */
#define MHH_STATS_FLUX_DIFF 10  /* the diffusive flux (:1735-1760): Diff_smag2::diff_flux (src/diff_smag2.cxx:739-842, :1217-1276) and
                                 * Diff_2::diff_flux (src/diff_2.cxx:88-105); averaged under flagh                                    */
#define MHH_STATS_FLUX_SUM  11  /* add_fluxes (:400-407) in the finish: the finished values of jobs a and b of the same call, added   */
typedef struct mhh_stats_job
{
    const void* fld;             /* the variable, [ncells] of the grid's dtype ([ijcells] for MEAN2D)                               */
    const void* mean;            /* moments: the FINISHED mean profiles of the variable, [nmasks][kcells] (offset and fill included,
                                  * as calc_moment reads profs.at(varname)); NULL otherwise                                         */
    int loc;                     /* fld.loc[2]: 0 full level, 1 half level                                                           */
    int op;                      /* MHH_STATS_*                                                                                      */
    double offset, threshold;    /* narrowed to the dtype on entry                                                                   */
    /* the fluxes only (MHH_STATS_FLUX_*); a full-level variable: a half-level one is refused, as the reference throws             */
    int kind;                    /* where the variable lives horizontally: 0 scalar, 1 u, 2 v (fld.loc[0], fld.loc[1])                */
    int scheme;                  /* FLUX_W: MHH_ADVEC_2 | MHH_ADVEC_2I5; FLUX_DIFF: MHH_DIFF_2 | MHH_DIFF_SMAG2                       */
    int limit;                   /* FLUX_W of a scalar in advec.fluxlimit_list: advec_flux_s_lim                                      */
    int surface_model;           /* FLUX_DIFF, smag2: boundary.get_switch() != "default": flux_bot / flux_top on the two boundary levels */
    const void* w;               /* FLUX_W, and FLUX_DIFF of u and v with smag2: the vertical velocity [ncells]                       */
    const void* wmean;           /* FLUX_W: calc_mean of w under flagh, [nmasks][kcells] (a MEAN job of w with loc 1, offset 0)       */
    const void* evisc;           /* FLUX_DIFF, smag2                                                                                 */
    const void* flux_bot; const void* flux_top;   /* FLUX_DIFF, smag2 with a surface model: [ijcells]                                */
    double visc, tPr;            /* FLUX_DIFF: the variable's visc (fields.visc for u and v), diff.tPr                                */
    int a, b;                    /* FLUX_SUM: the jobs of THIS call that hold _w and _diff                                            */
} mhh_stats_job;
unsigned long long mhh_stats_scratch_elems(const mhh_grid* g, int nmasks, int njobs);
int mhh_stats_chunk_rows(void);
/* Stats::initialize_masks (:1214-1227): every word of both fields, ghosts included, is the sum of the flags of nmasks masks        */
int mhh_stats_mask_init(const mhh_grid* g, void* mfield, void* mfield_bot, int nmasks, void* stream);
/* Stats::set_mask_thres / calc_mask_thres (:95-172, :1264-1301), all six loops; fld, fldh [ncells], fld_bot [ijcells]. Integer
 * logic: a bit whose test fails is cleared; NaN fails neither test and clears nothing.                                            */
int mhh_stats_mask_thres(const mhh_grid* g, void* mfield, void* mfield_bot, int mask, const void* fld, const void* fldh, const void* fld_bot,
                         double threshold, int mode, void* stream);
/* Stats::finalize_masks (:1229-1262) in two halves. count: the two cyclic fills (mhh_boundary_cyclic_u32, _2d_u32) and calc_nmask
 * over 0 .. kcells as doubles csums[2][nmasks][kcells] (full, half). finish: nmask int[nmasks][2][kcells] (full, half),
 * nmask_bot int[nmasks] = nmaskh[kstart], area and areah [nmasks][kcells] of the dtype (calc_area, :209-221).                       */
int mhh_stats_mask_count(const mhh_grid* g, void* mfield, void* mfield_bot, int nmasks, void* csums, void* scratch, void* stream);
int mhh_stats_mask_finish(const mhh_grid* g, int nmasks, const void* csums, void* nmask, void* nmask_bot, void* area, void* areah, void* stream);
/* The loops of Stats::calc_stats (:1607-1890), calc_tend (:1893-1919) and calc_stats_2d (:1921-1937): sums[job][mask][kcells]
 * doubles over kstart .. kend INCLUSIVE (zero elsewhere), then out[job][mask][kcells] of the dtype: sum / nmask[k], the offset
 * added to a mean, the fill value (NC_FILL_DOUBLE / NC_FILL_FLOAT) where nmask[k] == 0. The second pass (moments) reads the
 * finished means of the first from device memory. Unknown operations return MHH_EINVAL with a message.                              */
int mhh_stats_sums(const mhh_grid* g, const void* mfield, int nmasks, const mhh_stats_job* jobs, int njobs, void* sums, void* scratch, void* stream);
int mhh_stats_finish(const mhh_grid* g, int nmasks, const mhh_stats_job* jobs, int njobs, const void* sums, const void* nmask, void* out, void* stream);
/* calc_cover (:475-507) and calc_path (:435-473) of one variable, one thread per column: sums[nmasks][3] doubles = cover,
 * nmaskcover, path (a column's path serially in the dtype, as `data*rho*dz`); then out[nmasks][2] of the dtype = cover / nmaskcover
 * (0 without a column) and path / nmask_proj (NaN without a column, as in the reference).                                          */
int mhh_stats_columns(const mhh_grid* g, const void* mfield, int nmasks, const void* fld, int loc, double offset, double threshold,
                      const void* rhoref, void* sums, void* scratch, void* stream);
int mhh_stats_columns_finish(const mhh_grid* g, int nmasks, const void* sums, void* out, void* stream);
/* Grid::interpolate_2nd(wf, w, wloc, sloc) (src/grid.cxx:455-486) for the wplus / wmin masks of Fields::get_mask
 * (src/fields.cxx:631-643): wf [ncells] is zeroed, then written on the levels 0 .. kcells-2 of the interior columns.               */
int mhh_stats_interpolate_w(const mhh_grid* g, const void* w, void* wf, void* stream);

/* ---- Budget_2 (src/budget_2.cxx: Budget_2<TF>::exec_stats for second-order cases) ----------------------------------------------
 * The kinetic energies and the terms of the u2, v2, w2, tke, uw, vw, b2 and bw budgets as masked profiles, evaluated per cell and
 * per mask and reduced in the same launch: no term field reaches memory. EVERY profile, the "zh" ones included, is averaged under
 * the full-level flag and divided by the full-level nmask over kstart .. kend, as calc_mask_stats does with a tmp field of
 * loc {0,0,0} (src/fields.cxx:805); a level the loops of a term do not write counts as zero. Split into sums and finish like Stats;
 * the reductions are deterministic. `scratch`: mhh_budget_2_scratch_elems(g, nmasks) DOUBLES. Needs the cyclic ghost cells of
 * u, v, w, p, evisc, b and one vertical ghost level of each; the LES diffusion group two horizontal ghost cells. */
#define MHH_BUDGET_KE      0x001u  /* calc_kinetic_energy (:51-94): ke, tke                                                        */
#define MHH_BUDGET_SHEAR   0x002u  /* calc_shear_terms (:100-135): u2_shear, v2_shear, tke_shear, uw_shear, vw_shear               */
#define MHH_BUDGET_TURB    0x004u  /* calc_turb_terms (:141-233): u2_turb, v2_turb, w2_turb, tke_turb, uw_turb, vw_turb            */
#define MHH_BUDGET_COR     0x008u  /* calc_coriolis_terms (:239-279): u2_cor, v2_cor, uw_cor, vw_cor (swlspres=geo)                */
#define MHH_BUDGET_PRES    0x010u  /* calc_pressure_transport_terms (:285-352): w2_pres, tke_pres, uw_pres, vw_pres                */
#define MHH_BUDGET_RDSTR   0x020u  /* calc_pressure_redistribution_terms (:358-419): u2_rdstr, v2_rdstr, w2_rdstr, uw_rdstr, vw_rdstr */
#define MHH_BUDGET_DIFF    0x040u  /* calc_diffusion_terms_les (:680-1038), diff_smag2: u2_diff, v2_diff, w2_diff, tke_diff, uw_diff, vw_diff */
#define MHH_BUDGET_BUOY    0x080u  /* calc_buoyancy_terms (:1044-1090): w2_buoy, tke_buoy, uw_buoy, vw_buoy                         */
#define MHH_BUDGET_BW_BUOY 0x100u  /* calc_buoyancy_terms_scalar (:1096-1115) with s = b: bw_buoy                                   */
#define MHH_BUDGET_ADV_S   0x200u  /* calc_advection_terms_scalar (:1121-1156): b2_shear, b2_turb, bw_shear, bw_turb                */
#define MHH_BUDGET_PRES_S  0x400u  /* calc_pressure_terms_scalar (:1257-1279): bw_pres, bw_rdstr                                    */
typedef struct mhh_budget_2_desc
{
    const void *u, *v, *w, *p, *evisc, *b;       /* [ncells]; p, evisc, b may be NULL where no selected group reads them            */
    const void *u_fluxbot, *v_fluxbot;           /* [ijcells]: the LES diffusion group                                               */
    const void *umodel, *vmodel, *wmodel;        /* [nmasks][kcells]: mhh_budget_2_model_finish (Stats::calc_mask_mean_profile)      */
    const void *bmean, *pmean;                   /* [kcells]: field3d_operators.calc_mean_profile of b and p (mhh_field_mean_profile) */
    double utrans, vtrans, fc;                   /* gd.utrans, gd.vtrans, force.get_coriolis_parameter(); narrowed on entry          */
    int order;                                   /* grid.swspatialorder: 2; anything else is refused (Budget_4 is not built)         */
    int diff_scheme;                             /* MHH_DIFF_*: the LES diffusion group is diff_smag2's                              */
    unsigned int groups;                         /* MHH_BUDGET_* bits; profiles come in the order of the bits                         */
} mhh_budget_2_desc;
/* the number of profiles of a group set (-1: unknown bit) and the n-th one's name (Budget_2::create, :1315-1412) with *half = 0 for
 * "z", 1 for "zh"; NULL past the end */
int mhh_budget_2_nprofs(unsigned int groups);
const char* mhh_budget_2_prof_name(unsigned int groups, int n, int* half);
unsigned long long mhh_budget_2_scratch_elems(const mhh_grid* g, int nmasks);
/* Stats::calc_mask_mean_profile (src/stats.cxx:1328-1347) of u, v (full-level flag and nmask) and w (half-level flag and nmaskh):
 * calc_mean over ALL levels 0 .. kcells-1. sums[3][nmasks][kcells] doubles, then out[3][nmasks][kcells] of the dtype = umodel,
 * vmodel, wmodel. A level with nmask[k] == 0 holds 0 (the reference leaves what the vector held: the previous mask's value). */
int mhh_budget_2_model_sums(const mhh_grid* g, const void* mfield, int nmasks, const void* u, const void* v, const void* w, void* sums, void* scratch, void* stream);
int mhh_budget_2_model_finish(const mhh_grid* g, int nmasks, const void* sums, const void* nmask, void* out, void* stream);
/* The calc_* loops of Budget_2::exec_stats (src/budget_2.cxx:1414-1818) with the calc_mean of calc_mask_stats (src/stats.cxx:1350-1390)
 * over each: sums[nprofs][nmasks][kcells] doubles, then out[nprofs][nmasks][kcells] of the dtype with the fill value where
 * nmask[k] == 0. Refused with MHH_EINVAL and a message: order != 2; the LES diffusion group with igc < 2 or jgc < 2, with a scheme
 * other than diff_smag2; a buoyancy, b2 or bw group without b; an unknown group bit. */
int mhh_budget_2_sums(const mhh_grid* g, const void* mfield, int nmasks, const mhh_budget_2_desc* desc, void* sums, void* scratch, void* stream);
int mhh_budget_2_finish(const mhh_grid* g, int nmasks, const mhh_budget_2_desc* desc, const void* sums, const void* nmask, void* out, void* stream);
/* Thermo_dry::get_thermo_field("b") (calc_buoyancy, src/thermo_dry.cxx:51-63): b = grav/thref[k]*(th - thref[k]) on all kcells
 * levels of the interior columns */
int mhh_thermo_dry_buoyancy(const mhh_grid* g, void* b, const void* th, const void* thref, double grav, void* stream);

/* ---- Timeloop RK3/RK4 substep (src/timeloop.cxx:250-334, src/timeloop.cu:35-122) -------- */
int mhh_rk_substep(const mhh_grid* g, int rkorder, int substep, double dt, void* a, void* at, void* stream);
/* pres->exec(sub_dt) followed by timeloop.exec() for u, v, w (src/model.cxx:411,484): the sub-step rides in the pres_2 kernel that
 * stores the corrected tendencies (two array passes per field less than a separate kernel); the bits of mhh_pres_exec followed by
 * mhh_rk_substep(u), (v), (w), which is also what it falls back to (pres_4, the last sub-step of a step). f->u, v, w are WRITTEN. */
int mhh_pres_exec_rk(mhh_pres_plan* plan, const mhh_grid* g, const mhh_fields* f, double sub_dt, int rkorder, int substep, double dt, void* stream);

/* ---- Cross (src/cross.cxx: the cross-section files; src/field3d_io.cxx:754-861 save_xy_slice / save_xz_slice / save_yz_slice) -----
 * The reference runs Cross on the host, also in its GPU build, which copies every prognostic field back first (src/model.cxx:444-451).
 * Here the planes are gathered on the device: a JOB is one plane of one field, written PACKED (interior cells only, the layout the
 * writers put on disk) at its own place of a staging buffer that the caller copies to the host once and writes from there.
 * Indices are ARRAY indices of this rank, ghost cells included (a level k, a row j, a column i): a half-level xz row jend is the
 * north ghost row, as the serial writer reads it. Every entry only enqueues on its stream. */
#define MHH_CROSS_XY    0   /* level `index`:               out [jmax][imax]   (save_xy_slice, :828-861)                               */
#define MHH_CROSS_XZ    1   /* row `index`, levels k0..k1:  out [k1-k0][imax]  (save_xz_slice, :753-788)                               */
#define MHH_CROSS_YZ    2   /* column `index`, k0..k1:      out [k1-k0][jmax]  (save_yz_slice, :790-826): strided by nature            */
#define MHH_CROSS_PLANE 3   /* fld is a 2-D [ijcells] array: out [jmax][imax]  (Cross::cross_plane, src/cross.cxx:638-651)             */
#define MHH_CROSS_MAX_JOBS 32   /* jobs that travel with one launch; a call takes any number and launches per batch                    */
typedef struct mhh_cross_job
{
    const void* fld;             /* [ncells] of the grid's dtype ([ijcells] for PLANE)                                               */
    int kind;                    /* MHH_CROSS_*                                                                                      */
    int index;                   /* XY: k, XZ: j, YZ: i of the array; PLANE: not read                                                */
    int k0, k1;                  /* XZ, YZ: the levels k0 .. k1-1 (gd.kstart, gd.kend of cross_simple)                                */
    double offset;               /* data0: narrowed to the dtype, then added (TF data0)                                              */
    void* out;                   /* where the packed plane goes                                                                      */
} mhh_cross_job;
/* Cross::cross_simple / cross_plane (src/cross.cxx:564-651) without the write: out = data + offset per job. Refused with a reason:
 * an unknown kind, an index outside [0, kcells) / [0, jcells) / [0, icells), k0 / k1 outside [0, kcells].                           */
int mhh_cross_gather(const mhh_grid* g, const mhh_cross_job* jobs, int njobs, void* stream);
/* Cross::cross_lngrad (:653-703): calc_lngrad_2nd (:136-167, order 2) or calc_lngrad_4th (:42-133, order 4) evaluated on the cells
 * of the jobs' planes only (XY | XZ | YZ, inside the interior; the offset is not read), log(dtiny + gx^2 + gy^2 + gz^2) with the sum
 * and the log in double. Needs the filled ghost cells of fld: one in every direction (order 2), three (order 4).                   */
int mhh_cross_lngrad(const mhh_grid* g, int order, const mhh_cross_job* jobs, int njobs, void* stream);
/* Cross::cross_path (:705-725), calc_cross_path (:170-197): out [jmax][imax] = sum over kstart..kend-1 of rhoref[k]*fld*dz[k], serially in
 * the dtype in that operand order                                                                                                 */
int mhh_cross_path(const mhh_grid* g, const void* fld, const void* rhoref, void* out, void* stream);
/* Cross::cross_height_threshold (:738-760), calc_cross_height_threshold (:200-250): out [jmax][imax] = z[k] of the lowest (upward != 0)
 * or highest level with fld > threshold, the fill value TF(-1e-9) (:748) where there is none                                      */
int mhh_cross_height_threshold(const mhh_grid* g, const void* fld, double threshold, int upward, void* out, void* stream);
/* The search of Cross::create (:323-460) for the locations loc[nloc] of one direction (MHH_CROSS_XY: heights, XZ: y, YZ: x), in GLOBAL
 * interior indices: full[*nfull] and half[*nhalf] (room for nloc each), duplicates dropped per list. loc == size decrements the full
 * index (:337, :382); loc == zsize gives kmax-1 and kmax (:425-429); the half offset applies from z[k] on (:437). The metric pointers
 * of g are HOST pointers. A location outside the domain is refused and the message names it.                                      */
int mhh_cross_indices_host(const mhh_grid* g, int kind, const double* loc, int nloc, int* full, int* nfull, int* half, int* nhalf);

/* ---- Immersed_boundary (src/immersed_boundary.cxx, src/immersed_boundary.cu; sw_immersed_boundary=dem) --------------------------------
 * Flow over terrain: the cells just inside the wall (ghost cells) are set from an inverse-distance-weighted interpolation of cells
 * outside it, twice per sub-step (src/model.cxx:380, :407). The set-up (Immersed_boundary::create) runs on the HOST and touches no
 * GPU: every pointer of the three *_host entries is a host pointer. IB_type::User and the fourth order are not built. */
#define MHH_IB_DIRICHLET 0   /* Boundary_type::Dirichlet_type: n_idw-1 points and the boundary value, 2*bv - vI                          */
#define MHH_IB_NEUMANN   1   /* Boundary_type::Neumann_type:   vI - bv*di                                                               */
#define MHH_IB_FLUX      2   /* Boundary_type::Flux_type:      vI - (-bv/visc)*di                                                       */
#define MHH_IB_MAX_JOBS  8   /* jobs that travel with one launch; a call takes any number and launches per batch                         */
/* Ghost_cells<TF> (include/immersed_boundary.h:39-76) as calc_ghost_cells leaves it: nghost entries each, nghost*n_idw for ip_* and
 * c_idw ([n][q], the reference's layout); i, j, k are array indices of this rank; the void* arrays are of the grid's dtype. */
typedef struct mhh_ib_ghost_lists
{
    int* i; int* j; int* k;
    void* xb; void* yb; void* zb;
    void* xi; void* yi; void* zi;
    void* di;
    int* ip_i; int* ip_j; int* ip_k;
    void* ip_d; void* c_idw; void* c_idw_sum;
} mhh_ib_ghost_lists;
/* calc_ghost_cells (src/immersed_boundary.cxx:334-426) for one staggered location: is_ghost_cell (:107-185), find_nearest_location_wall
 * (:188-220) with the image point and di, find_interpolation_points (:223-285), precalculate_idw (:288-331), bit for bit on one host.
 * dem [ijcells] with filled halos; x, y [icells], [jcells] and z, dz [kcells] are the location's own (u: xh, y, z, dz; v: x, yh, z, dz;
 * w: x, y, zh, dzh; s: x, y, z, dz); dx, dy are g's. Two calls: out == NULL stores the count in *nghost; with out, *nghost must hold that
 * count and the lists are filled. The counting call keeps its scan (per thread) for a filling call with the same grid and values. Refused with a reason: "IB dem interpolation out of bounds!"; fewer than n_idw neighbours (naming
 * i, j, k); n_idw < 1; an unknown boundary type; igc < 2 or jgc < 2 (:622); a ghost cell with k+5 >= kcells (the reference reads past its
 * arrays there); a grid of more than 2^31-1 cells. */
int mhh_ib_ghost_cells_host(const mhh_grid* g, const void* dem, const void* x, const void* y, const void* z, const void* dz, int n_idw, int bc,
                            int mpi_offset_x, int mpi_offset_y, int* nghost, mhh_ib_ghost_lists* out);
/* find_k_dem (src/immersed_boundary.cxx:516-537): k_dem[ij] = the first level with z[k] > dem[ij], kend where there is none; interior
 * columns (the halos come from mhh_boundary_cyclic_2d_u32, :916) */
int mhh_ib_k_dem_host(const mhh_grid* g, const void* dem, const void* z, unsigned int* k_dem);
/* interp2_dem (src/immersed_boundary.cxx:65-103) of plane [ijcells] at the points (xp[n], yp[n]): the sbot_spatial boundary values at
 * (xb, yb) (:891-897) */
int mhh_ib_interp_dem_host(const mhh_grid* g, const void* plane, const void* x, const void* y, const void* xp, const void* yp, int n,
                           int mpi_offset_x, int mpi_offset_y, void* out);
/* One field's ghost cells. The DEVICE tables are not the reference's: cell[n] = i + j*icells + k*ijcells of ghost cell n (the list keeps
 * the k-j-i order of calc_ghost_cells), ip[q*nghost + n] the same of its q-th interpolation point, c_idw[q*nghost + n] its weight
 * (TRANSPOSED, [q][n]). Every offset must lie inside the field; interpolation points are never ghost cells of the same list. */
typedef struct mhh_ib_job
{
    void* fld;                      /* [ncells], written at cell[]                                                                 */
    const void* boundary_value;     /* [nghost]: mbot, or sbot of the scalar                                                        */
    int bc;                         /* MHH_IB_*                                                                                      */
    int nghost;                     /* 0: the job is a no-op                                                                         */
    double visc;                    /* Fields::visc or the scalar's; read by MHH_IB_FLUX                                             */
    const int* cell;                /* [nghost]                                                                                      */
    const int* ip;                  /* [n_idw][nghost]; the last row is not read by MHH_IB_DIRICHLET                                 */
    const void* c_idw;              /* [n_idw][nghost]                                                                               */
    const void* c_idw_sum;          /* [nghost]                                                                                      */
    const void* di;                 /* [nghost]                                                                                      */
} mhh_ib_job;
/* set_ghost_cells (src/immersed_boundary.cxx:441-485; set_ghost_cells_g, src/immersed_boundary.cu:33-78) for every job in ONE launch:
 * u, v, w of exec_momentum (:640-669, .cu:108-133), all scalars of exec_scalars (:677-696, .cu:140-168); the reference launches once
 * per field. Same bits: the sum over q in index order from 0, the Dirichlet term last, one division by c_idw_sum. Only enqueues: no
 * allocation, no synchronisation. The cyclic fills that follow (.cu:134-136, :166) are mhh_boundary_cyclic_n, issued by the caller.
 * Refused: a null pointer in a job with nghost > 0, an unknown boundary type, n_idw < 1. */
int mhh_ib_set_ghost_cells(const mhh_grid* g, int n_idw, const mhh_ib_job* jobs, int njobs, void* stream);
/* calc_mask (src/immersed_boundary.cxx:489-512) of get_mask (:930-946): mask = z[k] > dem, maskh = zh[k] > dem as 0 / 1 of the dtype on
 * the interior cells; dem [ijcells] on the device */
int mhh_ib_mask(const mhh_grid* g, const void* dem, void* mask, void* maskh, void* stream);
/* calc_fluxes (src/immersed_boundary.cxx:541-597) of exec_cross (:950-985): flux [ijcells] on the interior columns = the vertical flux
 * at k_dem plus the fluxes through the side faces shared with higher neighbours, / (dx*dy); one thread per column, the reference's
 * operand order. k_dem [ijcells] with filled halos, on the device. */
int mhh_ib_fluxbot(const mhh_grid* g, void* flux, const unsigned int* k_dem, const void* s, double svisc, void* stream);

/* ---- Source and Decay (src/source.cxx, src/decay.cxx; src/model.cxx:398, :401) ---------------------------------------------------
 * Tracer emissions into the tendencies of passive scalars (Gaussian blobs, line segments, blobs with a vertical emission profile)
 * and their exponential decay. The set-up of Source::create runs on the HOST inside the library; the target is the reference's CPU
 * path, which has the moving and time-varying sources its GPU path refuses (src/source.cu:134). */
typedef struct mhh_source_desc
{
    int scalar;                 /* index of the target in mhh_fields.st (sourcelist[n])                                          */
    int swvmr;                  /* != 0: strength in kmol s-1, scaling rhoref[k]/xmair; 0: kg s-1, scaling rhoref[k]              */
    int profile_index;          /* row of the emission profiles, < 0: none (sw_profile)                                          */
    int reserved;
    double x0, y0, z0, sigma_x, sigma_y, sigma_z, line_x, line_y, line_z, strength;    /* narrowed to the grid's dtype first    */
} mhh_source_desc;
typedef struct mhh_source mhh_source;
/* Source::create (src/source.cxx:266-316) for nsrc sources: per source the index ranges of calc_shape (:44-75) or, in z of a profile
 * source, calc_shape_profile (:77-98), and the norm of Source::calc_norm (:435-547), as the reference has them: no periodic wrap, the
 * ranges clipped to the interior; the norm's test INCLUSIVE (i <= range[1]) where the emission loop is exclusive; only the first
 * non-zero of line_x, line_y, line_z gets the three-branch segment. g holds HOST metric pointers (z and dz are read), profiles is host
 * memory [nprofiles][kcells], rhoref host memory [kcells], all of the grid's dtype. The norm is summed over the source's box alone
 * in k, j, i order with the host's exp: the reference adds +0 elsewhere. On a slab (npy > 1) x and y are those of the one-rank grid
 * (src/grid.cxx:252-262 with no offset) and every rank sums the norm of the WHOLE domain, so no exchange is needed and a rank's
 * tendencies are rows of the one-rank result. The device tables are uploaded on the stream, which is synchronised.
 * Refused with a reason: a profile source with a line length != 0 (the reference refuses > 0, :239-244), a scalar or profile index out of range, sigma <= 0. */
int mhh_source_create(const mhh_grid* g, const mhh_source_desc* src, int nsrc, const void* profiles, int nprofiles, const void* rhoref,
                      void* stream, mhh_source** out);
void mhh_source_destroy(mhh_source* h);
/* What Source::exec does under swtimedep_location and swtimedep_strength (src/source.cxx:362-401) once Timedep has interpolated: new
 * x0, y0, z0 and / or strength (NULL: kept) for source n (one value each) or, n < 0, for every source (arrays of the source count).
 * A move redoes the ranges and the norm; the tables are rebuilt and uploaded on the stream, which is synchronised: host work, not
 * part of a captured graph (the launch's size changes with the tables). Refused: a source with a profile ("Emission profiles with
 * time dependent location/strength are not (yet) supported!", :236, :381). */
int mhh_source_update(mhh_source* h, int n, const double* x0, const double* y0, const double* z0, const double* strength, void* stream);
int mhh_source_count(const mhh_source* h);
int mhh_source_tiles(const mhh_source* h);                      /* blocks of the launch                                           */
/* shape[n].range_x, range_y, range_z (array indices of this rank) and norm[n] (src/source.cxx:292-315) */
int mhh_source_ranges(const mhh_source* h, int n, int* range6);
int mhh_source_norm(const mhh_source* h, int n, double* norm);
/* calc_source (src/source.cxx:100-190) of Source::exec (:403-431) for all sources of all scalars in ONE launch; calc_source_g of
 * src/source.cu launches once per source. A cell of f->st[scalar] is read and written once and the sources whose box holds it are
 * added in source order: the bits of the reference's loops where the host's exp is the reference's. Only enqueues: no allocation,
 * no synchronisation, no host round trip. */
int mhh_source_exec(mhh_source* h, const mhh_grid* g, const mhh_fields* f, void* stream);
typedef struct mhh_decay_params
{
    int    exponential[MHH_MAX_SCALARS];   /* swdecay[name] = exponential; all zero: the call does nothing                       */
    double timescale[MHH_MAX_SCALARS];     /* [decay] timescale[name]                                                            */
} mhh_decay_params;
/* enforce_exponential_decay (src/decay.cxx:35-51) of Decay::exec (:97-111) for every decaying scalar in ONE launch over the interior:
 * st -= rate*s with rate = 1./max(timescale, dt_sub), the quotient in double and narrowed (the reference's `1.` is a double literal);
 * dt_sub is timeloop->get_sub_time_step() (src/model.cxx:398). Same bits, fp64 and fp32. stats.calc_tend is not built. */
int mhh_decay_exec(const mhh_grid* g, const mhh_fields* f, const mhh_decay_params* p, double dt_sub, void* stream);
/* Decay::get_mask("couvreux") (src/decay.cxx:123-187) in two halves, so that a slab can sum over its ranks between them as master.sum
 * does. _sums: sums [2][kcells] DOUBLES = the sums of s and of s*s (the square in the grid's dtype) over the rank's interior of each
 * level, through the deterministic two-stage reduction of the horizontal means; scratch holds
 * mhh_decay_couvreux_scratch_elems(g) doubles. _field: mean = sums/(itot*jtot) and var = sumsq/(itot*jtot) - mean*mean narrowed,
 * out = s - mean - nstd*sqrt(var) on the interior and zero elsewhere, outh = grid.interpolate_2nd(out) to the half levels
 * (src/grid.cxx:455-499). The mask is then mhh_stats_mask_thres(out, outh, threshold 0, MHH_STATS_MASK_PLUS). Only enqueue. */
unsigned long long mhh_decay_couvreux_scratch_elems(const mhh_grid* g);
int mhh_decay_couvreux_sums(const mhh_grid* g, const void* s, void* scratch, void* sums, void* stream);
int mhh_decay_couvreux_field(const mhh_grid* g, const void* s, const void* sums, double nstd, void* out, void* outh, void* stream);

/* ---- Boundary_outflow (src/boundary_outflow.cxx; src/model.cxx:347, :383) -------------------------------------------------------------
 * Open lateral boundaries for scalars: Boundary::set_prognostic_outflow_bcs (src/boundary.cxx:464-469) loops over the scalars of
 * scalar_outflow; momentum and the pressure solve stay periodic. */
#define MHH_OUTFLOW_WEST   1   /* Edge_location (include/boundary_outflow.h): the bits of edges_mask; dirs[] is indexed West, East, South, North */
#define MHH_OUTFLOW_EAST   2
#define MHH_OUTFLOW_SOUTH  4
#define MHH_OUTFLOW_NORTH  8
#define MHH_OUTFLOW_OUTFLOW 0  /* Flow_direction::Outflow: a[gc] = a[mirror interior cell]                                           */
#define MHH_OUTFLOW_INFLOW  1  /* Flow_direction::Inflow:  a[gc] = a_d - (n+1)*2*(a_d - inflow_prof[k])                               */
/* The inflow table of Boundary::process_time_dependent_outflow / Boundary::create (src/boundary.cxx:411-426): the ktot values of
 * prof_ktot at kstart .. kend-1 of table_kcells, its ghost levels ZERO (the zero-initialised vector and std::rotate of :421-424).
 * Both are host memory of the grid's dtype; the caller uploads the table. */
int mhh_boundary_outflow_profile_host(const mhh_grid* g, const void* prof_ktot, void* table_kcells);
/* Boundary_outflow<TF>::exec (src/boundary_outflow.cxx:236-343; GPU src/boundary_outflow.cu:147-291) for nfields scalars at once.
 * order 2: compute_inoutflow_2nd (:85-149) on the edges of edges_mask in the order West, East, South, North, West / East over all
 * jcells x kcells and South / North over all icells, so the corner ghost cells are the South / North rule applied to what West / East
 * wrote. South and North set kgc ghost rows, not jgc: the reference passes gd.kgc where the loops expect jgc (:311, :333). dirs[4]:
 * MHH_OUTFLOW_OUTFLOW or _INFLOW per edge; profiles[n]: device table [kcells] of field n, read on inflow edges only (may be NULL
 * without one). order 4: compute_inflow_4th with value 0 at West and compute_outflow_4th at East (:151-193), three ghost columns
 * each; dirs, profiles and the South / North bits are ignored. edges_mask: the edges this rank owns (the reference's mpicoordx == 0,
 * mpicoordy == 0, ... tests); 0 does nothing. At most TWO launches whatever nfields and edges_mask are, where the reference launches
 * once per scalar and edge. Bit for bit the reference's CPU loops. Only enqueues: no allocation, no synchronisation.
 * Refused with a reason, nothing launched: itot < igc, kgc > jgc, jmax < kgc with a South or North edge (the reference's serial loops
 * would read cells they also write, or index outside the field); order 4 with igc < 3 or itot < 3. */
int mhh_boundary_outflow_exec(const mhh_grid* g, int order, void* const* fields, int nfields, const void* const* profiles, const int* dirs,
                              int edges_mask, void* stream);
/* the launches the calling thread's last mhh_boundary_outflow_exec made (the reference: one per scalar and edge, src/boundary_outflow.cu:209-287) */
int mhh_boundary_outflow_last_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* MHH_HIP_H */
