// surface_layer.h -- Boundary_surface<TF>::exec on the device (src/boundary_surface.cxx:830-983): the Monin-Obukhov surface
// layer with the lookup solver (swconstantz0 = true). Kernels and C-ABI entry points; included from k_stencil.hip. The per-cell
// arithmetic is in cell_ops.h. Everything here works on 2-D arrays [ijcells] and the level kstart of the 3-D fields: one thread
// per column, launched through the generic cell kernel with one "level".
//
// Launch structure of mhh_boundary_surface_exec:
//   K1  dutot on the interior                                     (calc_dutot)
//       2-D cyclic fill of dutot
//   K2  all cells: stability (table walk from nobuk, ustar), surfs of every scalar, ugradbot / vgradbot, and on the interior
//       dudz / dvdz / dbdz -- everything that reads ustar / obuk of the OWN column only
//   K3  interior: ufluxbot, vfluxbot, which read ustar / obuk of the west / south neighbour: K2 must have finished grid-wide
//       2-D cyclic fills of ufluxbot, vfluxbot
#pragma once
#include <vector>
#include "k_common.h"

namespace mhh
{
template<class TF> struct SurfArgs
{
    GridDev<TF> g;
    int mbcbot, thermobc, kind, tidx, ns;
    TF thref, threfh, grav, n2;
    const float* zL; const float* f;
    const TF* z0m; const TF* z0h;
    TF* ustar; TF* obuk; int* nobuk;
    const TF* u; const TF* v; const TF* ubot; const TF* vbot;
    TF* ugradbot; TF* vgradbot; TF* ufluxbot; TF* vfluxbot;
    TF* dudz; TF* dvdz; TF* dbdz;
    const TF* s[MHH_MAX_SCALARS]; TF* sbot[MHH_MAX_SCALARS]; TF* sgradbot[MHH_MAX_SCALARS]; TF* sfluxbot[MHH_MAX_SCALARS];
    int sbc[MHH_MAX_SCALARS];
    const TF* th; const TF* thbot; const TF* thflux;     // the thermo scalar's field, bottom value and bottom flux: s[tidx] etc., named
                                                         // so that no kernel indexes the argument block with a value it loads
    TF* dutot;
    // Thermo_moist (kind 3): qt's field, bottom value and bottom flux, named like th's, and the base-state tables read at kstart
    int qidx;
    const TF* qt; const TF* qtbot; const TF* qtflux; const TF* thvref; const TF* thvrefh;
};

// ---- the stages as functions of one column, shared by the stage kernels and the fused ones ------------------------------
template<class TF> __device__ __forceinline__ bool surf_interior(const GridDev<TF>& g, int i, int j)
{ return i >= g.istart && i < g.iend && j >= g.jstart && j < g.jend; }

// buoyancy flux at the surface from the thermo scalar's flux (Thermo_dry calc_buoyancy_fluxbot / Thermo_buoy's copy); Thermo_moist
// (calc_buoyancy_fluxbot, src/thermo_moist.cxx:675-693): from the first level's thl and qt (cell c) and the two bottom fluxes
template<class TF> __device__ __forceinline__ TF surf_bfluxbot(const SurfArgs<TF>& A, int c, TF sflux, TF qflux)
{
    if (A.kind == 3) return moist_buoyancy_flux_no_ql(A.th[c], sflux, A.qt[c], qflux, uniform_load(A.thvrefh, A.g.kstart));
    return (A.kind == 1) ? dry_bfluxbot(A.grav, A.threfh, sflux) : sflux;
}
// qt's bottom flux of column ij as it stands in memory (0 unless Thermo_moist)
template<class TF> __device__ __forceinline__ TF surf_qflux(const SurfArgs<TF>& A, int ij) { return (A.kind == 3) ? A.qtflux[ij] : TF(0); }
// Thermo_moist's db of the Dirichlet case: calc_buoyancy_bot (:637-655) and get_db_ref (:1713-1717)
template<class TF> __device__ __forceinline__ TF surf_moist_db(const SurfArgs<TF>& A, int c, int ij)
{
    const TF thv = uniform_load(A.thvref, A.g.kstart), thvh = uniform_load(A.thvrefh, A.g.kstart);
    const TF bbot = moist_buoyancy_no_ql(A.thbot[ij], A.qtbot[ij], thvh);
    const TF b    = moist_buoyancy_no_ql(A.th[c], A.qt[c], thv);
    const TF db_ref = MoistC<TF>::grav/thv*(thv - thvh);
    return b - bbot + db_ref;
}

// stage c: stability / stability_neutral (src/boundary_surface.cxx:54-177) for column ij
template<class TF> __device__ __forceinline__ void surf_stability_cell(const SurfArgs<TF>& A, int i, int j, int ij)
{
    const int ks = A.g.kstart;
    const TF zsl = uniform_load(A.g.z, ks);
    if (A.kind == 0)
    {
        if (A.mbcbot == MHH_BC_USTAR) { if (surf_interior(A.g, i, j)) A.obuk[ij] = TF(-1.e9); }     // -Constants::dbig, interior only (:157-163)
        else
        {
            const TF L = TF(-1.e9);
            A.obuk[ij] = L;
            A.ustar[ij] = A.dutot[ij] * most_fm(zsl, A.z0m[ij], L);
        }
        return;
    }
    const int c = ij + ks*A.g.ijcells;
    if (A.mbcbot == MHH_BC_USTAR)
    {
        A.obuk[ij] = surf_obuk_ustar_flux(A.ustar[ij], surf_bfluxbot(A, c, A.thflux[ij], surf_qflux(A, ij)));
        return;
    }
    int n = A.nobuk[ij];
    const TF du = A.dutot[ij];
    TF L;
    if (A.thermobc == MHH_BC_FLUX)
        L = surf_obuk_flux(A.zL, A.f, n, du, surf_bfluxbot(A, c, A.thflux[ij], surf_qflux(A, ij)), zsl);
    else
    {
        const TF th = A.th[c], thbot = A.thbot[ij];
        const TF db = (A.kind == 3) ? surf_moist_db(A, c, ij) : (A.kind == 1) ? dry_db(A.grav, A.thref, A.threfh, th, thbot) : th - thbot + A.n2;
        L = surf_obuk_dirichlet(A.zL, A.f, n, du, db, zsl);
    }
    A.nobuk[ij] = n;
    A.obuk[ij] = L;
    A.ustar[ij] = du * most_fm(zsl, A.z0m[ij], L);
}

// entry n of a per-scalar member of the argument block, through constant indices and selects: an index that is a loop variable
// would make the compiler keep a copy of the whole block in scratch
template<class T> __device__ __forceinline__ T surf_pick(T const (&a)[MHH_MAX_SCALARS], int n)
{
    T r = a[0];
#pragma unroll
    for (int m=1; m<MHH_MAX_SCALARS; ++m) r = (n == m) ? a[m] : r;
    return r;
}
// stage e: surfs for scalar n (:291-339); returns the scalar's bottom flux as it stands afterwards
template<class TF> __device__ __forceinline__ TF surf_scalar_cell(const SurfArgs<TF>& A, int n, int ij)
{
    const int c = ij + A.g.kstart*A.g.ijcells;
    const TF zsl = uniform_load(A.g.z, A.g.kstart);
    const TF* __restrict__ s = surf_pick(A.s, n);
    TF* __restrict__ sbot = surf_pick(A.sbot, n); TF* __restrict__ sgradbot = surf_pick(A.sgradbot, n); TF* __restrict__ sfluxbot = surf_pick(A.sfluxbot, n);
    const int bc = surf_pick(A.sbc, n);
    const TF var = s[c];
    if (bc == MHH_BC_DIRICHLET)
    {
        const TF bot = sbot[ij];
        const TF flux = surf_scalar_flux(var, bot, A.ustar[ij], A.obuk[ij], A.z0h[ij], zsl);
        sfluxbot[ij] = flux;
        sgradbot[ij] = surf_lin_grad(var, bot, zsl);
        return flux;
    }
    const TF flux = sfluxbot[ij];
    if (bc == MHH_BC_FLUX)
    {
        const TF bot = surf_scalar_bot(var, flux, A.ustar[ij], A.obuk[ij], A.z0h[ij], zsl);
        sbot[ij] = bot;
        sgradbot[ij] = surf_lin_grad(var, bot, zsl);
    }
    return flux;                                                   // any other type: surfs leaves the scalar alone
}

// stage d, gradient part (:276-287), all cells
template<class TF> __device__ __forceinline__ void surf_momgrad_cell(const SurfArgs<TF>& A, int ij)
{
    const int c = ij + A.g.kstart*A.g.ijcells;
    const TF zsl = uniform_load(A.g.z, A.g.kstart);
    A.ugradbot[ij] = surf_lin_grad(A.u[c], A.ubot[ij], zsl);
    A.vgradbot[ij] = surf_lin_grad(A.v[c], A.vbot[ij], zsl);
}
// stage d, flux part (:200-252), interior
template<class TF> __device__ __forceinline__ void surf_momflux_cell(const SurfArgs<TF>& A, int ij)
{
    const int jj = A.g.icells, c = ij + A.g.kstart*A.g.ijcells;
    const TF zsl = uniform_load(A.g.z, A.g.kstart);
    if (A.mbcbot == MHH_BC_DIRICHLET)
    {
        A.ufluxbot[ij] = surf_mom_flux(A.u[c], A.ubot[ij], A.ustar, A.obuk, A.z0m, ij, ij-1,  zsl);
        A.vfluxbot[ij] = surf_mom_flux(A.v[c], A.vbot[ij], A.ustar, A.obuk, A.z0m, ij, ij-jj, zsl);
    }
    else
    {
        TF uf, vf;
        surf_mom_flux_ustar(uf, vf, A.u, A.v, A.ubot, A.vbot, A.ustar, c, ij, jj);
        A.ufluxbot[ij] = uf; A.vfluxbot[ij] = vf;
    }
}
// stage f: calc_duvdz_mo, calc_dbdz_mo (boundary_surface_kernels.h:186-243), interior; sflux = the thermo scalar's bottom flux,
// qflux = qt's (Thermo_moist)
template<class TF> __device__ __forceinline__ void surf_mograd_cell(const SurfArgs<TF>& A, int ij, TF sflux, TF qflux)
{
    const int jj = A.g.icells, c = ij + A.g.kstart*A.g.ijcells;
    const TF zsl = uniform_load(A.g.z, A.g.kstart);
    const TF us = A.ustar[ij], L = A.obuk[ij], z0 = A.z0m[ij];
    const TF du_c = TF(0.5)*((A.u[c] - A.ubot[ij]) + (A.u[c+1 ] - A.ubot[ij+1 ]));
    const TF dv_c = TF(0.5)*((A.v[c] - A.vbot[ij]) + (A.v[c+jj] - A.vbot[ij+jj]));
    A.dudz[ij] = surf_duvdz_mo(du_c, us, L, z0, zsl);
    A.dvdz[ij] = surf_duvdz_mo(dv_c, us, L, z0, zsl);
    if (A.kind != 0) A.dbdz[ij] = surf_dbdz_mo(surf_bfluxbot(A, c, sflux, qflux), us, L, zsl);
}

// ---- the operators the generic cell kernel runs (k is the single pseudo-level 0) ------------------------------------------
template<class TF> struct SurfDutotOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const
    {
        const int ij = i + j*A.g.icells;
        A.dutot[ij] = surf_dutot(A.u, A.v, A.ubot, A.vbot, ij + A.g.kstart*A.g.ijcells, ij, A.g.icells);
    }
};
template<class TF> struct SurfStabilityOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const { surf_stability_cell(A, i, j, i + j*A.g.icells); }
};
template<class TF> struct SurfMomGradOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const { surf_momgrad_cell(A, i + j*A.g.icells); }
};
template<class TF> struct SurfMomFluxOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const { surf_momflux_cell(A, i + j*A.g.icells); }
};
template<class TF> struct SurfScalarOp
{
    SurfArgs<TF> A; int n;
    __device__ void operator()(int i, int j, int, int) const { surf_scalar_cell(A, n, i + j*A.g.icells); }
};
template<class TF> struct SurfMoGradOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const
    {
        const int ij = i + j*A.g.icells;
        surf_mograd_cell(A, ij, A.kind != 0 ? A.thflux[ij] : TF(0), surf_qflux(A, ij));
    }
};
// K2 of the fused entry point: c, e, the gradients of d, f for one column
template<class TF> struct SurfColumnOp
{
    SurfArgs<TF> A;
    __device__ void operator()(int i, int j, int, int) const
    {
        const int ij = i + j*A.g.icells;
        surf_stability_cell(A, i, j, ij);
        surf_momgrad_cell(A, ij);
        TF sflux = TF(0), qflux = TF(0);
#pragma unroll
        for (int n=0; n<MHH_MAX_SCALARS; ++n)            // constant indices into the argument block (see surf_pick)
            if (n < A.ns)
            {
                const TF fl = surf_scalar_cell(A, n, ij);
                if (n == A.tidx) sflux = fl;
                if (n == A.qidx) qflux = fl;
            }
        if (surf_interior(A.g, i, j)) surf_mograd_cell(A, ij, sflux, qflux);
    }
};

inline const char* surf_refusal(const mhh_grid* g, const mhh_surface_params* p)
{
    if (!p->swconstantz0) return "swconstantz0 = false: the iterative Obukhov-length solvers (include/boundary_surface_kernels.h:287-470) are not built, only the lookup solver";
    if (p->swcharnock) return "swcharnock: the Charnock roughness update (calc_z0_charnock) is not built";
    if (g->igc < 2 || g->jgc < 2) return "igc >= 2 and jgc >= 2: calc_dutot reads u[i+2] and v[j+2] (include/boundary_surface_kernels.h:164-172)";
    return nullptr;
}

// which pointers a stage needs: bit set of what is checked
enum { SURF_NEED_DUTOT_IN = 1, SURF_NEED_STAB = 2, SURF_NEED_MOM = 4, SURF_NEED_SCAL = 8, SURF_NEED_MO = 16, SURF_NEED_VEL = 32 };

static int surf_check(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, const void* dutot, int need)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(f != nullptr && p != nullptr, "null pointer");
    if (const char* why = surf_refusal(g, p)) { set_error("Boundary_surface refused: %s", why); return MHH_EINVAL; }
    MHH_REQUIRE(g->z != nullptr, "grid.z (zsl = z[kstart])");
    MHH_REQUIRE(p->mbcbot == MHH_BC_DIRICHLET || p->mbcbot == MHH_BC_USTAR, "mbcbot: Dirichlet (noslip) or Ustar");
    MHH_REQUIRE(p->thermo_kind >= MHH_THERMO_NONE && p->thermo_kind <= MHH_THERMO_MOIST, "thermo_kind: 0 none, 1 dry, 2 buoy, 3 moist");
    MHH_REQUIRE(f->nscalars >= 0 && f->nscalars <= MHH_MAX_SCALARS, "nscalars");
    if (p->thermo_kind != MHH_THERMO_NONE)
    {
        MHH_REQUIRE(p->thermo_index >= 0 && p->thermo_index < f->nscalars, "thermo_index names a scalar");
        MHH_REQUIRE(p->thermobc == p->sbcbot[p->thermo_index], "thermobc is the boundary type of the thermo scalar");
        MHH_REQUIRE(p->thermobc == MHH_BC_FLUX || (p->thermobc == MHH_BC_DIRICHLET && p->mbcbot == MHH_BC_DIRICHLET),
                    "thermo bc: Flux, or Dirichlet with mbcbot = Dirichlet (the cases of stability, src/boundary_surface.cxx:83-133)");
        if (p->thermo_kind == MHH_THERMO_DRY) MHH_REQUIRE(p->thref_kstart > 0. && p->threfh_kstart > 0., "thref[kstart], threfh[kstart]");
        if (p->thermo_kind == MHH_THERMO_MOIST)
        {
            const int q = p->qt_index;
            MHH_REQUIRE(q >= 0 && q < f->nscalars && q != p->thermo_index, "qt_index names a scalar other than thl");
            MHH_REQUIRE(p->sbcbot[q] == p->thermobc, "Thermo_moist: qt must have the same kind of bottom bc as thl (thermobc is thl's; the buoyancy flux and the surface buoyancy need both scalars' fluxes or both surface values)");
            MHH_REQUIRE(p->thvref && p->thvrefh, "Thermo_moist: the device tables thvref, thvrefh");
            MHH_REQUIRE(f->s[q] && f->s_fluxbot[q] && p->sbot[q], "qt, its bottom flux and bottom value");
        }
    }
    MHH_REQUIRE(p->ustar && p->obuk && p->z0m && p->z0h, "ustar, obuk, z0m, z0h");
    if (need & (SURF_NEED_DUTOT_IN | SURF_NEED_VEL)) MHH_REQUIRE(dutot != nullptr, "dutot");
    if (need & (SURF_NEED_VEL | SURF_NEED_MOM | SURF_NEED_MO)) MHH_REQUIRE(f->u && f->v && p->ubot && p->vbot, "u, v, ubot, vbot");
    if (need & SURF_NEED_STAB)
    {
        const bool lookup = p->thermo_kind != MHH_THERMO_NONE && p->mbcbot == MHH_BC_DIRICHLET;
        if (lookup) MHH_REQUIRE(p->zL && p->f && p->nobuk, "the lookup table zL, f (mhh_surface_lut_host) and nobuk");
        if (p->thermo_kind != MHH_THERMO_NONE)
        {
            const int t = p->thermo_index;
            MHH_REQUIRE(f->s[t] && f->s_fluxbot[t] && p->sbot[t], "the thermo scalar, its bottom flux and bottom value");
        }
    }
    if (need & SURF_NEED_MOM) MHH_REQUIRE(p->ugradbot && p->vgradbot && f->u_fluxbot && f->v_fluxbot, "ugradbot, vgradbot, u_fluxbot, v_fluxbot");
    if (need & SURF_NEED_SCAL)
        for (int n=0; n<f->nscalars; ++n)
        {
            MHH_REQUIRE(p->sbcbot[n] >= MHH_BC_DIRICHLET && p->sbcbot[n] <= MHH_BC_FLUX, "sbcbot: Dirichlet, Neumann or Flux");
            if (p->sbcbot[n] != MHH_BC_NEUMANN) MHH_REQUIRE(f->s[n] && f->s_fluxbot[n] && p->sbot[n] && p->sgradbot[n], "scalar, s_fluxbot, sbot, sgradbot");
        }
    if (need & SURF_NEED_MO)
    {
        MHH_REQUIRE(f->dudz && f->dvdz, "dudz, dvdz");
        if (p->thermo_kind != MHH_THERMO_NONE) MHH_REQUIRE(f->dbdz && f->s_fluxbot[p->thermo_index], "dbdz and the thermo scalar's bottom flux");
    }
    return MHH_OK;
}

// The flux and gradient arrays of mhh_fields are const for the OPERATORS, which read them; the surface layer is what writes them.
template<class TF> static SurfArgs<TF> surf_args(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* dutot)
{
    SurfArgs<TF> A{};
    A.g = make_grid<TF>(g);
    A.mbcbot = p->mbcbot; A.thermobc = p->thermobc; A.kind = p->thermo_kind; A.tidx = p->thermo_kind ? p->thermo_index : -1; A.ns = f->nscalars;
    A.thref = TF(p->thref_kstart); A.threfh = TF(p->threfh_kstart); A.grav = TF(p->grav); A.n2 = TF(p->bg_n2);
    A.zL = static_cast<const float*>(p->zL); A.f = static_cast<const float*>(p->f);
    A.z0m = cp<TF>(p->z0m); A.z0h = cp<TF>(p->z0h);
    A.ustar = mp<TF>(p->ustar); A.obuk = mp<TF>(p->obuk); A.nobuk = static_cast<int*>(p->nobuk);
    A.u = cp<TF>(f->u); A.v = cp<TF>(f->v); A.ubot = cp<TF>(p->ubot); A.vbot = cp<TF>(p->vbot);
    A.ugradbot = mp<TF>(p->ugradbot); A.vgradbot = mp<TF>(p->vgradbot);
    A.ufluxbot = const_cast<TF*>(cp<TF>(f->u_fluxbot)); A.vfluxbot = const_cast<TF*>(cp<TF>(f->v_fluxbot));
    A.dudz = const_cast<TF*>(cp<TF>(f->dudz)); A.dvdz = const_cast<TF*>(cp<TF>(f->dvdz)); A.dbdz = const_cast<TF*>(cp<TF>(f->dbdz));
    for (int n=0; n<MHH_MAX_SCALARS; ++n)
    {
        const bool on = n < f->nscalars;
        A.s[n] = on ? cp<TF>(f->s[n]) : nullptr; A.sbot[n] = on ? mp<TF>(p->sbot[n]) : nullptr; A.sgradbot[n] = on ? mp<TF>(p->sgradbot[n]) : nullptr;
        A.sfluxbot[n] = on ? const_cast<TF*>(cp<TF>(f->s_fluxbot[n])) : nullptr; A.sbc[n] = on ? p->sbcbot[n] : MHH_BC_NEUMANN;
    }
    if (A.tidx >= 0) { A.th = A.s[A.tidx]; A.thbot = A.sbot[A.tidx]; A.thflux = A.sfluxbot[A.tidx]; }
    A.qidx = -1;
    if (A.kind == MHH_THERMO_MOIST)
    {
        A.qidx = p->qt_index;
        A.qt = A.s[A.qidx]; A.qtbot = A.sbot[A.qidx]; A.qtflux = A.sfluxbot[A.qidx];
        A.thvref = cp<TF>(p->thvref); A.thvrefh = cp<TF>(p->thvrefh);
    }
    A.dutot = mp<TF>(dutot);
    return A;
}

template<class TF, class Op> static int surf_launch(const mhh_grid* g, const Op& op, bool all_cells, hipStream_t st)
{
    if (all_cells) return launch_cells(st, op, 0, g->icells, 0, g->jcells, 0, 1, g->icells, g->ijcells);
    return launch_cells(st, op, g->istart, g->iend, g->jstart, g->jend, 0, 1, g->icells, g->ijcells);
}
// Boundary_cyclic::exec_2d of one array: what mhh_boundary_cyclic_2d launches
template<class TF> static int surf_fill(const mhh_grid* g, void* a, hipStream_t st)
{
    void* d[1] = {a};
    return cyclic_launch<TF>(g, d, 1, MHH_EDGE_BOTH, 1, 0, 1, st);
}

template<class TF> static int surf_exec(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* dutot, hipStream_t st)
{
    const SurfArgs<TF> A = surf_args<TF>(g, f, p, dutot);
    if (int e = surf_launch<TF>(g, SurfDutotOp<TF>{A}, false, st)) return e;
    if (int e = surf_fill<TF>(g, dutot, st)) return e;
    if (int e = surf_launch<TF>(g, SurfColumnOp<TF>{A}, true, st)) return e;
    if (int e = surf_launch<TF>(g, SurfMomFluxOp<TF>{A}, false, st)) return e;
    if (int e = surf_fill<TF>(g, A.ufluxbot, st)) return e;
    return surf_fill<TF>(g, A.vfluxbot, st);
}

// prepare_lut (include/boundary_surface_kernels.h:78-133) on the host: the temporaries in TF, the tables float. The integer
// exponents reach the C library's pow as the reference's std::pow(TF, int) does, through double; they are read from volatile
// objects so that no compiler turns the call into products.
template<class TF> static void surf_lut(TF zsl, TF z0m, TF z0h, int mbcbot, int thermobc, float* zL_sl, float* f_sl)
{
    const int nzL = SURF_NZL;
    std::vector<TF> zL_tmp(nzL);
    const TF zL_max = 10., zL_min = -1.e4;                         // Constants::zL_max / zL_min
    const TF zLrange_min = -5.;
    TF dzL = (zL_max - zLrange_min) / (9.*nzL/10.-1.);
    zL_tmp[0] = -zL_max;
    for (int n=1; n<9*nzL/10; ++n)
        zL_tmp[n] = zL_tmp[n-1] + dzL;
    const TF zLend = -(zL_min - zLrange_min);
    TF r  = 1.01;
    TF r0 = 1.e30;                                                 // Constants::dhuge
    while (std::abs( (r-r0)/r0 ) > 1.e-10)
    {
        r0 = r;
        r  = std::pow( 1. - (zLend/dzL)*(1.-r), (1./ (nzL/10.) ) );
    }
    for (int n=9*nzL/10; n<nzL; ++n)
    {
        zL_tmp[n] = zL_tmp[n-1] + dzL;
        dzL *= r;
    }
    for (int n=0; n<nzL; ++n)
        zL_sl[n] = -zL_tmp[nzL-n-1];
    const volatile int two = 2, three = 3;
    if (mbcbot == MHH_BC_DIRICHLET && thermobc == MHH_BC_FLUX)
    {
        for (int n=0; n<nzL; ++n)
            f_sl[n] = zL_sl[n] * std::pow(most_fm(zsl, z0m, zsl/zL_sl[n]), (int)three);
    }
    else if (mbcbot == MHH_BC_DIRICHLET && thermobc == MHH_BC_DIRICHLET)
    {
        for (int n=0; n<nzL; ++n)
            f_sl[n] = zL_sl[n] * std::pow(most_fm(zsl, z0m, zsl/zL_sl[n]), (int)two) / most_fh(zsl, z0h, zsl/zL_sl[n]);
    }
}
} // namespace mhh
using namespace mhh;

MHH_API int mhh_surface_lut_host(double zsl, double z0m, double z0h, int mbcbot, int thermobc, int dtype, float* zL_out, float* f_out)
{
    MHH_REQUIRE(dtype == MHH_F64 || dtype == MHH_F32, "dtype");
    MHH_REQUIRE(zL_out && f_out, "null pointer");
    MHH_REQUIRE(zsl > 0. && z0m > 0. && z0h > 0., "zsl, z0m, z0h must be positive");
    for (int n=0; n<SURF_NZL; ++n) f_out[n] = 0.f;                 // a pair without a table (Ustar): defined contents
    if (dtype == MHH_F64) surf_lut<double>(zsl, z0m, z0h, mbcbot, thermobc, zL_out, f_out);
    else                  surf_lut<float>((float)zsl, (float)z0m, (float)z0h, mbcbot, thermobc, zL_out, f_out);
    return MHH_OK;
}

MHH_API int mhh_surface_dutot(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* dutot, void* stream)
{
    if (int e = surf_check(g, f, p, dutot, SURF_NEED_VEL)) return e;
#define CALL(TF) surf_launch<TF>(g, SurfDutotOp<TF>{surf_args<TF>(g, f, p, dutot)}, false, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_surface_stability(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, const void* dutot, void* stream)
{
    if (int e = surf_check(g, f, p, dutot, SURF_NEED_DUTOT_IN | SURF_NEED_STAB)) return e;
#define CALL(TF) surf_launch<TF>(g, SurfStabilityOp<TF>{surf_args<TF>(g, f, p, const_cast<void*>(dutot))}, true, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_surface_momentum(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* stream)
{
    if (int e = surf_check(g, f, p, nullptr, SURF_NEED_MOM)) return e;
#define CALL(TF) [&]{ const SurfArgs<TF> A = surf_args<TF>(g, f, p, nullptr); hipStream_t st = as_stream(stream); \
                      if (int e = surf_launch<TF>(g, SurfMomFluxOp<TF>{A}, false, st)) return e; \
                      return surf_launch<TF>(g, SurfMomGradOp<TF>{A}, true, st); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_surface_scalar(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, int n, void* stream)
{
    if (int e = surf_check(g, f, p, nullptr, SURF_NEED_SCAL)) return e;
    MHH_REQUIRE(n >= 0 && n < f->nscalars, "scalar index");
    if (p->sbcbot[n] == MHH_BC_NEUMANN) return MHH_OK;             // surfs has no Neumann branch: nothing to do
#define CALL(TF) surf_launch<TF>(g, SurfScalarOp<TF>{surf_args<TF>(g, f, p, nullptr), n}, true, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_surface_mo_gradients(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* stream)
{
    if (int e = surf_check(g, f, p, nullptr, SURF_NEED_MO)) return e;
#define CALL(TF) surf_launch<TF>(g, SurfMoGradOp<TF>{surf_args<TF>(g, f, p, nullptr)}, false, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_boundary_surface_exec(const mhh_grid* g, const mhh_fields* f, const mhh_surface_params* p, void* scratch, void* stream)
{
    if (int e = surf_check(g, f, p, scratch, SURF_NEED_VEL | SURF_NEED_STAB | SURF_NEED_MOM | SURF_NEED_SCAL | SURF_NEED_MO)) return e;
    MHH_REQUIRE(g->npy == 1, "slab-decomposed grid: the north-south rows of dutot, u_fluxbot, v_fluxbot travel between the stages (mhh_surface_*), which the driver calls one by one");
#define CALL(TF) surf_exec<TF>(g, f, p, scratch, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
