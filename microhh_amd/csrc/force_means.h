// force_means.h -- the tendency terms between diff->exec and pres->exec of the reference's sub-step (src/model.cxx:395,404) and
// the reductions they read (src/model.cxx:351): Field3d_operators' horizontal means, Buffer::exec, Force::exec and the fused
// pass of the two. Kernels and C-ABI entry points; included from k_stencil.hip. The per-cell arithmetic is in cell_ops.h.
#pragma once
#include "level_reduce.h"
#include <gfx950_prims.h>

namespace mhh
{
// =======================================================================================================
// Field3d_operators: calc_mean_profile (src/field3d_operators.cxx:45-66), the sum of calc_mean (:132-155)
// The reduction is that of level_reduce.h, with the tree as the block's order: one double per thread, ONE partial per block.
// =======================================================================================================
constexpr int NMF = MHH_MAX_MEAN_FIELDS;
template<class TF> struct MeanArgs
{
    const TF* f[NMF]; TF* prof[NMF];
    const TF* dz;
    LevelDomain dom; int k0;
};

template<class TF, bool WEIGHTED>
__global__ void __launch_bounds__(LEVEL_THREADS) mean_partial_kernel(const MeanArgs<TF> A, const Tiling t, double* __restrict__ part, int nk, int nchunks)
{
    LevelTile T;
    if (!level_tile(t, blockIdx.x, A.k0, A.dom, T)) return;
    const TF* __restrict__ fld = A.f[blockIdx.y] + (size_t)T.k*A.dom.ijcells;
    const TF dzk = WEIGHTED ? uniform_load(A.dz, T.k) : TF(0);
    double acc = 0.;
    for_chunk_cells<4>(A.dom, T.j0, T.j1, [&](int, int, int ij)
        { acc += WEIGHTED ? double(fld[ij]*dzk) : double(fld[ij]); });         // the product in TF, as `fld[ijk] * gd.dz[k]` is (:148)
    const double sum = block_tree_sum(acc);
    if (threadIdx.x == 0 && threadIdx.y == 0) part[((size_t)blockIdx.y*nk + T.kz)*nchunks + T.by] = sum;
}

// prof[k] = TF(tmp / n), n = double(itot*jtot) (:49,62): one thread per (field, level), the chunks in index order
template<class TF>
__global__ void __launch_bounds__(256) mean_profile_finish_kernel(const MeanArgs<TF> A, const double* __restrict__ part, int nk, int nchunks, double n)
{
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= nk) return;
    const double* __restrict__ q = part + ((size_t)blockIdx.y*nk + k)*nchunks;
    double tmp = 0.;
    for (int c=0; c<nchunks; ++c) tmp += q[c];
    A.prof[blockIdx.y][k] = TF(tmp / n);
}
// one block per field: each level's partials in index order, thread t the levels t, t+256, ... in order, then the tree
__global__ void __launch_bounds__(LEVEL_THREADS) mean_sum_finish_kernel(const double* __restrict__ part, double* __restrict__ sums, int nk, int nchunks)
{
    const int tid = threadIdx.x;
    double acc = 0.;
    for (int k=tid; k<nk; k+=LEVEL_THREADS)
    {
        const double* __restrict__ q = part + ((size_t)blockIdx.x*nk + k)*nchunks;
        double lev = 0.;
        for (int c=0; c<nchunks; ++c) lev += q[c];
        acc += lev;
    }
    const double sum = block_tree_sum(acc);
    if (tid == 0) sums[blockIdx.x] = sum;
}

template<class TF>
static int mean_launch(const mhh_grid* g, const void* const* fields, int nf, void* const* profs, double* sums, double* scratch, hipStream_t st)
{
    MeanArgs<TF> A{};
    for (int n=0; n<NMF; ++n) { A.f[n] = cp<TF>(fields[n < nf ? n : 0]); A.prof[n] = profs ? mp<TF>(profs[n < nf ? n : 0]) : nullptr; }
    A.dz = cp<TF>(g->dz);
    A.dom = level_domain(g);
    const bool weighted = (sums != nullptr);
    A.k0 = weighted ? g->kstart : 0;
    const int nk = weighted ? g->kmax : g->kcells, nchunks = level_chunks(g);
    const Tiling t = level_tiling(g, nk);
    if (weighted) hipLaunchKernelGGL((mean_partial_kernel<TF, true>),  dim3(tiling_blocks(t), nf), dim3(BX, BY, 1), 0, st, A, t, scratch, nk, nchunks);
    else          hipLaunchKernelGGL((mean_partial_kernel<TF, false>), dim3(tiling_blocks(t), nf), dim3(BX, BY, 1), 0, st, A, t, scratch, nk, nchunks);
    MHH_LAUNCH_CHECK();
    if (weighted) hipLaunchKernelGGL(mean_sum_finish_kernel, dim3(nf), dim3(LEVEL_THREADS), 0, st, scratch, sums, nk, nchunks);
    else          hipLaunchKernelGGL(mean_profile_finish_kernel<TF>, dim3((nk + 255)/256, nf), dim3(256), 0, st, A, scratch, nk, nchunks, double(g->itot * g->jtot));
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
static int mean_check(const mhh_grid* g, const void* const* fields, int nf, const void* scratch)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(nf >= 1 && nf <= NMF, "1 .. 3 + MHH_MAX_SCALARS fields per call");
    MHH_REQUIRE(fields && scratch, "null pointer");
    for (int n=0; n<nf; ++n) MHH_REQUIRE(fields[n] != nullptr, "null field");
    return MHH_OK;
}

// =======================================================================================================
// Buffer::exec (src/buffer.cxx:163-206) and Force::exec (src/force.cxx:581-729): ONE kernel, the term groups compiled in by
// BUF and FRC. A 64 x 4 block works one field (blockIdx.y: u, v, w, scalars) on one level; what acts on that field at that level
// is wave-uniform, and a block with nothing to do leaves before its first load. Per-level values come as scalar table loads.
// =======================================================================================================
template<class TF> struct ForceField
{
    TF* t; const TF* a;                        // tendency and field
    const TF* abuf; const TF* sigma; int kbuf; // sponge: profile, table and first level (NULL profile: none)
    int wls;                                   // 0 none, 1 mean profile, 2 local, 3 local, w form
    const TF* ls; const TF* mean; const TF* nref;   // swls profile; mean profile (swwls mean, nudging); nudging reference
};
template<class TF> struct ForceArgs
{
    GridDev<TF> g;
    ForceField<TF> f[NMF];
    int lspres, order;
    TF fbody, uflux, dt, mean_den, fc, utrans, vtrans;
    const double* sums;
    const TF* ug; const TF* vg; const TF* wls; const TF* nfac;
};

template<class TF, bool BUF, bool FRC>
__global__ void __launch_bounds__(BX*BY) buffer_force_kernel(const ForceArgs<TF> A, const Tiling t, int k0)
{
    int bx, by, kz;
    if (!decode_tile(t, blockIdx.x, bx, by, kz)) return;
    const int n = blockIdx.y;                  // 0 u, 1 v, 2 w, 3.. scalars
    const int k = k0 + kz;
    const ForceField<TF>& F = A.f[n];
    const int ks = A.g.kstart;
    const bool buf = BUF && F.abuf != nullptr && k >= F.kbuf;
    const bool frc = FRC && k >= ks;
    const bool pres = frc && ((n == 0 && (A.lspres == MHH_LSPRES_DPDX || A.lspres == MHH_LSPRES_UFLUX)) || (n < 2 && A.lspres == MHH_LSPRES_GEO));
    const bool ls = frc && F.ls != nullptr;
    const bool wl = frc && F.wls != 0 && (F.wls != 3 || k > ks);
    const bool nud = frc && F.nref != nullptr;
    if (!(buf || pres || ls || wl || nud)) return;
    const int i = A.g.istart + bx*BX + threadIdx.x;
    const int j = A.g.jstart + by*BY + threadIdx.y;
    if (i >= A.g.iend || j >= A.g.jend) return;
    const int jj = A.g.icells, kk = A.g.ijcells;
    const int c = i + j*jj + k*kk;
    TF x = F.t[c];
    if (buf) x -= buffer_sub(uniform_load(F.sigma, k), F.a[c], uniform_load(F.abuf, k));
    if (pres)
    {
        if (A.lspres == MHH_LSPRES_DPDX) x += A.fbody;
        else if (A.lspres == MHH_LSPRES_UFLUX)
        {
            const TF u_mean = mean_of_sum(uniform_load(A.sums, 0), A.mean_den), ut_mean = mean_of_sum(uniform_load(A.sums, 1), A.mean_den);
            x += force_fixed_flux_body(A.uflux, u_mean, ut_mean, A.utrans, A.dt);
        }
        else if (n == 0)
        {
            const TF vg = uniform_load(A.vg, k);
            x += (A.order == 4) ? coriolis4_u(A.f[1].a, c, jj, A.fc, A.vtrans, vg) : coriolis2_u(A.f[1].a, c, jj, A.fc, A.vtrans, vg);
        }
        else
        {
            const TF ug = uniform_load(A.ug, k);
            x -= (A.order == 4) ? coriolis4_v(A.f[0].a, c, jj, A.fc, A.utrans, ug) : coriolis2_v(A.f[0].a, c, jj, A.fc, A.utrans, ug);
        }
    }
    if (ls) x += uniform_load(F.ls, k);
    if (wl)
    {
        const TF wk = uniform_load(A.wls, k);
        if (F.wls == 3)      x -= wls_local_w_sub(F.a, c, kk, uniform_load(A.wls, k-1), wk, uniform_load(A.g.dzi, k-1), uniform_load(A.g.dzi, k));
        else if (F.wls == 2) x -= wls_local_sub(F.a, c, kk, wk, uniform_load(A.g.dzhi, k), uniform_load(A.g.dzhi, k+1));
        else                 x -= wls_mean_sub(uniform_load(F.mean, k-1), uniform_load(F.mean, k), uniform_load(F.mean, k+1), wk,
                                               uniform_load(A.g.dzhi, k), uniform_load(A.g.dzhi, k+1));
    }
    if (nud) x += nudge_tend(uniform_load(A.nfac, k), uniform_load(F.mean, k), uniform_load(F.nref, k));
    F.t[c] = x;
}

template<class TF>
static int buffer_force_launch(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, const mhh_force_params* p, hipStream_t st)
{
    const bool buf = b && b->swbuffer, frc = p != nullptr;
    ForceArgs<TF> A{};
    A.g = make_grid<TF>(g);
    const int nf = 3 + f->nscalars;
    void* const tend[3] = {f->ut, f->vt, f->wt}; const void* const fld[3] = {f->u, f->v, f->w};
    bool any = false;
    for (int n=0; n<nf; ++n)
    {
        ForceField<TF>& F = A.f[n];
        const int s = n - 3;
        F.t = mp<TF>(n < 3 ? tend[n] : f->st[s]); F.a = cp<TF>(n < 3 ? fld[n] : f->s[s]);
        if (buf)
        {
            F.abuf = cp<TF>(n == 0 ? b->abuf_u : n == 1 ? b->abuf_v : n == 2 ? b->abuf_w : b->abuf_s[s]);
            F.sigma = cp<TF>(n == 2 ? b->sigmah : b->sigma); F.kbuf = (n == 2) ? b->bufferkstarth : b->bufferkstart;
            any = any || F.abuf;
        }
        if (!frc) continue;
        if (p->swls && n != 2) F.ls = cp<TF>(n == 0 ? p->ls_u : n == 1 ? p->ls_v : p->ls_s[s]);
        if (n != 2) F.mean = cp<TF>(n == 0 ? p->mean_u : n == 1 ? p->mean_v : p->mean_s[s]);
        if (p->swnudge && n != 2) F.nref = cp<TF>(n == 0 ? p->nudge_u : n == 1 ? p->nudge_v : p->nudge_s[s]);
        if (p->swwls && (n >= 3 || p->swwls_mom))
            F.wls = (p->swwls == MHH_WLS_MEAN) ? (n == 2 ? 0 : 1) : (n == 2 ? 3 : 2);
        any = any || F.ls || F.nref || F.wls;
    }
    if (frc)
    {
        A.lspres = p->swlspres; A.order = p->order;
        // the reference's operands are TF: fbody = TF(-1.)*dpdx (:599), uflux, dt passed as const TF (:66-67), fc, utrans, vtrans
        A.fbody = TF(-1.)*TF(p->dpdx); A.uflux = TF(p->uflux); A.dt = TF(p->dt);
        A.mean_den = TF(g->itot * g->jtot) * TF(g->zsize);          // gd.itot * gd.jtot * gd.zsize (src/field3d_operators.cxx:152)
        A.fc = TF(p->fc); A.utrans = TF(p->utrans); A.vtrans = TF(p->vtrans);
        A.sums = static_cast<const double*>(p->uflux_sums);
        A.ug = cp<TF>(p->ug); A.vg = cp<TF>(p->vg); A.wls = cp<TF>(p->wls); A.nfac = cp<TF>(p->nudge_factor);
        any = any || p->swlspres != MHH_LSPRES_NONE;
    }
    if (!any) return MHH_OK;
    // the sponge alone: only the levels inside the buffer are launched
    const int k0 = frc ? g->kstart : (b->bufferkstart < b->bufferkstarth ? b->bufferkstart : b->bufferkstarth);
    if (k0 >= g->kend) return MHH_OK;
    const Tiling t = make_tiling(g->imax, g->jmax, g->kend - k0);
    const dim3 grid(tiling_blocks(t), nf), block(BX, BY, 1);
    if (buf && frc)  hipLaunchKernelGGL((buffer_force_kernel<TF, true, true>),  grid, block, 0, st, A, t, k0);
    else if (buf)    hipLaunchKernelGGL((buffer_force_kernel<TF, true, false>), grid, block, 0, st, A, t, k0);
    else             hipLaunchKernelGGL((buffer_force_kernel<TF, false, true>), grid, block, 0, st, A, t, k0);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

static int buffer_force_check(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, const mhh_force_params* p)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(f != nullptr && f->nscalars >= 0 && f->nscalars <= MHH_MAX_SCALARS, "fields");
    MHH_REQUIRE(f->u && f->v && f->w && f->ut && f->vt && f->wt, "null field");
    for (int n=0; n<f->nscalars; ++n) MHH_REQUIRE(f->s[n] && f->st[n], "null scalar");
    if (b && b->swbuffer)
    {
        MHH_REQUIRE(b->sigma && b->sigmah, "the sponge tables sigma and sigmah (mhh_buffer_sigma_host)");
        MHH_REQUIRE(b->bufferkstart >= g->kstart && b->bufferkstart <= g->kend && b->bufferkstarth >= g->kstart && b->bufferkstarth < g->kend,
                    "bufferkstart / bufferkstarth inside [kstart, kend): Buffer::create (src/buffer.cxx:107-126)");
    }
    if (!p) return MHH_OK;
    MHH_REQUIRE(p->swlspres >= MHH_LSPRES_NONE && p->swlspres <= MHH_LSPRES_GEO, "swlspres: 0 none, 1 dpdx, 2 uflux, 3 geo");
    if (p->swlspres == MHH_LSPRES_UFLUX) MHH_REQUIRE(p->uflux_sums != nullptr && p->dt != 0., "uflux needs the two device sums and dt");
    if (p->swlspres == MHH_LSPRES_GEO)
    {
        MHH_REQUIRE(p->order == 2 || p->order == 4, "order must be 2 or 4 (grid.swspatialorder)");
        MHH_REQUIRE(p->ug && p->vg, "geo needs the ug and vg profiles");
        MHH_REQUIRE(g->igc >= (p->order == 4 ? 2 : 1) && g->jgc >= (p->order == 4 ? 2 : 1), "ghost cells: igc >= 2 and jgc >= 2 for the 4th-order Coriolis stencil");
    }
    MHH_REQUIRE(p->swwls >= MHH_WLS_NONE && p->swwls <= MHH_WLS_LOCAL, "swwls: 0 none, 1 mean, 2 local");
    if (p->swwls)
    {
        MHH_REQUIRE(p->wls != nullptr && g->kgc >= 1, "swwls needs the wls profile and a vertical ghost level");
        if (p->swwls == MHH_WLS_MEAN)
        {
            for (int n=0; n<f->nscalars; ++n) MHH_REQUIRE(p->mean_s[n] != nullptr, "swwls = mean needs the mean profile of every scalar");
            MHH_REQUIRE(!p->swwls_mom || (p->mean_u && p->mean_v), "swwls = mean with swwls_mom needs the mean profiles of u and v");
        }
    }
    if (p->swnudge)
    {
        MHH_REQUIRE(p->nudge_factor != nullptr, "swnudge needs nudge_factor");
        MHH_REQUIRE((!p->nudge_u || p->mean_u) && (!p->nudge_v || p->mean_v), "a nudged field needs its mean profile");
        for (int n=0; n<f->nscalars; ++n) MHH_REQUIRE(!p->nudge_s[n] || p->mean_s[n], "a nudged field needs its mean profile");
    }
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

MHH_API unsigned long long mhh_field_mean_scratch_elems(const mhh_grid* g, int nfields)
{
    if (!g || nfields < 1) return 0;
    return (unsigned long long)nfields * (unsigned long long)g->kcells * (unsigned long long)level_chunks(g);
}
MHH_API int mhh_field_mean_chunk_rows(void) { return LEVEL_ROWS; }
MHH_API int mhh_field_mean_profile(const mhh_grid* g, const void* const* fields, int nfields, void* const* profs, void* scratch, void* stream)
{
    if (int e = mean_check(g, fields, nfields, scratch)) return e;
    MHH_REQUIRE(profs != nullptr, "null pointer");
    for (int n=0; n<nfields; ++n) MHH_REQUIRE(profs[n] != nullptr, "null profile");
#define CALL(TF) mean_launch<TF>(g, fields, nfields, profs, nullptr, static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_field_mean_sum(const mhh_grid* g, const void* const* fields, int nfields, void* sums, void* scratch, void* stream)
{
    if (int e = mean_check(g, fields, nfields, scratch)) return e;
    MHH_REQUIRE(sums != nullptr && g->dz != nullptr, "null pointer");
#define CALL(TF) mean_launch<TF>(g, fields, nfields, nullptr, static_cast<double*>(sums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// host helper: the sponge table, with the C library's pow of a TF like the reference (src/buffer.cxx:44,48) -- `g` carries HOST
// metric pointers here, as in mhh_smag2_mlen0_host
template<class TF>
static void buffer_sigma(const mhh_grid* g, TF zstart, TF sigma, TF beta, int half, TF* o)
{
    const TF* z = cp<TF>(half ? g->zh : g->z);
    const TF zsizebuf = TF(g->zsize) - zstart;
    for (int k=0; k<g->kcells; ++k)
        o[k] = (k >= g->kstart && k < g->kend && !(z[k] < zstart)) ? sigma*std::pow((z[k]-zstart)/zsizebuf, beta) : TF(0);
}
MHH_API int mhh_buffer_sigma_host(const mhh_grid* g, double zstart, double sigma, double beta, int half_level, void* out)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE((half_level ? g->zh : g->z) && out, "null pointer");
    if (g->dtype == MHH_F64) buffer_sigma<double>(g, zstart, sigma, beta, half_level, mp<double>(out));
    else                     buffer_sigma<float>(g, (float)zstart, (float)sigma, (float)beta, half_level, mp<float>(out));
    return MHH_OK;
}

MHH_API int mhh_buffer_exec(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, void* stream)
{
    MHH_REQUIRE(b != nullptr, "params");
    if (int e = buffer_force_check(g, f, b, nullptr)) return e;
    if (!b->swbuffer) return MHH_OK;
#define CALL(TF) buffer_force_launch<TF>(g, f, b, nullptr, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_force_exec(const mhh_grid* g, const mhh_fields* f, const mhh_force_params* p, void* stream)
{
    MHH_REQUIRE(p != nullptr, "params");
    if (int e = buffer_force_check(g, f, nullptr, p)) return e;
#define CALL(TF) buffer_force_launch<TF>(g, f, nullptr, p, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_buffer_force_exec(const mhh_grid* g, const mhh_fields* f, const mhh_buffer_params* b, const mhh_force_params* p, void* stream)
{
    MHH_REQUIRE(b != nullptr && p != nullptr, "params");
    if (int e = buffer_force_check(g, f, b, p)) return e;
#define CALL(TF) buffer_force_launch<TF>(g, f, b, p, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
