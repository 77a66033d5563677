// microphys_2mom_warm.h -- Microphys_2mom_warm (src/microphys_2mom_warm.cxx: Seifert & Beheng 2006 warm rain, Stevens & Seifert 2008
// sedimentation) and Limiter (src/limiter.cxx). Kernels and C-ABI entry points; included from k_stencil.hip. The per-cell arithmetic
// is in cell_ops.h (micro_*, limiter_increment). Everything is column-local: no LDS, no neighbour in i or j, any row length.
//
// Microphys_2mom_warm::exec (:639-752) in two passes over the columns:
//   A  walks up. remove_negative_values on qr and nr, the local processes (autoconversion, accretion, evaporation, selfcollection and
//      breakup) with ql from sat_adjust inline, and steps 1-3 of sedimentation_ss08: the sedimentation CFL numbers and the minmod
//      slopes of qr and nr, written to four scratch arrays. rain_mass, rain_diameter, mu_r, lambda_r, w_qr and w_nr, eight of the
//      reference's twelve slice arrays, stay in registers.
//   B  walks down from kend-1 with the flux above in a register: the two gathers over the levels a drop falls through in dt, the
//      limiter against the flux above, the flux divergence, rr_bot at kstart. flux_qr and flux_nr stay in registers.
// Pass A has two forms with the same bits: one thread per column marching over a chunk of levels (w, qr, nr of three levels carried
// in registers), and one thread per cell and level through the generic cell kernel (the three levels recomputed per cell).
#pragma once
#include "k_march_common.h"
#include "thermo_moist.h"
#include <gfx950_prims.h>
#include <wave_reduce.h>

namespace mhh
{
template<class TF>
struct MicroArgs
{
    TF* qr; TF* nr; const TF* thl; const TF* qt; TF* qrt; TF* nrt; TF* thlt; TF* qtt; TF* rr_bot;
    const TF* rho; const TF* p; const TF* exn; const TF* dz; const TF* dzi;
    TF* c_qr; TF* c_nr; TF* s_qr; TF* s_nr; int* nonconv;
    TF nc; double dt; int mask;
    int icells, ijcells, istart, iend, kstart, kend;          // the i bounds and icells: the marching kernel's own frame
};

// qr or nr of level k as the processes see it: remove_negative_values (:51-64) covers the interior levels only, the slopes read
// the ghost levels as the caller left them
template<class TF> __device__ __forceinline__ TF micro_clipped(const MicroArgs<TF>& A, TF v, int k)
{
    return ((A.mask & MICRO_CLIP) && k >= A.kstart && k < A.kend) ? tmax(TF(0.), v) : v;
}

// w_qr and w_nr of level k < kend from its qr, nr (step 1 of sedimentation_ss08); r is the level's prepare_microphysics_slice
template<class TF> __device__ __forceinline__ void micro_w_level(const MicroArgs<TF>& A, int k, TF qr, TF nr, TF b_R, MicroRain<TF>& r, TF& wq, TF& wn)
{
    const TF rho = A.rho[k];
    r = micro_rain(qr, nr, rho);
    const TF rho_n = sqrt(TF(1.2) / rho);
    wq = micro_w_sedi(qr, r, rho_n, b_R, TF(4.));
    wn = micro_w_sedi(qr, r, rho_n, b_R, TF(1.));
}

// One cell of pass A at level k, cell c: qr, nr of k-1, k, k+1 (q[0..2], n[0..2]), w_qr, w_nr of the same three levels with the
// ghost rule of :422-430 applied by the caller, r of level k.
template<class TF> __device__ __forceinline__ void micro_cell_A(const MicroArgs<TF>& A, int k, int c, const TF* q, const TF* n, const TF* wq, const TF* wn,
                                                               const MicroRain<TF>& r)
{
    if (A.mask & MICRO_CLIP) { A.qr[c] = q[1]; A.nr[c] = n[1]; }
    if (A.mask & MICRO_LOCAL)
    {
        const TF rho = A.rho[k], exn = A.exn[k], p = A.p[k];
        const TF thl = A.thl[c], qt = A.qt[c];
        // get_thermo_field("ql_qi"): calc_condensate (src/thermo_moist.cxx:437-457)
        const MoistSat<TF> s = moist_sat_adjust(thl, qt, p, exn);
        moist_count(A.nonconv, s.niter);
        const TF ql = tmax(qt - s.qs, TF(0.));
        MicroTend<TF> t = {A.qrt[c], A.nrt[c], A.thlt[c], A.qtt[c]};
        if (A.mask & MICRO_AUTO) micro_autoconversion(t, q[1], ql, rho, exn, A.nc);
        if (A.mask & MICRO_ACCR) micro_accretion(t, q[1], ql, rho, exn);
        if (A.mask & MICRO_EVAP) micro_evaporation(t, q[1], n[1], ql, qt, thl, rho, exn, p, r);
        if (A.mask & MICRO_SCBR) micro_selfcollection_breakup(t, q[1], n[1], rho, r);
        A.qrt[c] = t.qrt; A.nrt[c] = t.nrt; A.thlt[c] = t.thlt; A.qtt[c] = t.qtt;
    }
    if (A.mask & MICRO_SEDI)
    {
        // steps 2 and 3 (:432-452); dt is a double in both builds
        const TF dzi = A.dzi[k];
        A.c_qr[c] = TF(TF(0.25) * (wq[0] + TF(2.)*wq[1] + wq[2]) * dzi * A.dt);
        A.c_nr[c] = TF(TF(0.25) * (wn[0] + TF(2.)*wn[1] + wn[2]) * dzi * A.dt);
        A.s_qr[c] = micro_minmod(q[1]-q[0], q[2]-q[1]);
        A.s_nr[c] = micro_minmod(n[1]-n[0], n[2]-n[1]);
    }
}

// ---- pass A, one thread per cell and level ------------------------------------------------------------------------------------
template<class TF>
struct MicroClipOp
{
    TF* __restrict__ qr; TF* __restrict__ nr;
    __device__ void operator()(int, int, int, int c) const { qr[c] = tmax(TF(0.), qr[c]); nr[c] = tmax(TF(0.), nr[c]); }
};
// (runs behind MicroClipOp: qr and nr are read as they stand)
template<class TF>
struct MicroCellOp
{
    MicroArgs<TF> A;
    __device__ void operator()(int, int, int k, int c) const
    {
        const int kk = A.ijcells;
        TF q[3], n[3], wq[3] = {TF(0.), TF(0.), TF(0.)}, wn[3] = {TF(0.), TF(0.), TF(0.)};
        MicroRain<TF> r = {TF(0), TF(0), TF(0), TF(0)}, rr;
        q[1] = A.qr[c]; n[1] = A.nr[c];
        const bool sedi = A.mask & MICRO_SEDI;
        if (sedi)
        {
            const TF b_R = micro_b_R<TF>();
            q[0] = A.qr[c-kk]; n[0] = A.nr[c-kk]; q[2] = A.qr[c+kk]; n[2] = A.nr[c+kk];
            micro_w_level(A, k, q[1], n[1], b_R, r, wq[1], wn[1]);
            if (k > A.kstart) micro_w_level(A, k-1, q[0], n[0], b_R, rr, wq[0], wn[0]);
            else              { wq[0] = wq[1]; wn[0] = wn[1]; }
            if (k+1 < A.kend) micro_w_level(A, k+1, q[2], n[2], b_R, rr, wq[2], wn[2]);
        }
        else if (A.mask & (MICRO_EVAP | MICRO_SCBR))
            r = micro_rain(q[1], n[1], A.rho[k]);
        MicroArgs<TF> B = A;
        B.mask &= ~MICRO_CLIP;                     // MicroClipOp has stored the clipped values
        micro_cell_A(B, k, c, q, n, wq, wn, r);
    }
};

// ---- pass A, marching: one thread per column, a wave on one i-row of 64 cells, NJ rows per block, walking up a chunk of kc levels.
// A chunk clips the levels next to its seams itself (max(0, .) gives the same value on either side of a neighbour's store).
constexpr int MICRO_NJ = 4;
template<class TF>
__global__ void __launch_bounds__(64*MICRO_NJ) micro_march_kernel(const MicroArgs<TF> A, const MarchTiling t)
{
    int bx, by, kc;
    if (!decode_march(t, blockIdx.x, bx, by, kc)) return;
    int j0, jlim;
    march_tile_rows(t, by, MICRO_NJ, j0, jlim);
    const int i = A.istart + bx*64 + (int)threadIdx.x, j = j0 + (int)threadIdx.y;
    if (i >= A.iend || j >= jlim) return;                        // a ragged row or tile: the lane sits out (no barrier below)
    const int k0 = A.kstart + kc*t.kc;
    const int k1 = (k0 + t.kc < A.kend) ? k0 + t.kc : A.kend;
    if (k0 >= k1) return;
    const int kk = A.ijcells;
    int c = i + j*A.icells + k0*kk;
    const bool sedi = A.mask & MICRO_SEDI;
    const bool rain = A.mask & (MICRO_EVAP | MICRO_SCBR | MICRO_SEDI);
    const TF b_R = micro_b_R<TF>();
    TF q[3], n[3], wq[3] = {TF(0.), TF(0.), TF(0.)}, wn[3] = {TF(0.), TF(0.), TF(0.)};
    MicroRain<TF> r = {TF(0), TF(0), TF(0), TF(0)}, r_n = r, r_m;
    q[0] = micro_clipped(A, A.qr[c-kk], k0-1); n[0] = micro_clipped(A, A.nr[c-kk], k0-1);
    q[1] = micro_clipped(A, A.qr[c], k0);      n[1] = micro_clipped(A, A.nr[c], k0);
    if (sedi)
    {
        micro_w_level(A, k0, q[1], n[1], b_R, r, wq[1], wn[1]);
        if (k0 > A.kstart) micro_w_level(A, k0-1, q[0], n[0], b_R, r_m, wq[0], wn[0]);
        else               { wq[0] = wq[1]; wn[0] = wn[1]; }
    }
    else if (rain)
        r = micro_rain(q[1], n[1], uniform_load(A.rho, k0));
    for (int k=k0; k<k1; ++k)
    {
        q[2] = micro_clipped(A, A.qr[c+kk], k+1); n[2] = micro_clipped(A, A.nr[c+kk], k+1);
        wq[2] = TF(0.); wn[2] = TF(0.);
        if (sedi)
        {
            if (k+1 < A.kend) micro_w_level(A, k+1, q[2], n[2], b_R, r_n, wq[2], wn[2]);
        }
        else if (rain && k+1 < k1)
            r_n = micro_rain(q[2], n[2], uniform_load(A.rho, k+1));
        micro_cell_A(A, k, c, q, n, wq, wn, r);
        q[0] = q[1]; q[1] = q[2]; n[0] = n[1]; n[1] = n[2];
        wq[0] = wq[1]; wq[1] = wq[2]; wn[0] = wn[1]; wn[1] = wn[2];
        r = r_n;
        c += kk;
    }
}

// ---- pass B: the flux of sedimentation_ss08 (:454-538), one thread per column walking down ------------------------------------
// The gather of level k sums the levels a drop crosses in dt, as far as the sedimentation CFL number of each reaches: its trip
// count differs from lane to lane. The update of cc reads the reference's indices as they stand: for qr the CFL number of the level
// just summed against dzi of the level above it (dzi[kend] on the last turn), for nr against dzi[k].
template<class TF>
__device__ __forceinline__ TF micro_gather(const MicroArgs<TF>& A, int col, int k, const TF* __restrict__ a, const TF* __restrict__ cfl,
                                           const TF* __restrict__ slope, bool dzi_of_k)
{
    int kk = k;
    TF ftot = TF(0), dzz = TF(0);
    TF cc = tmin(TF(1), cfl[col + k*A.ijcells]);
    while (cc > 0 && kk < A.kend)
    {
        const int ckk = col + kk*A.ijcells;
        ftot += A.rho[kk] * (a[ckk] + TF(0.5) * slope[ckk] * (TF(1.)-cc)) * cc * A.dz[kk];
        dzz += A.dz[kk];
        kk  += 1;
        cc   = tmin(TF(1.), cfl[ckk] - dzz*A.dzi[dzi_of_k ? k : kk]);
    }
    return ftot;
}
template<class TF>
struct MicroFluxOp
{
    MicroArgs<TF> A;
    __device__ void operator()(int, int, int, int col) const
    {
        TF fq_up = TF(0.), fn_up = TF(0.), fq = TF(0.), fn = TF(0.);           // the flux at kend is zero
        for (int k=A.kend-1; k>A.kstart-1; --k)
        {
            const int c = col + k*A.ijcells;
            const TF rho = A.rho[k], dz = A.dz[k], dzi = A.dzi[k];
            TF ftot = micro_gather(A, col, k, A.qr, A.c_qr, A.s_qr, false);
            ftot = tmin(ftot, rho * dz * A.qr[c] - fq_up * TF(A.dt));
            fq = TF(-ftot / A.dt);
            ftot = micro_gather(A, col, k, A.nr, A.c_nr, A.s_nr, true);
            ftot = tmin(ftot, rho * dz * A.nr[c] - fn_up * TF(A.dt));
            fn = TF(-ftot / A.dt);
            A.qrt[c] += -(fq_up - fq) / rho * dzi;
            A.nrt[c] += -(fn_up - fn) / rho * dzi;
            fq_up = fq; fn_up = fn;
        }
        A.rr_bot[col] = -fq;
    }
};

template<class TF>
static int micro_exec(const mhh_grid* g, int impl, const mhh_micro_params* P, void* qr, void* nr, const void* thl, const void* qt, void* qrt, void* nrt,
                      void* thlt, void* qtt, void* rr_bot, const void* rhoref, const void* pref, const void* exnref, void* const* scratch, int* nonconv,
                      hipStream_t st)
{
    const bool sedi = P->processes & MICRO_SEDI;
    const MicroArgs<TF> A{mp<TF>(qr), mp<TF>(nr), cp<TF>(thl), cp<TF>(qt), mp<TF>(qrt), mp<TF>(nrt), mp<TF>(thlt), mp<TF>(qtt), mp<TF>(rr_bot),
                          cp<TF>(rhoref), cp<TF>(pref), cp<TF>(exnref), cp<TF>(g->dz), cp<TF>(g->dzi),
                          sedi ? mp<TF>(scratch[0]) : nullptr, sedi ? mp<TF>(scratch[1]) : nullptr, sedi ? mp<TF>(scratch[2]) : nullptr, sedi ? mp<TF>(scratch[3]) : nullptr, nonconv,
                          TF(P->Nc0), P->dt, P->processes,
                          g->icells, g->ijcells, g->istart, g->iend, g->kstart, g->kend};
    const GridDev<TF> gd = make_grid<TF>(g);
    if (impl == MHH_MICRO_IMPL_CELL)
    {
        if (P->processes & MICRO_CLIP)
        {
            MicroClipOp<TF> clip{mp<TF>(qr), mp<TF>(nr)};
            if (int e = launch_interior(st, gd, g->kstart, g->kend, clip)) return e;
        }
        if (P->processes & (MICRO_LOCAL | MICRO_SEDI))
        {
            MicroCellOp<TF> op{A};
            if (int e = launch_interior(st, gd, g->kstart, g->kend, op)) return e;
        }
    }
    else
    {
        const MarchTiling t = make_march_tiling(g, MICRO_NJ, march_kc(g, MarchRows{}, MHH_MOIST_KC, "MHH_MARCH_KC_RT"));
        hipLaunchKernelGGL(micro_march_kernel<TF>, dim3(march_blocks(t)), dim3(64, MICRO_NJ, 1), 0, st, A, t);
        MHH_LAUNCH_CHECK();
    }
    if (sedi)
        return launch_columns(st, gd, 1, MicroFluxOp<TF>{A});
    return MHH_OK;
}

// ---- calc_max_sedimentation_cfl (:163-234): w_qr of three levels in registers, mirrored over BOTH ghost levels -----------------
template<class TF>
__global__ void __launch_bounds__(BX*BY) micro_cfl_kernel(const TF* __restrict__ qr, const TF* __restrict__ nr, const TF* __restrict__ rho,
                                                          const TF* __restrict__ dzi, TF dt, typename Bits<TF>::U* __restrict__ out,
                                                          int i0, int i1, int j0, int j1, int k0, int k1, int jj, int kk)
{
    const int i = i0 + (int)blockIdx.x*BX + (int)threadIdx.x;
    const int j = j0 + (int)blockIdx.y*BY + (int)threadIdx.y;
    TF m = TF(0);
    if (i < i1 && j < j1)
    {
        const TF b_R = micro_b_R<TF>();
        int c = i + j*jj + k0*kk;
        TF wc = micro_w_cfl(qr[c], nr[c], rho[k0], b_R), wm = wc;
        for (int k=k0; k<k1; ++k)
        {
            const TF wp = (k+1 < k1) ? micro_w_cfl(qr[c+kk], nr[c+kk], rho[k+1], b_R) : wc;
            m = tmax(m, TF(0.25) * (wm + TF(2.)*wc + wp) * dzi[k] * dt);
            wm = wc; wc = wp;
            c += kk;
        }
    }
    block_max_publish<TF, BY>(m, out);
}
template<class TF>
static int micro_cfl(const mhh_grid* g, const void* qr, const void* nr, const void* rhoref, double dt, void* work, double* out, hipStream_t st)
{
    using U = typename Bits<TF>::U;
    MHH_HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(micro_cfl_kernel<TF>, dim3((g->imax + BX-1)/BX, (g->jmax + BY-1)/BY, 1), dim3(BX, BY), 0, st, cp<TF>(qr), cp<TF>(nr), cp<TF>(rhoref),
                       cp<TF>(g->dzi), TF(dt), static_cast<U*>(work), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells);
    MHH_LAUNCH_CHECK();
    TF h = 0;
    MHH_HIP_TRY(hipMemcpyAsync(&h, work, sizeof(TF), hipMemcpyDeviceToHost, st));
    MHH_HIP_TRY(hipStreamSynchronize(st));
    *out = static_cast<double>(tmax(TF(1e-5), h));
    return MHH_OK;
}

// ---- Limiter::tendency_limiter (src/limiter.cxx:54-75) --------------------------------------------------------------------------
template<class TF>
struct LimiterOp
{
    TF* __restrict__ at; const TF* __restrict__ a; TF dt, dti;
    __device__ void operator()(int, int, int, int c) const { at[c] += limiter_increment(a[c], at[c], dt, dti); }
};
} // namespace mhh
using namespace mhh;

MHH_API int mhh_micro_2mom_warm_exec_impl(const mhh_grid* g, int impl, const mhh_micro_params* params, void* qr, void* nr, const void* thl, const void* qt,
                                          void* qrt, void* nrt, void* thlt, void* qtt, void* rr_bot, const void* rhoref, const void* pref,
                                          const void* exnref, void* const* scratch, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(impl == MHH_MICRO_IMPL_MARCH || impl == MHH_MICRO_IMPL_CELL, "impl: MHH_MICRO_IMPL_MARCH or MHH_MICRO_IMPL_CELL");
    MHH_REQUIRE(params != nullptr, "null params");
    MHH_REQUIRE((params->processes & ~(MICRO_LOCAL | MICRO_SEDI | MICRO_CLIP)) == 0, "processes: a mask of MHH_MICRO_AUTO ... MHH_MICRO_CLIP");
    MHH_REQUIRE(qr && nr && qrt && nrt && rhoref, "null field");
    MHH_REQUIRE(!(params->processes & MICRO_LOCAL) || (thl && qt && thlt && qtt && pref && exnref), "the local processes need thl, qt, thlt, qtt, pref, exnref");
    MHH_REQUIRE(!(params->processes & MICRO_AUTO) || params->Nc0 > 0., "Nc0");
    MHH_REQUIRE(!(params->processes & MICRO_SEDI) || (scratch && scratch[0] && scratch[1] && scratch[2] && scratch[3] && rr_bot && params->dt > 0.),
                "sedimentation needs four scratch arrays, rr_bot and dt > 0");
    MHH_REQUIRE(g->dz && g->dzi, "the grid's metric arrays");
    MHH_REQUIRE(g->kgc >= 1, "one vertical ghost cell");
    if (params->processes == 0) return MHH_OK;
#define CALL(TF) micro_exec<TF>(g, impl, params, qr, nr, thl, qt, qrt, nrt, thlt, qtt, rr_bot, rhoref, pref, exnref, scratch, nonconv, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_micro_2mom_warm_exec(const mhh_grid* g, const mhh_micro_params* params, void* qr, void* nr, const void* thl, const void* qt,
                                     void* qrt, void* nrt, void* thlt, void* qtt, void* rr_bot, const void* rhoref, const void* pref,
                                     const void* exnref, void* const* scratch, int* nonconv, void* stream)
{
    return mhh_micro_2mom_warm_exec_impl(g, MHH_MICRO_IMPL_MARCH, params, qr, nr, thl, qt, qrt, nrt, thlt, qtt, rr_bot, rhoref, pref, exnref, scratch,
                                         nonconv, stream);
}

MHH_API int mhh_micro_2mom_warm_cfl(const mhh_grid* g, const void* qr, const void* nr, const void* rhoref, double dt, void* work, double* out, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(qr && nr && rhoref, "null field");
    MHH_REQUIRE(work && out, "null work/out");
    MHH_REQUIRE(g->dzi, "the grid's metric arrays");
#define CALL(TF) micro_cfl<TF>(g, qr, nr, rhoref, dt, work, out, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

MHH_API int mhh_limiter_exec(const mhh_grid* g, void* at, const void* a, double dt, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(at && a, "null field");
    MHH_REQUIRE(dt > 0., "dt");
#define CALL(TF) [&]{ const TF d = TF(dt); LimiterOp<TF> op{mp<TF>(at), cp<TF>(a), d, TF(1.)/d}; \
                      return launch_interior(as_stream(stream), make_grid<TF>(g), g->kstart, g->kend, op); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
