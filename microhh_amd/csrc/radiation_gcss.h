// radiation_gcss.h -- Radiation_gcss (src/radiation_gcss.cxx: the GCSS long- and short-wave fluxes of the DYCOMS case), the CPU
// path of the reference. Kernels and C-ABI entry points; included from k_stencil.hip. The arithmetic is in cell_ops.h (rad_gcss_*).
// Everything is column-local: one thread per column, a wave on 64 consecutive i of a row, no LDS, no neighbour in i or j, any row
// length (a ragged row's lanes sit out).
//
// exec_gcss_rad (:253-309) needs of a column, before any flux can be formed, the totals lwp and tauc and the inversion index ki,
// which are known only after a full upward sweep. Two forms with the same bits:
//   0  two sweeps in one kernel. Up: lwp, tauc, ki, with flx_up = fr1*exp(-xka*lwp_cum) of :228 to ONE scratch field. Down from
//      kend-1: the long-wave flux from flx_up and the column's constants, the short-wave flux along taupath (tau[k] formed again
//      from ql), the flux of the level above in registers, thlt read and written once per cell.
//   1  the reference's own sequence: a column kernel per flux that keeps the whole flux array (calc_gcss_rad_LW :203-252,
//      calc_gcss_rad_SW + sunray :101-200), then a cell kernel for thlt (:273-307).
// ql is the caller's or, without one, moist_sat_adjust per cell into scratch 0 (get_thermo_field("ql"), :361).
#pragma once
#include "k_march_common.h"
#include "thermo_moist.h"

namespace mhh
{
template<class TF>
struct RadArgs
{
    TF* thlt; const TF* ql; const TF* qt; const TF* rho; const TF* z; const TF* dzhi;
    TF* flx; TF* swn;          // form 0: flx holds flx_up between the sweeps, swn is unused; form 1: the two flux arrays
    TF* lflx; TF* sflx;        // form 0: the outputs asked for (NULL: none)
    TF xka, fr0, fr1, div, mu;
    int lw, sw, lw_tend, sw_tend;
    int icells, ijcells, istart, iend, jstart, jend, kstart, kend;
};
constexpr int RAD_NJ = 4;

// the constants of a column's long-wave flux: what :233-243 form from ki and the total lwp
template<class TF> struct RadLw { TF fact, down_kstart; double down_above; int ki; };
template<class TF> __device__ __forceinline__ RadLw<TF> rad_lw_column(const RadArgs<TF>& A, TF lwp, int ki)
{
    RadLw<TF> L;
    L.fact = rad_gcss_fact(A.div, A.rho[ki]);
    L.down_kstart = rad_gcss_down_kstart(A.fr0, A.xka, lwp);
    L.down_above = rad_gcss_down_above(A.fr0, A.xka, lwp);       // a double exp in fp32 too: once per column
    L.ki = ki;
    return L;
}
// thlt of level kt from the fluxes of kt and of km = max(kstart+1, kt-1): the long-wave term first, then the short-wave one
template<class TF> __device__ __forceinline__ void rad_tend(const RadArgs<TF>& A, int c, int kt, TF f, TF fm, TF s, TF sm)
{
    const TF dzhi = A.dzhi[kt], rho = A.rho[kt];
    TF tt = A.thlt[c];
    if (A.lw_tend) tt = tt - rad_gcss_tend(f, fm, dzhi, rho);
    if (A.sw_tend) tt = tt + rad_gcss_tend(s, sm, dzhi, rho);
    A.thlt[c] = tt;
}

// ---- form 0 ----------------------------------------------------------------------------------------------------------------------
template<class TF>
__global__ void __launch_bounds__(64*RAD_NJ) rad_sweep_kernel(const RadArgs<TF> A)
{
    const int i = A.istart + (int)blockIdx.x*64 + (int)threadIdx.x, j = A.jstart + (int)blockIdx.y*RAD_NJ + (int)threadIdx.y;
    if (i >= A.iend || j >= A.jend) return;
    const int col = i + j*A.icells, kk = A.ijcells;
    TF lwp = TF(0.0), tauc = TF(0.0);
    int ki = A.kend;
    for (int k=A.kstart; k<A.kend; ++k)
    {
        const int c = col + k*kk;
        const TF ql = A.ql[c], rho = A.rho[k], depth = rad_gcss_depth(A.z, k);
        if (A.lw)
        {
            lwp = rad_gcss_lwp(lwp, ql, rho, depth);
            A.flx[c] = rad_gcss_flx_up(A.fr1, A.xka, lwp);
            if (rad_gcss_in_pbl(ql, A.qt[c])) ki = k;
        }
        if (A.sw) tauc = tauc + rad_gcss_tau(ql, rho, depth);
    }
    RadLw<TF> L = {TF(0.), TF(0.), 0., ki};
    RadSun<TF> S = {TF(0.), TF(0.), TF(0.), TF(0.), TF(0.), TF(0.)};
    if (A.lw) L = rad_lw_column(A, lwp, ki);
    if (A.sw) S = rad_gcss_sunray(A.mu, tauc);
    const bool tend = A.lw_tend || A.sw_tend;
    TF f_up = TF(0.), s_up = TF(0.), taupath = TF(0.);           // the fluxes of level k+1
    for (int k=A.kend-1; k>=A.kstart; --k)
    {
        const int c = col + k*kk;
        TF f = TF(0.), s = TF(0.);
        if (A.lw)
        {
            f = rad_gcss_flx(A.flx[c], k, A.kstart, L.down_kstart, L.down_above, L.ki, L.fact, A.z);
            if (A.lflx) A.lflx[c] = f;
        }
        if (A.sw)
        {
            taupath = rad_gcss_taupath(S, taupath, rad_gcss_tau(A.ql[c], A.rho[k], rad_gcss_depth(A.z, k)));
            s = rad_gcss_swn(S, A.mu, taupath);
            if (A.sflx) A.sflx[c] = s;
        }
        if (tend && k > A.kstart)
        {
            if (k+1 < A.kend)    rad_tend(A, c + kk, k+1, f_up, f, s_up, s);
            if (k == A.kstart+1) rad_tend(A, c, k, f, f, s, s);
        }
        f_up = f; s_up = s;
    }
}

// ---- form 1 ----------------------------------------------------------------------------------------------------------------------
template<class TF>
__global__ void __launch_bounds__(64*RAD_NJ) rad_lw_kernel(const RadArgs<TF> A)
{
    const int i = A.istart + (int)blockIdx.x*64 + (int)threadIdx.x, j = A.jstart + (int)blockIdx.y*RAD_NJ + (int)threadIdx.y;
    if (i >= A.iend || j >= A.jend) return;
    const int col = i + j*A.icells, kk = A.ijcells;
    TF lwp = TF(0.0);
    int ki = A.kend;
    for (int k=A.kstart; k<A.kend; ++k)
    {
        const int c = col + k*kk;
        const TF ql = A.ql[c];
        lwp = rad_gcss_lwp(lwp, ql, A.rho[k], rad_gcss_depth(A.z, k));
        A.flx[c] = rad_gcss_flx_up(A.fr1, A.xka, lwp);
        if (rad_gcss_in_pbl(ql, A.qt[c])) ki = k;
    }
    const RadLw<TF> L = rad_lw_column(A, lwp, ki);
    for (int k=A.kstart; k<A.kend; ++k)
    {
        const int c = col + k*kk;
        A.flx[c] = rad_gcss_flx(A.flx[c], k, A.kstart, L.down_kstart, L.down_above, L.ki, L.fact, A.z);
    }
}
// (swn may be the array ql lives in: a level's ql is read in front of the store of its swn, by the same lane)
template<class TF>
__global__ void __launch_bounds__(64*RAD_NJ) rad_sw_kernel(const RadArgs<TF> A)
{
    const int i = A.istart + (int)blockIdx.x*64 + (int)threadIdx.x, j = A.jstart + (int)blockIdx.y*RAD_NJ + (int)threadIdx.y;
    if (i >= A.iend || j >= A.jend) return;
    const int col = i + j*A.icells, kk = A.ijcells;
    TF tauc = TF(0.0);
    for (int k=A.kstart; k<A.kend; ++k)
        tauc = tauc + rad_gcss_tau(A.ql[col + k*kk], A.rho[k], rad_gcss_depth(A.z, k));
    const RadSun<TF> S = rad_gcss_sunray(A.mu, tauc);
    TF taupath = TF(0.);
    for (int k=A.kend-1; k>=A.kstart; --k)
    {
        const int c = col + k*kk;
        taupath = rad_gcss_taupath(S, taupath, rad_gcss_tau(A.ql[c], A.rho[k], rad_gcss_depth(A.z, k)));
        A.swn[c] = rad_gcss_swn(S, A.mu, taupath);
    }
}
template<class TF>
struct RadTendOp
{
    RadArgs<TF> A;
    __device__ void operator()(int, int, int k, int c) const
    {
        const int cm = c + (((A.kstart+1 < k-1) ? k-1 : A.kstart+1) - k)*A.ijcells;
        rad_tend(A, c, k, A.lw_tend ? A.flx[c] : TF(0.), A.lw_tend ? A.flx[cm] : TF(0.), A.sw_tend ? A.swn[c] : TF(0.), A.sw_tend ? A.swn[cm] : TF(0.));
    }
};

template<class TF>
static int rad_exec(const mhh_grid* g, int impl, const mhh_radiation_gcss_params* P, void* thlt, const void* ql_in, const void* thl, const void* qt,
                    const void* rhoref, const void* pref, const void* exnref, void* lflx, void* sflx, void* const* scratch, int* nonconv, hipStream_t st)
{
    const GridDev<TF> gd = make_grid<TF>(g);
    const TF mu = TF(P->mu);
    const bool day = mu > rad_gcss_mu_min<TF>();
    const bool lw_tend = thlt && (P->parts & RAD_LW), sw_tend = thlt && (P->parts & RAD_SW) && day;
    const bool lw = lw_tend || lflx, sw = sw_tend || (sflx && day);
    if (sflx)                                                      // :175-176, :432-433: all ncells, the ghost cells included
        MHH_HIP_TRY(hipMemsetAsync(sflx, 0, sizeof(TF)*(size_t)g->ncells, st));
    if (!lw && !sw) return MHH_OK;
    const TF* ql = cp<TF>(ql_in);
    if (!ql)
    {
        MoistFieldsOp<TF> op{gd, cp<TF>(thl), cp<TF>(qt), cp<TF>(pref), cp<TF>(exnref), nullptr, nullptr, mp<TF>(scratch[0]), nullptr, nullptr, nonconv};
        if (int e = launch_interior(st, gd, g->kstart, g->kend, op)) return e;
        ql = cp<TF>(scratch[0]);
    }
    RadArgs<TF> A{mp<TF>(thlt), ql, cp<TF>(qt), cp<TF>(rhoref), cp<TF>(g->z), cp<TF>(g->dzhi), mp<TF>(scratch[1]), nullptr, mp<TF>(lflx), mp<TF>(sflx),
                  TF(P->xka), TF(P->fr0), TF(P->fr1), TF(P->div), mu, lw, sw, lw_tend, sw_tend,
                  g->icells, g->ijcells, g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend};
    const dim3 grid((g->imax + 63)/64, (g->jmax + RAD_NJ-1)/RAD_NJ, 1), block(64, RAD_NJ, 1);
    if (impl == MHH_RAD_IMPL_SWEEP)
    {
        hipLaunchKernelGGL(rad_sweep_kernel<TF>, grid, block, 0, st, A);
        MHH_LAUNCH_CHECK();
        return MHH_OK;
    }
    // the flux arrays: the caller's output where there is one, else scratch 1 (long wave) and scratch 0 (short wave, over ql where
    // ql was put there: the long-wave kernel has read it by then)
    A.flx = lflx ? mp<TF>(lflx) : mp<TF>(scratch[1]);
    A.swn = sflx ? mp<TF>(sflx) : mp<TF>(scratch[0]);
    if (lw)
    {
        hipLaunchKernelGGL(rad_lw_kernel<TF>, grid, block, 0, st, A);
        MHH_LAUNCH_CHECK();
    }
    if (sw)
    {
        hipLaunchKernelGGL(rad_sw_kernel<TF>, grid, block, 0, st, A);
        MHH_LAUNCH_CHECK();
    }
    if (lw_tend || sw_tend)
    {
        RadTendOp<TF> op{A};
        if (int e = launch_interior(st, gd, g->kstart+1, g->kend, op)) return e;
    }
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

MHH_API int mhh_radiation_gcss_zenith_host(int dtype, double lat, double lon, double day_of_year, double* mu)
{
    MHH_REQUIRE(dtype == MHH_F64 || dtype == MHH_F32, "dtype must be MHH_F64 or MHH_F32");
    MHH_REQUIRE(mu != nullptr, "null mu");
    // gd.lat and gd.lon are TF (:363)
    *mu = (dtype == MHH_F64) ? rad_gcss_zenith<double>(lat, lon, day_of_year) : (double)rad_gcss_zenith<float>((float)lat, (float)lon, day_of_year);
    return MHH_OK;
}

MHH_API int mhh_radiation_gcss_exec_impl(const mhh_grid* g, int impl, const mhh_radiation_gcss_params* params, void* thlt, const void* ql, const void* thl,
                                         const void* qt, const void* rhoref, const void* pref, const void* exnref, void* lflx, void* sflx,
                                         void* const* scratch, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(impl == MHH_RAD_IMPL_SWEEP || impl == MHH_RAD_IMPL_PLAIN, "impl: MHH_RAD_IMPL_SWEEP or MHH_RAD_IMPL_PLAIN");
    MHH_REQUIRE(params != nullptr, "null params");
    MHH_REQUIRE(params->parts != 0 && (params->parts & ~(RAD_LW | RAD_SW)) == 0, "parts: MHH_RAD_LW, MHH_RAD_SW or both");
    MHH_REQUIRE(qt && rhoref, "null field");
    MHH_REQUIRE(ql || (thl && pref && exnref), "without ql the saturation adjustment needs thl, pref and exnref");
    MHH_REQUIRE(scratch && scratch[0] && scratch[1], "two scratch fields");
    MHH_REQUIRE(thlt || lflx || sflx, "no output asked for");
    MHH_REQUIRE(g->z && g->dzhi, "the grid's metric arrays");
    MHH_REQUIRE(g->kgc >= 1, "one vertical ghost cell");
#define CALL(TF) rad_exec<TF>(g, impl, params, thlt, ql, thl, qt, rhoref, pref, exnref, lflx, sflx, scratch, nonconv, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_radiation_gcss_exec(const mhh_grid* g, const mhh_radiation_gcss_params* params, void* thlt, const void* ql, const void* thl,
                                    const void* qt, const void* rhoref, const void* pref, const void* exnref, void* lflx, void* sflx,
                                    void* const* scratch, int* nonconv, void* stream)
{
    return mhh_radiation_gcss_exec_impl(g, MHH_RAD_IMPL_SWEEP, params, thlt, ql, thl, qt, rhoref, pref, exnref, lflx, sflx, scratch, nonconv, stream);
}
