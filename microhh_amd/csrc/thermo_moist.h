// thermo_moist.h -- Thermo_moist (src/thermo_moist.cxx, include/thermo_moist_functions.h): the buoyancy tendency of w with its
// saturation adjustment per cell, the diagnostic fields b / ql / qi / T, and the hydrostatic base state on the host and on the
// device. Kernels and C-ABI entry points; included from k_stencil.hip. The per-cell arithmetic is in cell_ops.h (moist_*).
#pragma once
#include "k_march_common.h"
#include <gfx950_prims.h>

namespace mhh
{
// One more cell on which the reference would throw "Non-converging saturation adjustment" (thermo_moist_functions.h:277-288):
// a vector atomic on the caller's counter (NULL: not counted). The lane keeps the value of its tenth iterate.
__device__ __forceinline__ void moist_count(int* nonconv, int niter)
{
    if (niter == moist_nitermax && nonconv)
    {
#if defined(__HIPCC__)
        atomicAdd(nonconv, 1);
#else
        __atomic_fetch_add(nonconv, 1, __ATOMIC_RELAXED);
#endif
    }
}

// =======================================================================================================
// sat_adjust on n independent cells (thl, qt, p, exn per cell): the point functions behind a call of their own
// =======================================================================================================
template<class TF>
__global__ void __launch_bounds__(256) moist_sat_adjust_kernel(long long n, const TF* __restrict__ thl, const TF* __restrict__ qt, const TF* __restrict__ p,
                                                               const TF* __restrict__ exn, TF* __restrict__ ql, TF* __restrict__ qi,
                                                               TF* __restrict__ t, TF* __restrict__ qs, int* nonconv)
{
    const long long c = (long long)blockIdx.x*256 + threadIdx.x;
    if (c >= n) return;
    const MoistSat<TF> s = moist_sat_adjust(thl[c], qt[c], p[c], exn[c]);
    moist_count(nonconv, s.niter);
    if (ql) ql[c] = s.ql;
    if (qi) qi[c] = s.qi;
    if (t)  t[c]  = s.t;
    if (qs) qs[c] = s.qs;
}

// =======================================================================================================
// calc_buoyancy_tend_2nd (src/thermo_moist.cxx:78-120), k in (kstart, kend)
// =======================================================================================================
// the one-thread-per-cell form: six array passes (thl and qt of two levels, wt read and written)
template<class TF>
struct MoistTendOp
{
    GridDev<TF> g; TF* __restrict__ wt; const TF* __restrict__ thl; const TF* __restrict__ qt;
    const TF* __restrict__ prefh; const TF* __restrict__ exnrefh; const TF* __restrict__ thvrefh; int* nonconv;
    __device__ void operator()(int, int, int k, int c) const
    {
        const TF exnh = exnrefh[k];
        const TF thlh = i2(thl[c-g.ijcells], thl[c]);
        const TF qth  = i2(qt[c-g.ijcells], qt[c]);
        const MoistSat<TF> s = moist_sat_adjust(thlh, qth, prefh[k], exnh);
        moist_count(nonconv, s.niter);
        wt[c] += moist_buoyancy(exnh, thlh, qth, s.ql, s.qi, thvrefh[k]);
    }
};

// The marching form: one thread per column, a wave on one i-row of 64 cells, NJ rows per block, walking up a chunk of kc levels.
// thl and qt of the level below stay in registers, so a level costs two loads and one read-modify-write of wt (four array
// passes); the loads of the next level are issued in front of the Newton loop, whose trip count differs from lane to lane (each
// lane leaves the loop after its own last iteration; the wave goes on when its slowest lane has). The three reference profiles
// are wave-uniform table loads on the scalar cache. No LDS, no neighbour in i or j: any row alignment, any jtot.
#ifndef MHH_MOIST_KC
#define MHH_MOIST_KC 32
#endif
constexpr int MOIST_NJ = 4;
template<class TF>
struct MoistMarchArgs
{
    TF* wt; const TF* thl; const TF* qt; const TF* prefh; const TF* exnrefh; const TF* thvrefh; int* nonconv;
    int icells, ijcells, istart, iend, kstart, kend;
};
template<class TF>
__global__ void __launch_bounds__(64*MOIST_NJ) moist_tend_march_kernel(const MoistMarchArgs<TF> A, const MarchTiling t)
{
    int bx, by, kc;
    if (!decode_march(t, blockIdx.x, bx, by, kc)) return;
    int j0, jlim;
    march_tile_rows(t, by, MOIST_NJ, j0, jlim);
    const int i = A.istart + bx*64 + (int)threadIdx.x, j = j0 + (int)threadIdx.y;
    if (i >= A.iend || j >= jlim) return;                        // a ragged row or tile: the lane sits out (no barrier below)
    int k0 = A.kstart + kc*t.kc;
    const int k1 = (k0 + t.kc < A.kend) ? k0 + t.kc : A.kend;
    if (k0 == A.kstart) ++k0;                                     // w at kstart has no buoyancy
    if (k0 >= k1) return;
    const int kk = A.ijcells;
    int c = i + j*A.icells + k0*kk;
    TF* __restrict__ wt = A.wt; const TF* __restrict__ thl = A.thl; const TF* __restrict__ qt = A.qt;
    TF thl_m = thl[c-kk], qt_m = qt[c-kk];
    TF thl_n = thl[c], qt_n = qt[c], wt_n = stream_load(wt + c);
    for (int k=k0; k<k1; ++k)
    {
        const TF thl_c = thl_n, qt_c = qt_n, wt_c = wt_n;
        if (k+1 < k1)                                             // wave-uniform: the next level's values are on their way during the loop
        {
            thl_n = thl[c+kk]; qt_n = qt[c+kk]; wt_n = stream_load(wt + c + kk);
        }
        const TF ph = uniform_load(A.prefh, k), exnh = uniform_load(A.exnrefh, k), thvh = uniform_load(A.thvrefh, k);
        const TF thlh = i2(thl_m, thl_c);
        const TF qth  = i2(qt_m, qt_c);
        const MoistSat<TF> s = moist_sat_adjust(thlh, qth, ph, exnh);
        moist_count(A.nonconv, s.niter);
        stream_store(wt + c, wt_c + moist_buoyancy(exnh, thlh, qth, s.ql, s.qi, thvh));
        thl_m = thl_c; qt_m = qt_c;
        c += kk;
    }
}

template<class TF>
static int moist_tend(const mhh_grid* g, int impl, void* wt, const void* thl, const void* qt, const void* prefh, const void* exnrefh,
                      const void* thvrefh, int* nonconv, hipStream_t st)
{
    if (g->kmax < 2) return MHH_OK;
    if (impl == MHH_MOIST_IMPL_CELL)
    {
        MoistTendOp<TF> op{make_grid<TF>(g), mp<TF>(wt), cp<TF>(thl), cp<TF>(qt), cp<TF>(prefh), cp<TF>(exnrefh), cp<TF>(thvrefh), nonconv};
        return launch_interior(st, op.g, g->kstart+1, g->kend, op);
    }
    const MarchTiling t = make_march_tiling(g, MOIST_NJ, march_kc(g, MarchRows{}, MHH_MOIST_KC, "MHH_MARCH_KC_RT"));
    const MoistMarchArgs<TF> A{mp<TF>(wt), cp<TF>(thl), cp<TF>(qt), cp<TF>(prefh), cp<TF>(exnrefh), cp<TF>(thvrefh), nonconv,
                               g->icells, g->ijcells, g->istart, g->iend, g->kstart, g->kend};
    hipLaunchKernelGGL(moist_tend_march_kernel<TF>, dim3(march_blocks(t)), dim3(64, MOIST_NJ, 1), 0, st, A, t);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// =======================================================================================================
// get_thermo_field: calc_buoyancy (:123-167), calc_liquid_water (:231-250), calc_ice (:414-434), calc_T (:478-496) in one pass
// =======================================================================================================
template<class TF>
struct MoistFieldsOp
{
    GridDev<TF> g; const TF* __restrict__ thl; const TF* __restrict__ qt;
    const TF* __restrict__ pref; const TF* __restrict__ exnref; const TF* __restrict__ thvref;
    TF* __restrict__ b; TF* __restrict__ ql; TF* __restrict__ qi; TF* __restrict__ T; int* nonconv;
    __device__ void operator()(int, int, int k, int c) const
    {
        if (k >= g.kstart && k < g.kend)
        {
            const TF ex = exnref[k];
            const MoistSat<TF> s = moist_sat_adjust(thl[c], qt[c], pref[k], ex);
            moist_count(nonconv, s.niter);
            if (ql) ql[c] = s.ql;
            if (qi) qi[c] = s.qi;
            if (T)  T[c]  = s.t;
            if (b)  b[c]  = moist_buoyancy(ex, thl[c], qt[c], s.ql, s.qi, thvref[k]);
        }
        // the ghost levels of b: ql = qi = 0, so Lv*ql/(cp*ex) is +0 whatever positive ex is -- the table's exnref is not read,
        // which the base state leaves unset below kstart, where the reference takes exner(pref[k]) (:134)
        else if (b) b[c] = moist_buoyancy(TF(1.), thl[c], qt[c], TF(0.), TF(0.), thvref[k]);
    }
};

// =======================================================================================================
// get_thermo_field("ql_h"): calc_liquid_water_h (:368-411). thl and qt interpolated to the half level, the saturation adjustment
// at prefh; levels kstart+1 .. kend, and zero at kstart. exnrefh[k] is the table's exner(prefh[k]), the reference's `exnh`.
// =======================================================================================================
template<class TF>
struct MoistQlhOp
{
    GridDev<TF> g; const TF* __restrict__ thl; const TF* __restrict__ qt;
    const TF* __restrict__ prefh; const TF* __restrict__ exnrefh; TF* __restrict__ qlh; int* nonconv;
    __device__ void operator()(int, int, int k, int c) const
    {
        if (k == g.kstart) { qlh[c] = TF(0.); return; }
        const MoistSat<TF> s = moist_sat_adjust(i2(thl[c-g.ijcells], thl[c]), i2(qt[c-g.ijcells], qt[c]), prefh[k], exnrefh[k]);
        moist_count(nonconv, s.niter);
        qlh[c] = s.ql;
    }
};

// =======================================================================================================
// calc_base_state (thermo_moist_functions.h:293-349), statement by statement. OUT writes through to the caller's profile where
// there is one; what the recurrence itself reads back (the pressures) it keeps in registers.
// =======================================================================================================
template<class TF> MHH_HD void moist_put(TF* a, int k, TF v) { if (a) a[k] = v; }
template<class TF>
MHH_HD int moist_base_state(TF* pref, TF* prefh, TF* rho, TF* rhoh, TF* thv, TF* thvh, TF* ex, TF* exh,
                            const TF* thlmean, const TF* qtmean, TF pbot, int kstart, int kend, const TF* z, const TF* dz, const TF* dzh)
{
    typedef MoistC<TF> K;
    int nonconv = 0;
    const TF thlsurf = TF(0.5)*(thlmean[kstart-1] + thlmean[kstart]);
    const TF qtsurf  = TF(0.5)*(qtmean [kstart-1] + qtmean[kstart]);
    TF ph = pbot;
    moist_put(prefh, kstart, ph);
    TF exh_k = moist_exner(ph);
    moist_put(exh, kstart, exh_k);
    MoistSat<TF> ssa = moist_sat_adjust(thlsurf, qtsurf, ph, exh_k);
    nonconv += (ssa.niter == moist_nitermax);
    TF thvh_k = moist_virtual_temperature(exh_k, thlsurf, qtsurf, ssa.ql, ssa.qi);
    moist_put(thvh, kstart, thvh_k);
    moist_put(rhoh, kstart, pbot / (K::Rd * exh_k * thvh_k));
    TF p = ph * std::exp(-K::grav * z[kstart] / (K::Rd * exh_k * thvh_k));
    const TF pref_kstart = p;
    moist_put(pref, kstart, p);
    for (int k=kstart+1; k<kend+1; ++k)
    {
        const TF ex_m = moist_exner(p);
        moist_put(ex, k-1, ex_m);
        ssa = moist_sat_adjust(thlmean[k-1], qtmean[k-1], p, ex_m);
        nonconv += (ssa.niter == moist_nitermax);
        const TF thv_m = moist_virtual_temperature(ex_m, thlmean[k-1], qtmean[k-1], ssa.ql, ssa.qi);
        moist_put(thv, k-1, thv_m);
        moist_put(rho, k-1, p / (K::Rd * ex_m * thv_m));

        ph = ph * std::exp(-K::grav * dz[k-1] / (K::Rd * ex_m * thv_m));
        moist_put(prefh, k, ph);
        exh_k = moist_exner(ph);
        moist_put(exh, k, exh_k);

        const TF thli = TF(0.5)*(thlmean[k-1] + thlmean[k]);
        const TF qti  = TF(0.5)*(qtmean [k-1] + qtmean [k]);
        ssa = moist_sat_adjust(thli, qti, ph, exh_k);
        nonconv += (ssa.niter == moist_nitermax);
        thvh_k = moist_virtual_temperature(exh_k, thli, qti, ssa.ql, ssa.qi);
        moist_put(thvh, k, thvh_k);
        moist_put(rhoh, k, ph / (K::Rd * exh_k * thvh_k));

        p = p * std::exp(-K::grav * dzh[k] / (K::Rd * exh_k * thvh_k));
        moist_put(pref, k, p);
    }
    moist_put(pref, kstart-1, TF(2.)*pbot - pref_kstart);
    return nonconv;
}

// The chain over the levels is serial (pow, sat_adjust, exp, twice per level): one thread walks it, on the stream, so a
// captured step holds it and nothing goes through the host.
template<class TF>
struct MoistBaseArgs
{
    TF* pref; TF* prefh; TF* rho; TF* rhoh; TF* thv; TF* thvh; TF* ex; TF* exh;
    const TF* thlmean; const TF* qtmean; const TF* z; const TF* dz; const TF* dzh; int* nonconv;
    TF pbot; int kstart, kend;
};
template<class TF>
__global__ void __launch_bounds__(64) moist_base_state_kernel(const MoistBaseArgs<TF> A)
{
    const int n = moist_base_state(A.pref, A.prefh, A.rho, A.rhoh, A.thv, A.thvh, A.ex, A.exh, A.thlmean, A.qtmean, A.pbot, A.kstart, A.kend, A.z, A.dz, A.dzh);
    if (n && A.nonconv)
    {
#if defined(__HIPCC__)
        atomicAdd(A.nonconv, n);
#else
        __atomic_fetch_add(A.nonconv, n, __ATOMIC_RELAXED);
#endif
    }
}
} // namespace mhh
using namespace mhh;

MHH_API int mhh_thermo_moist_sat_adjust(int dtype, long long n, const void* thl, const void* qt, const void* p, const void* exn,
                                        void* ql, void* qi, void* t, void* qs, int* nonconv, void* stream)
{
    MHH_REQUIRE(dtype == MHH_F64 || dtype == MHH_F32, "dtype must be MHH_F64 or MHH_F32");
    MHH_REQUIRE(n >= 0 && n < (1LL << 31) * 256, "n");
    MHH_REQUIRE(thl && qt && p && exn, "null input");
    if (n == 0) return MHH_OK;
    const dim3 grid((unsigned)((n + 255)/256));
    if (dtype == MHH_F64)
        hipLaunchKernelGGL(moist_sat_adjust_kernel<double>, grid, dim3(256), 0, as_stream(stream), n, cp<double>(thl), cp<double>(qt), cp<double>(p),
                           cp<double>(exn), mp<double>(ql), mp<double>(qi), mp<double>(t), mp<double>(qs), nonconv);
    else
        hipLaunchKernelGGL(moist_sat_adjust_kernel<float>, grid, dim3(256), 0, as_stream(stream), n, cp<float>(thl), cp<float>(qt), cp<float>(p),
                           cp<float>(exn), mp<float>(ql), mp<float>(qi), mp<float>(t), mp<float>(qs), nonconv);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

MHH_API int mhh_thermo_moist_buoyancy_tend_impl(const mhh_grid* g, int impl, void* wt, const void* thl, const void* qt, const void* prefh,
                                                const void* exnrefh, const void* thvrefh, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(impl == MHH_MOIST_IMPL_MARCH || impl == MHH_MOIST_IMPL_CELL, "impl: MHH_MOIST_IMPL_MARCH or MHH_MOIST_IMPL_CELL");
    MHH_REQUIRE(wt && thl && qt && prefh && exnrefh && thvrefh, "null field");
    MHH_REQUIRE(g->kgc >= 1, "one vertical ghost cell");
#define CALL(TF) moist_tend<TF>(g, impl, wt, thl, qt, prefh, exnrefh, thvrefh, nonconv, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_thermo_moist_buoyancy_tend(const mhh_grid* g, void* wt, const void* thl, const void* qt, const void* prefh,
                                           const void* exnrefh, const void* thvrefh, int* nonconv, void* stream)
{
    return mhh_thermo_moist_buoyancy_tend_impl(g, MHH_MOIST_IMPL_MARCH, wt, thl, qt, prefh, exnrefh, thvrefh, nonconv, stream);
}

MHH_API int mhh_thermo_moist_fields(const mhh_grid* g, const void* thl, const void* qt, const void* pref, const void* exnref, const void* thvref,
                                    void* b, void* ql, void* qi, void* T, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(thl && qt && pref && exnref, "null field");
    MHH_REQUIRE(b || ql || qi || T, "no output asked for");
    MHH_REQUIRE(!b || thvref, "b needs thvref");
    // b covers every level (calc_buoyancy runs k over kcells), the other three the interior
#define CALL(TF) [&]{ MoistFieldsOp<TF> op{make_grid<TF>(g), cp<TF>(thl), cp<TF>(qt), cp<TF>(pref), cp<TF>(exnref), cp<TF>(thvref), \
                                           mp<TF>(b), mp<TF>(ql), mp<TF>(qi), mp<TF>(T), nonconv}; \
                      return launch_interior(as_stream(stream), op.g, b ? 0 : g->kstart, b ? g->kcells : g->kend, op); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

MHH_API int mhh_thermo_moist_ql_h(const mhh_grid* g, const void* thl, const void* qt, const void* prefh, const void* exnrefh, void* ql_h,
                                  int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(thl && qt && prefh && exnrefh && ql_h, "null field");
    MHH_REQUIRE(g->kgc >= 1, "the half level kend reads the ghost level of thl and qt");
#define CALL(TF) [&]{ MoistQlhOp<TF> op{make_grid<TF>(g), cp<TF>(thl), cp<TF>(qt), cp<TF>(prefh), cp<TF>(exnrefh), mp<TF>(ql_h), nonconv}; \
                      return launch_interior(as_stream(stream), op.g, g->kstart, g->kend + 1, op); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_top_and_bot (src/thermo_moist.cxx:58-75)
template<class TF>
static void moist_top_and_bot(TF* thl0, TF* qt0, const TF* z, const TF* zh, const TF* dzhi, int kstart, int kend)
{
    TF thl0s, qt0s, thl0t, qt0t;
    thl0s = thl0[kstart] - z[kstart]*(thl0[kstart+1]-thl0[kstart])*dzhi[kstart+1];
    qt0s  = qt0[kstart]  - z[kstart]*(qt0[kstart+1] -qt0[kstart] )*dzhi[kstart+1];
    thl0t = thl0[kend-1] + (zh[kend]-z[kend-1])*(thl0[kend-1]-thl0[kend-2])*dzhi[kend-1];
    qt0t  = qt0[kend-1]  + (zh[kend]-z[kend-1])*(qt0[kend-1]- qt0[kend-2] )*dzhi[kend-1];
    thl0[kstart-1]  = TF(2.)*thl0s - thl0[kstart];
    thl0[kend]      = TF(2.)*thl0t - thl0[kend-1];
    qt0[kstart-1]   = TF(2.)*qt0s  - qt0[kstart];
    qt0[kend]       = TF(2.)*qt0t  - qt0[kend-1];
}
template<class TF>
static int moist_base_state_host(const mhh_grid* g, void* thl0, void* qt0, double pbot, int boussinesq, double thvref0,
                                 void* pref, void* prefh, void* rhoref, void* rhorefh, void* thvref, void* thvrefh, void* exnref, void* exnrefh, int* nonconv)
{
    moist_top_and_bot(mp<TF>(thl0), mp<TF>(qt0), cp<TF>(g->z), cp<TF>(g->zh), cp<TF>(g->dzhi), g->kstart, g->kend);
    const int n = moist_base_state(mp<TF>(pref), mp<TF>(prefh), mp<TF>(rhoref), mp<TF>(rhorefh), mp<TF>(thvref), mp<TF>(thvrefh), mp<TF>(exnref), mp<TF>(exnrefh),
                                   cp<TF>(thl0), cp<TF>(qt0), TF(pbot), g->kstart, g->kend, cp<TF>(g->z), cp<TF>(g->dz), cp<TF>(g->dzh));
    if (nonconv) *nonconv += n;
    if (boussinesq)             // :1229-1241
        for (int k=0; k<g->kcells; ++k)
        {
            moist_put(mp<TF>(rhoref), k, TF(1.)); moist_put(mp<TF>(rhorefh), k, TF(1.));
            moist_put(mp<TF>(thvref), k, TF(thvref0)); moist_put(mp<TF>(thvrefh), k, TF(thvref0));
        }
    return MHH_OK;
}
MHH_API int mhh_thermo_moist_base_state_host(const mhh_grid* g_host, void* thl0, void* qt0, double pbot, int boussinesq, double thvref0,
                                             void* pref, void* prefh, void* rhoref, void* rhorefh, void* thvref, void* thvrefh,
                                             void* exnref, void* exnrefh, int* nonconv)
{
    const mhh_grid* g = g_host;
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(thl0 && qt0, "null profile");
    MHH_REQUIRE(g->z && g->zh && g->dz && g->dzh && g->dzhi, "the grid's metric arrays (host pointers here)");
    MHH_REQUIRE(g->kgc >= 1 && g->kmax >= 2, "one vertical ghost cell, two levels");
#define CALL(TF) moist_base_state_host<TF>(g, thl0, qt0, pbot, boussinesq, thvref0, pref, prefh, rhoref, rhorefh, thvref, thvrefh, exnref, exnrefh, nonconv)
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

MHH_API int mhh_thermo_moist_base_state(const mhh_grid* g, const void* thlmean, const void* qtmean, double pbot,
                                        void* pref, void* prefh, void* rhoref, void* rhorefh, void* thvref, void* thvrefh,
                                        void* exnref, void* exnrefh, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(thlmean && qtmean, "null profile");
    MHH_REQUIRE(g->z && g->dz && g->dzh, "the grid's metric arrays");
    MHH_REQUIRE(g->kgc >= 1, "one vertical ghost cell");
#define CALL(TF) [&]{ const MoistBaseArgs<TF> A{mp<TF>(pref), mp<TF>(prefh), mp<TF>(rhoref), mp<TF>(rhorefh), mp<TF>(thvref), mp<TF>(thvrefh), mp<TF>(exnref), mp<TF>(exnrefh), \
                                                cp<TF>(thlmean), cp<TF>(qtmean), cp<TF>(g->z), cp<TF>(g->dz), cp<TF>(g->dzh), nonconv, TF(pbot), g->kstart, g->kend}; \
                      hipLaunchKernelGGL(moist_base_state_kernel<TF>, dim3(1), dim3(1), 0, as_stream(stream), A); \
                      MHH_LAUNCH_CHECK(); return (int)MHH_OK; }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
