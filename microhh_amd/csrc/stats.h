// stats.h -- the sampling of Stats<TF> for second-order cases (src/stats.cxx): the mask words, the masked per-level sums in two
// passes, the column pass of cover and path, and the finish kernels that turn sums and counts into profiles and time series.
// Kernels and C-ABI entry points; included from k_stencil.hip. The masked sums are reduced as level_reduce.h says, with
// block_sums as the block's order: no floating-point atomics anywhere, the same bits on every run.
#pragma once
#include "level_reduce.h"
#include <gfx950_prims.h>

namespace mhh
{
constexpr int SNM = MHH_STATS_MAX_MASKS;
constexpr int SNJ = MHH_STATS_MAX_JOBS;
static_assert(SNJ <= LEVEL_MAX_RANGES, "a level range per job");

template<class TF> __host__ __device__ inline TF stats_fill();      // netcdf_fp_fillvalue (src/stats.cxx:51-53): NC_FILL_DOUBLE / NC_FILL_FLOAT
template<> __host__ __device__ inline double stats_fill<double>() { return 9.9692099683868690e+36; }
template<> __host__ __device__ inline float  stats_fill<float>()  { return 9.9692099683868690e+36f; }

// =======================================================================================================
// initialize_masks (:1214-1227): every word, ghosts included, is the sum of all flags
// =======================================================================================================
__global__ void __launch_bounds__(256) stats_mask_init_kernel(unsigned int* __restrict__ m, long long n, unsigned int flagmax)
{
    const long long c = (long long)blockIdx.x*256 + threadIdx.x;
    if (c < n) m[c] = flagmax;
}

// =======================================================================================================
// calc_mask_thres (:95-172), all six loops in one launch over the interior columns and ALL levels. A level takes its full-level
// test from itself, from kstart below the domain and from kend-1 at and above kend; its half-level test from itself up to and
// including kend, from kstart below and from kend above. Level 0 also does mfield_bot. Integer logic: a set bit whose test fails
// is cleared, which is what `m -= (m & flag) * is_false` leaves; NaN fails neither test.
// =======================================================================================================
template<class TF, int MODE> __device__ __forceinline__ bool stats_is_false(TF v, TF t) { return MODE == MHH_STATS_MASK_PLUS ? (v <= t) : (v > t); }

template<class TF, int MODE> struct StatsThresOp
{
    unsigned int* mfield; unsigned int* mfield_bot;
    const TF* fld; const TF* fldh; const TF* fld_bot;
    TF thres; unsigned int flag, flagh; int kstart, kend, jj, kk;
    __device__ void operator()(int i, int j, int k, int ijk) const
    {
        const int ij = i + j*jj;
        const int kf = k < kstart ? kstart : (k >= kend ? kend-1 : k);
        const int kh = k < kstart ? kstart : (k >  kend ? kend   : k);
        unsigned int m = mfield[ijk];
        if (stats_is_false<TF, MODE>(fld [ij + kf*kk], thres)) m &= ~flag;
        if (stats_is_false<TF, MODE>(fldh[ij + kh*kk], thres)) m &= ~flagh;
        mfield[ijk] = m;
        if (k == 0 && stats_is_false<TF, MODE>(fld_bot[ij], thres)) mfield_bot[ij] &= ~flag;
    }
};

// =======================================================================================================
// Grid::interpolate_2nd(wf, w, wloc, sloc) (src/grid.cxx:455-486), what Fields::get_mask (src/fields.cxx:631-643) makes for the
// wplus and wmin masks: the eight-term expression with iih = jjh = 0 and kkh = +kk, its literals doubles as there (so the sum runs
// in double whatever TF is and is narrowed once), over the levels 0 .. kcells-2 of the interior columns.
// =======================================================================================================
template<class TF> struct StatsInterpWOp
{
    TF* out; const TF* in; int kk;
    __device__ void operator()(int, int, int, int c) const
    {
        out[c] = 0.25*(0.5*in[c   ] + 0.5*in[c   ]) + 0.25*(0.5*in[c   ] + 0.5*in[c   ])
               + 0.25*(0.5*in[c+kk] + 0.5*in[c+kk]) + 0.25*(0.5*in[c+kk] + 0.5*in[c+kk]);
    }
};

// =======================================================================================================
// The masked sums. A job is one variable and one operation. The term of a cell is what the reference's
// loop adds before the product with in_mask<double>:
//   MEAN     calc_mean (:263-287), also the mean of w under flagh, calc_tend (:1893-1919)      double(fld)
//   MOMENTp  calc_moment (:341-365)      pow(fld - mean[k] + offset, p): the argument in TF, the power in double
//   FRAC     calc_frac (:410-433)        (fld + offset) > threshold
//   GRAD     calc_grad_2nd (:2171-2195)  (fld[k] - fld[k-1]) * dzhi[k], under the flag of the OTHER level
//   COUNT    calc_nmask (:224-261)       1
//   MEAN2D   calc_mean_2d (:289-306)     double(fld[ij]), no mask, one "level"
// Masks are spread over NM accumulators per thread and job (NM = 1, 2, 4, 8: the next power of two at or above nmasks, bits of
// masks that do not exist are never set); up to SGJ consecutive jobs of one variable share a block and one read of the variable.
// =======================================================================================================
template<class TF> struct StatsJob
{
    const TF* fld; const TF* mean;             // the variable; moments: its finished mean profiles [nmasks][kcells]
    TF offset, threshold;
    int op, half, k0, nk;                      // half: the flag the sum runs under (1 = flagh); levels k0 .. k0+nk-1
};
constexpr int SGJ = 4;                         // jobs of one variable that one block serves with one read of it
template<class TF> struct StatsFlux            // what a flux job takes beyond StatsJob
{
    const TF* w; const TF* wmean; const TF* evisc; const TF* flux_bot; const TF* flux_top;
    TF visc, tPr;
    int kind, scheme, limit, sm, a, b;
};
template<class TF> struct StatsArgs
{
    StatsJob<TF> job[SNJ];
    StatsFlux<TF> flux[SNJ];
    TF dxi, dyi; int kstart, kend;
    unsigned char gjob[SNJ][SGJ]; unsigned char gn[SNJ];     // the groups: consecutive jobs of the same variable and level range
    const unsigned int* mfield; const TF* dzhi;
    LevelDomain dom;
    int nmasks, ngroups, kcells;
};

// blockIdx.y is a GROUP of up to SGJ jobs of one variable: the variable, the level below it (where a gradient is among them) and
// the mask word are read once per cell and serve every job of the group. SGJ x NM double accumulators per thread, indexed
// statically (the loops over slots and masks are unrolled): registers, no scratch. part[job][mask][kcells][nchunks].
template<class TF, int NM>
__global__ void __launch_bounds__(LEVEL_THREADS) stats_partial_kernel(const StatsArgs<TF> A, const Tiling t, double* __restrict__ part, int nchunks)
{
    const int ng = A.gn[blockIdx.y];
    const StatsJob<TF>& J0 = A.job[A.gjob[blockIdx.y][0]];        // the variable and the level range are the group's
    LevelTile T;
    if (!level_tile(t, blockIdx.x, J0.k0, A.dom, T)) return;
    if (T.kz >= J0.nk || J0.op >= MHH_STATS_FLUX_W) return;       // a flux job is a group of its own, served by stats_flux_kernel
    const int k = T.k, kk = A.dom.ijcells;
    const bool flat = (J0.op == MHH_STATS_MEAN2D), ones = (J0.op == MHH_STATS_COUNT);
    const TF* __restrict__ fld = J0.fld + (flat ? (size_t)0 : (size_t)k*kk);
    const unsigned int* __restrict__ msk = A.mfield + (size_t)k*kk;
    const double dzhik = A.dzhi ? double(uniform_load(A.dzhi, k)) : 0.;
    int op[SGJ], sh[SGJ];
    TF offset[SGJ], thres[SGJ], mean[SGJ][NM];
    double acc[SGJ][NM];
    bool grad = false;
#pragma unroll
    for (int s=0; s<SGJ; ++s)
    {
        const StatsJob<TF>& J = A.job[A.gjob[blockIdx.y][s < ng ? s : 0]];
        op[s] = (s < ng) ? J.op : -1; sh[s] = J.half; offset[s] = J.offset; thres[s] = J.threshold;
        grad = grad || op[s] == MHH_STATS_GRAD;
        const bool moment = (op[s] >= MHH_STATS_MOMENT2 && op[s] <= MHH_STATS_MOMENT4);
#pragma unroll
        for (int n=0; n<NM; ++n)
        {
            acc[s][n] = 0.;
            mean[s][n] = (moment && n < A.nmasks) ? uniform_load(J.mean, n*A.kcells + k) : TF(0);
        }
    }
    for_chunk_cells(A.dom, T.j0, T.j1, [&](int, int, int ij) __attribute__((always_inline))
    {
        const unsigned int m = flat ? 0xffffffffu : msk[ij];
        const TF v = ones ? TF(1) : fld[ij];
        const TF below = grad ? fld[ij - kk] : TF(0);
#pragma unroll
        for (int s=0; s<SGJ; ++s)
        {
            if (op[s] < 0) continue;
            if (op[s] >= MHH_STATS_MOMENT2 && op[s] <= MHH_STATS_MOMENT4)
            {
#pragma unroll
                for (int n=0; n<NM; ++n)
                {
                    const double x = double(TF(TF(v - mean[s][n]) + offset[s]));
                    const double x2 = x*x;
                    const double p = (op[s] == MHH_STATS_MOMENT2) ? x2 : (op[s] == MHH_STATS_MOMENT3) ? x2*x : x2*x2;
                    acc[s][n] += double((m >> (2*n + sh[s])) & 1u) * p;
                }
            }
            else
            {
                const bool g = (op[s] == MHH_STATS_GRAD);
                double term;
                if (op[s] == MHH_STATS_FRAC) term = (TF(v + offset[s]) > thres[s]) ? 1. : 0.;
                else if (g)                  term = double(TF(v - below));
                else                         term = double(v);
#pragma unroll
                for (int n=0; n<NM; ++n)
                {
                    const double q = double((m >> (2*n + sh[s])) & 1u) * term;
                    acc[s][n] += g ? q*dzhik : q;                             // in_mask * (d[k] - d[k-1]) * dzhi[k], left to right
                }
            }
        }
    });
    const int tid = threadIdx.x + threadIdx.y*BX;
#pragma unroll
    for (int s=0; s<SGJ; ++s)
    {
        if (s >= ng) break;                                        // block-uniform: every thread takes the same barriers
        const double sum = block_sums<NM>(acc[s]);
        if (tid < NM && tid < A.nmasks) part[(((size_t)A.gjob[blockIdx.y][s]*A.nmasks + tid)*A.kcells + k)*nchunks + T.by] = sum;
    }
}


// =======================================================================================================
// The fluxes. blockIdx.y is a job; jobs that are no flux leave at once.
// FLUX_W: the reference writes fld' = fld - mean[k] and w' = w - wmean[k] into two tmp fields (subtract_mean, :514-535: fld' on
// kstart .. kend-1, w' on kstart .. kend) and calls advec.get_advec_flux on them; here the same expressions are evaluated on the
// fly from fld, w and the two profiles, per mask, because the means are the mask's. A level of fld' outside kstart .. kend-1 (which
// advec_2 alone reads, at the two walls, against w' = 0 there) counts as zero: the tmp field of a first sample.
//   advec_2    (src/advec_2.cxx:206-252):   W * interp2(s'[k-1], s'[k]) on kstart .. kend
//   advec_2i5  (src/advec_2i5.cxx:730-913): zero on both walls; interp2 at kstart+1 and kend-1; interp4_ws / interp3_ws at kstart+2
//              and kend-2; interp6_ws / interp5_ws in between -- the five near-wall bodies and the interior
//   limited    (include/advec_monotonic.h:183-235): zero on both walls, flux_lim_bot at kstart+1, flux_lim_top at kend-1, flux_lim between
// with W = w' for a scalar, interp2(w'[i-1], w'[i]) for u, interp2(w'[j-1], w'[j]) for v.
// FLUX_DIFF: Diff_2::diff_flux (src/diff_2.cxx:88-105); Diff_smag2::diff_flux (src/diff_smag2.cxx:739-842, :1217-1276) with the wall
// included, or with flux_bot / flux_top on kstart and kend and the interior from kstart+1. The eddy viscosity at the face is formed
// with the reference's double literals (0.5 *, 0.25 *) and narrowed once, as `const TF eviscc = ...` does.
// =======================================================================================================
template<class TF, int NM>
__global__ void __launch_bounds__(LEVEL_THREADS) stats_flux_kernel(const StatsArgs<TF> A, const Tiling t, double* __restrict__ part, int nchunks)
{
    const StatsJob<TF>& J = A.job[blockIdx.y];
    const StatsFlux<TF>& F = A.flux[blockIdx.y];
    LevelTile T;
    if (!level_tile(t, blockIdx.x, J.k0, A.dom, T)) return;
    if ((J.op != MHH_STATS_FLUX_W && J.op != MHH_STATS_FLUX_DIFF) || T.kz >= J.nk) return;
    const int k = T.k, kk = A.dom.ijcells, jj = A.dom.icells, ks = A.kstart, ke = A.kend;
    const bool resolved = (J.op == MHH_STATS_FLUX_W);
    const int hoff = (F.kind == 1) ? 1 : (F.kind == 2 ? jj : 0);   // the neighbour of u or v that shares the face
    const unsigned int* __restrict__ msk = A.mfield + (size_t)k*kk;
    const TF dzhik = uniform_load(A.dzhi, k);
    // the body of this level: 0 zero flux, 2 second order, 4 fourth / third, 6 sixth / fifth; limited: 1 bottom, 3 top, 5 interior
    int body = 2;
    if (resolved && F.limit)                  body = (k == ks || k == ke) ? 0 : (k == ks+1 ? 1 : (k == ke-1 ? 3 : 5));
    else if (resolved && F.scheme == MHH_ADVEC_2I5)
        body = (k == ks || k == ke) ? 0 : ((k == ks+1 || k == ke-1) ? 2 : ((k == ks+2 || k == ke-2) ? 4 : 6));
    TF mean[NM][6], wm[NM];
    double acc[NM];
#pragma unroll
    for (int n=0; n<NM; ++n)
    {
        acc[n] = 0.;
        wm[n] = (resolved && n < A.nmasks) ? uniform_load(F.wmean, n*A.kcells + k) : TF(0);
#pragma unroll
        for (int d=0; d<6; ++d)
        {
            const int kl = k - 3 + d;
            mean[n][d] = (resolved && n < A.nmasks && kl >= ks && kl < ke) ? uniform_load(J.mean, n*A.kcells + kl) : TF(0);
        }
    }
    for_chunk_cells(A.dom, T.j0, T.j1, [&](int, int, int ij) __attribute__((always_inline))
    {
        const unsigned int m = msk[ij];
        if (resolved)
        {
            TF sv[6];
#pragma unroll
            for (int d=0; d<6; ++d)
            {
                const int kl = k - 3 + d;
                sv[d] = (body != 0 && kl >= ks && kl < ke) ? J.fld[ij + (size_t)kl*kk] : TF(0);
            }
            const TF w0 = F.w[ij + (size_t)k*kk];
            const TF w1 = hoff ? F.w[ij - hoff + (size_t)k*kk] : TF(0);
#pragma unroll
            for (int n=0; n<NM; ++n)
            {
                TF sp[6];
#pragma unroll
                for (int d=0; d<6; ++d)
                {
                    const int kl = k - 3 + d;
                    sp[d] = (kl >= ks && kl < ke) ? TF(sv[d] - mean[n][d]) : TF(0);
                }
                const TF W = hoff ? i2(TF(w1 - wm[n]), TF(w0 - wm[n])) : TF(w0 - wm[n]);
                TF f;
                if (body == 0)      f = TF(0);
                else if (body == 2) f = W * i2(sp[2], sp[3]);
                else if (body == 4) f = W * i4ws(sp[1], sp[2], sp[3], sp[4]) - tabs(W) * i3ws(sp[1], sp[2], sp[3], sp[4]);
                else if (body == 6) f = W * i6(sp[0], sp[1], sp[2], sp[3], sp[4], sp[5]) - tabs(W) * i5(sp[0], sp[1], sp[2], sp[3], sp[4], sp[5]);
                else                f = koren_flux(body == 1 ? 1 : (body == 3 ? 2 : 0), W, sp[1], sp[2], sp[3], sp[4]);
                acc[n] += double((m >> (2*n + 1)) & 1u) * double(f);
            }
        }
        else
        {
            const size_t c = ij + (size_t)k*kk;
            TF f;
            if (F.scheme == MHH_DIFF_2) f = - F.visc*(J.fld[c] - J.fld[c-kk])*dzhik;
            else if (F.sm && k == ks)   f = F.flux_bot[ij];
            else if (F.sm && k == ke)   f = F.flux_top[ij];
            else if (F.kind == 0)
            {
                const TF eviscc = 0.5*(F.evisc[c-kk]+F.evisc[c])/F.tPr + F.visc;
                f = - eviscc*(J.fld[c] - J.fld[c-kk])*dzhik;
            }
            else
            {
                const TF evisch = 0.25*(F.evisc[c-hoff-kk]+F.evisc[c-hoff]+F.evisc[c-kk]+F.evisc[c]) + F.visc;
                f = - evisch*( (J.fld[c]-J.fld[c-kk])*dzhik + (F.w[c]-F.w[c-hoff])*(F.kind == 1 ? A.dxi : A.dyi) );
            }
#pragma unroll
            for (int n=0; n<NM; ++n) acc[n] += double((m >> (2*n + 1)) & 1u) * double(f);
        }
    });
    const int tid = threadIdx.x + threadIdx.y*BX;
    const double sum = block_sums<NM>(acc);
    if (tid < NM && tid < A.nmasks) part[(((size_t)blockIdx.y*A.nmasks + tid)*A.kcells + k)*nchunks + T.by] = sum;
}

// prof[k] = tmp / nmask[k] (double by int, narrowed to TF), the offset added to a mean on EVERY level (:1635), the fill value where
// nmask[k] == 0 over ALL levels (set_fillvalue_prof, :85-93); levels outside kstart .. kend of a counted level hold 0, a mean's its
// offset: a profile that starts from zero, as a first sample's does.
// MEAN2D: out[0] = tmp / (itot*jtot) + offset (:305, :1934).
template<class TF>
__global__ void __launch_bounds__(256) stats_finish_kernel(const StatsArgs<TF> A, const double* __restrict__ sums, const int* __restrict__ nmask,
                                                           TF* __restrict__ out, int ijtot)
{
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= A.kcells) return;
    const int job = blockIdx.y / A.nmasks, n = blockIdx.y % A.nmasks;
    const StatsJob<TF>& J = A.job[job];
    const size_t o = ((size_t)job*A.nmasks + n)*A.kcells + k;
    if (J.op == MHH_STATS_MEAN2D)
    {
        out[o] = (k == 0) ? TF(TF(sums[o] / ijtot) + J.offset) : TF(0);
        return;
    }
    const int cnt = nmask[(n*2 + J.half)*A.kcells + k];
    TF v = TF(0);
    if (J.op == MHH_STATS_FLUX_SUM)                               // add_fluxes (:400-407): flux[k] = turb[k] + diff[k], both finished
    {
        const StatsFlux<TF>& F = A.flux[job];
        if (k >= J.k0 && k < J.k0 + J.nk && cnt != 0)
            v = TF(sums[((size_t)F.a*A.nmasks + n)*A.kcells + k] / cnt) + TF(sums[((size_t)F.b*A.nmasks + n)*A.kcells + k] / cnt);
    }
    else if (k >= J.k0 && k < J.k0 + J.nk && cnt != 0) v = TF(sums[o] / cnt);
    if (J.op == MHH_STATS_MEAN) v += J.offset;                    // every level, as `for (auto& value : ...) value += offset` (:1635)
    if (cnt == 0) v = stats_fill<TF>();
    out[o] = v;
}

// finalize_masks after the counts (:1241-1260): the integer counts, nmask_bot = nmaskh[kstart], area and areah (calc_area,
// :209-221, over kstart .. kend + loc). csums is the COUNT pass: [2][nmasks][kcells], full then half.
template<class TF>
__global__ void __launch_bounds__(256) stats_mask_finish_kernel(const double* __restrict__ csums, int nmasks, int kcells, int kstart, int kend, int ijtot,
                                                                int* __restrict__ nmask, int* __restrict__ nmask_bot, TF* __restrict__ area, TF* __restrict__ areah)
{
    const int k = blockIdx.x*256 + threadIdx.x;
    const int n = blockIdx.y;
    if (k >= kcells) return;
    const int c  = (int)csums[((size_t)0*nmasks + n)*kcells + k];
    const int ch = (int)csums[((size_t)1*nmasks + n)*kcells + k];
    nmask[(n*2 + 0)*kcells + k] = c;
    nmask[(n*2 + 1)*kcells + k] = ch;
    if (k == kstart) nmask_bot[n] = ch;
    area [n*kcells + k] = (k >= kstart && k < kend   && c ) ? TF(c )/TF(ijtot) : TF(0);
    areah[n*kcells + k] = (k >= kstart && k < kend+1 && ch) ? TF(ch)/TF(ijtot) : TF(0);
}

// =======================================================================================================
// The column pass: calc_cover (:475-507) and calc_path (:435-473), one thread per column marching k, all masks at once.
// cover counts the columns with a masked cell above the threshold, nmaskcover those with any masked cell (a column that is
// covered has one). calc_path's nmask_proj is a running count, so its `nmask_proj > 0` lets every column at or after the first
// non-empty one in; but what a column adds is its MASKED cells alone, so the columns let in early or late add nothing and the
// running count ends as the number of non-empty columns: path = the sum over masked cells, nmask_proj = nmaskcover. A column's
// sum runs serially in TF as `data*rho*dz`; columns are added in double, a block's by block_sums (level_reduce.h), the blocks in index order.
// part[block][mask][3] = cover, nmaskcover, path.
// =======================================================================================================
template<class TF> struct StatsColArgs
{
    const unsigned int* mfield; const TF* fld; const TF* rho; const TF* dz;
    TF offset, threshold;
    LevelDomain dom;
    int nmasks, half, kstart, kend, nbx;
};
template<class TF, int NM>
__global__ void __launch_bounds__(LEVEL_THREADS) stats_column_kernel(const StatsColArgs<TF> A, double* __restrict__ part)
{
    const int bx = blockIdx.x % A.nbx, by = blockIdx.x / A.nbx;
    const int i = A.dom.istart + bx*BX + (int)threadIdx.x, j = A.dom.jstart + by*BY + (int)threadIdx.y;
    const bool live = (i < A.dom.iend && j < A.dom.jend);
    unsigned int has = 0, cov = 0;
    TF path[NM];
#pragma unroll
    for (int n=0; n<NM; ++n) path[n] = TF(0);
    if (live)
    {
        const int ij = i + j*A.dom.icells;
        for (int k=A.kstart; k<A.kend; ++k)
        {
            const unsigned int m = A.mfield[ij + (size_t)k*A.dom.ijcells];
            const TF v = A.fld[ij + (size_t)k*A.dom.ijcells];
            const TF t = v*uniform_load(A.rho, k)*uniform_load(A.dz, k);
            const bool above = TF(v + A.offset) > A.threshold;
#pragma unroll
            for (int n=0; n<NM; ++n)
            {
                const bool in = (m >> (2*n + A.half)) & 1u;
                if (in) { has |= 1u << n; path[n] += t; if (above) cov |= 1u << n; }
            }
        }
    }
    const int tid = threadIdx.x + threadIdx.y*BX;
    double vc[NM], vh[NM], vp[NM];
#pragma unroll
    for (int n=0; n<NM; ++n) { vc[n] = double((cov >> n) & 1u); vh[n] = double((has >> n) & 1u); vp[n] = double(path[n]); }
    const double c = block_sums<NM>(vc);
    const double h = block_sums<NM>(vh);
    const double p = block_sums<NM>(vp);
    if (tid < NM && tid < A.nmasks)
    {
        double* q = part + ((size_t)blockIdx.x*A.nmasks + tid)*3;
        q[0] = c; q[1] = h; q[2] = p;
    }
}
// sums[mask][3]: the blocks in index order
__global__ void __launch_bounds__(64) stats_column_sums_kernel(const double* __restrict__ part, double* __restrict__ sums, int nblocks, int nmasks)
{
    const int e = threadIdx.x;
    if (e >= nmasks*3) return;
    double tmp = 0.;
    for (int b=0; b<nblocks; ++b) tmp += part[(size_t)b*nmasks*3 + e];
    sums[e] = tmp;
}
// out[mask][2]: cover = TF(cover)/TF(nmaskcover), 0 with no column (:1863); path = path / nmask_proj, TF by int, NaN with no
// column as in the reference (:1837)
template<class TF>
__global__ void __launch_bounds__(64) stats_column_finish_kernel(const double* __restrict__ sums, TF* __restrict__ out, int nmasks)
{
    const int n = threadIdx.x;
    if (n >= nmasks) return;
    const int cover = (int)sums[n*3], ncol = (int)sums[n*3 + 1];
    out[n*2]     = (ncol > 0) ? TF(cover)/TF(ncol) : TF(0);
    out[n*2 + 1] = TF(sums[n*3 + 2]) / TF(ncol);
}

// ---- host side ---------------------------------------------------------------------------------------------
inline int stats_col_blocks(const mhh_grid* g) { return ((g->imax + BX-1)/BX) * ((g->jmax + BY-1)/BY); }

static int stats_check(const mhh_grid* g, int nmasks)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(nmasks >= 1 && nmasks <= SNM, "1 .. MHH_STATS_MAX_MASKS masks");
    MHH_REQUIRE(g->kgc >= 1, "the profiles read level kend and level kstart-1: one vertical ghost level");
    return MHH_OK;
}

template<class TF>
static int stats_fill_args(const mhh_grid* g, const void* mfield, int nmasks, const mhh_stats_job* jobs, int njobs, StatsArgs<TF>& A, int& nkmax)
{
    A = StatsArgs<TF>{};
    A.mfield = static_cast<const unsigned int*>(mfield); A.dzhi = cp<TF>(g->dzhi);
    A.nmasks = nmasks; A.dom = level_domain(g); A.kcells = g->kcells;
    { const GridDev<TF> gd = make_grid<TF>(g); A.dxi = gd.dxi_d; A.dyi = gd.dyi_d; }
    A.kstart = g->kstart; A.kend = g->kend;
    nkmax = 1;
    for (int n=0; n<njobs; ++n)
    {
        const mhh_stats_job& j = jobs[n];
        StatsJob<TF>& J = A.job[n];
        MHH_REQUIRE(j.loc == 0 || j.loc == 1, "loc: 0 full level, 1 half level");
        MHH_REQUIRE(j.op == MHH_STATS_COUNT || j.fld != nullptr, "null field");
        J.fld = cp<TF>(j.fld); J.mean = cp<TF>(j.mean); J.offset = TF(j.offset); J.threshold = TF(j.threshold); J.op = j.op;
        J.half = j.loc; J.k0 = g->kstart; J.nk = g->kmax + 1;                  // kstart .. kend inclusive (:271)
        switch (j.op)
        {
            case MHH_STATS_MEAN: case MHH_STATS_FRAC: break;
            case MHH_STATS_MOMENT2: case MHH_STATS_MOMENT3: case MHH_STATS_MOMENT4:
                MHH_REQUIRE(j.mean != nullptr, "a moment needs the finished mean profiles of its variable"); break;
            case MHH_STATS_GRAD: J.half = !j.loc; MHH_REQUIRE(g->dzhi != nullptr, "dzhi"); break;       // !fld.loc[2] (:1787)
            case MHH_STATS_COUNT: J.k0 = 0; J.nk = g->kcells; break;                                      // 0 .. kcells (:1244)
            case MHH_STATS_MEAN2D: J.k0 = 0; J.nk = 1; break;
            case MHH_STATS_FLUX_W: case MHH_STATS_FLUX_DIFF: case MHH_STATS_FLUX_SUM:
            {
                StatsFlux<TF>& F = A.flux[n];
                if (j.loc != 0) { set_error("mhh_stats: the flux of a half-level variable (w itself) cannot be delivered at that location"); return MHH_EINVAL; }
                J.half = 1;                                          // !fld.loc[2] (:1715, :1744, :1769)
                F.w = cp<TF>(j.w); F.wmean = cp<TF>(j.wmean); F.evisc = cp<TF>(j.evisc); F.flux_bot = cp<TF>(j.flux_bot); F.flux_top = cp<TF>(j.flux_top);
                F.visc = TF(j.visc); F.tPr = TF(j.tPr); F.kind = j.kind; F.scheme = j.scheme; F.limit = j.limit; F.sm = j.surface_model; F.a = j.a; F.b = j.b;
                MHH_REQUIRE(j.kind >= 0 && j.kind <= 2, "kind: 0 scalar, 1 u, 2 v");
                if (j.op == MHH_STATS_FLUX_W)
                {
                    if (j.scheme != MHH_ADVEC_2 && j.scheme != MHH_ADVEC_2I5)
                    { set_error("mhh_stats: the resolved flux of advection scheme %d is not built (2 and 2i5 are)", j.scheme); return MHH_EINVAL; }
                    MHH_REQUIRE(j.mean && j.w && j.wmean, "the resolved flux needs the finished means of the variable, w and the mean of w under flagh");
                    MHH_REQUIRE(!j.limit || (j.kind == 0 && j.scheme == MHH_ADVEC_2I5), "advec_flux_s_lim is a scalar's, with advec_2i5");
                    MHH_REQUIRE(j.scheme == MHH_ADVEC_2 || g->kmax >= 6, "advec_2i5's flux has five near-wall bodies: at least 6 levels");
                    MHH_REQUIRE(j.kind == 0 || (g->igc >= 1 && g->jgc >= 1), "ghost cells");
                }
                else if (j.op == MHH_STATS_FLUX_DIFF)
                {
                    if (j.scheme != MHH_DIFF_2 && j.scheme != MHH_DIFF_SMAG2)
                    { set_error("mhh_stats: the diffusive flux of diffusion scheme %d is not built (2 and smag2 are)", j.scheme); return MHH_EINVAL; }
                    if (j.scheme == MHH_DIFF_SMAG2)
                    {
                        MHH_REQUIRE(j.evisc != nullptr && (j.kind == 0 || j.w != nullptr), "smag2 needs evisc, and w for u and v");
                        MHH_REQUIRE(!j.surface_model || (j.flux_bot && j.flux_top), "a surface model needs flux_bot and flux_top");
                    }
                }
                else
                    MHH_REQUIRE(j.a >= 0 && j.a < njobs && j.b >= 0 && j.b < njobs && jobs[j.a].op == MHH_STATS_FLUX_W && jobs[j.b].op == MHH_STATS_FLUX_DIFF,
                                "_flux adds the _w and the _diff job of the same call");
                break;
            }
            default:
                set_error("mhh_stats: unknown operation %d (covariances, budgets and the 4th-order gradient are not built)", j.op);
                return MHH_EINVAL;
        }
        if (J.nk > nkmax) nkmax = J.nk;
        // a job joins the group of the job before it where the variable and the levels are the same
        const int gr = A.ngroups - 1;
        if (n > 0 && A.gn[gr] < SGJ && J.op != MHH_STATS_COUNT && J.op != MHH_STATS_MEAN2D && J.op < MHH_STATS_FLUX_W && A.job[n-1].op < MHH_STATS_FLUX_W && A.job[n-1].fld == J.fld && A.job[n-1].k0 == J.k0 &&
            A.job[n-1].nk == J.nk && A.job[n-1].op != MHH_STATS_MEAN2D)
            A.gjob[gr][A.gn[gr]++] = (unsigned char)n;
        else { A.gjob[A.ngroups][0] = (unsigned char)n; A.gn[A.ngroups++] = 1; }
    }
    return MHH_OK;
}

template<class TF>
static int stats_sums_launch(const mhh_grid* g, const void* mfield, int nmasks, const mhh_stats_job* jobs, int njobs, double* sums, double* scratch, hipStream_t st)
{
    StatsArgs<TF> A; int nkmax;
    if (int e = stats_fill_args<TF>(g, mfield, nmasks, jobs, njobs, A, nkmax)) return e;
    const int nchunks = level_chunks(g);
    const Tiling t = level_tiling(g, nkmax);
    const dim3 grid(tiling_blocks(t), A.ngroups), block(BX, BY, 1);
    with_mask_width(nmasks, [&](auto nm) { hipLaunchKernelGGL((stats_partial_kernel<TF, decltype(nm)::value>), grid, block, 0, st, A, t, scratch, nchunks); });
    MHH_LAUNCH_CHECK();
    bool any_flux = false;
    for (int n=0; n<njobs; ++n) any_flux = any_flux || jobs[n].op == MHH_STATS_FLUX_W || jobs[n].op == MHH_STATS_FLUX_DIFF;
    if (any_flux)
    {
        const dim3 fgrid(tiling_blocks(t), njobs);
        with_mask_width(nmasks, [&](auto nm) { hipLaunchKernelGGL((stats_flux_kernel<TF, decltype(nm)::value>), fgrid, block, 0, st, A, t, scratch, nchunks); });
        MHH_LAUNCH_CHECK();
    }
    LevelRanges R{nmasks};                                         // the masks of a job share its levels
    for (int n=0; n<njobs; ++n) { R.k0[n] = A.job[n].k0; R.nk[n] = A.job[n].nk; }
    return level_sums_launch(g, scratch, sums, njobs*nmasks, R, st);
}

template<class TF>
static int stats_finish_launch(const mhh_grid* g, int nmasks, const mhh_stats_job* jobs, int njobs, const double* sums, const int* nmask, void* out, hipStream_t st)
{
    StatsArgs<TF> A; int nkmax;
    if (int e = stats_fill_args<TF>(g, nullptr, nmasks, jobs, njobs, A, nkmax)) return e;
    hipLaunchKernelGGL(stats_finish_kernel<TF>, dim3((g->kcells + 255)/256, njobs*nmasks), dim3(256), 0, st, A, sums, nmask, mp<TF>(out), g->itot*g->jtot);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

template<class TF>
static int stats_thres_launch(const mhh_grid* g, void* mfield, void* mfield_bot, int mask, const void* fld, const void* fldh, const void* fld_bot,
                              double threshold, int mode, hipStream_t st)
{
    const unsigned int flag = 1u << (2*mask), flagh = 1u << (2*mask + 1);            // add_mask (:841-850)
    if (mode == MHH_STATS_MASK_PLUS)
    {
        const StatsThresOp<TF, MHH_STATS_MASK_PLUS> op{static_cast<unsigned int*>(mfield), static_cast<unsigned int*>(mfield_bot), cp<TF>(fld), cp<TF>(fldh),
                                                       cp<TF>(fld_bot), TF(threshold), flag, flagh, g->kstart, g->kend, g->icells, g->ijcells};
        return launch_cells(st, op, g->istart, g->iend, g->jstart, g->jend, 0, g->kcells, g->icells, g->ijcells);
    }
    const StatsThresOp<TF, MHH_STATS_MASK_MIN> op{static_cast<unsigned int*>(mfield), static_cast<unsigned int*>(mfield_bot), cp<TF>(fld), cp<TF>(fldh),
                                                  cp<TF>(fld_bot), TF(threshold), flag, flagh, g->kstart, g->kend, g->icells, g->ijcells};
    return launch_cells(st, op, g->istart, g->iend, g->jstart, g->jend, 0, g->kcells, g->icells, g->ijcells);
}

template<class TF>
static int stats_columns_launch(const mhh_grid* g, const void* mfield, int nmasks, const void* fld, int loc, double offset, double threshold,
                                const void* rhoref, double* sums, double* scratch, hipStream_t st)
{
    StatsColArgs<TF> A{};
    A.mfield = static_cast<const unsigned int*>(mfield); A.fld = cp<TF>(fld); A.rho = cp<TF>(rhoref); A.dz = cp<TF>(g->dz);
    A.offset = TF(offset); A.threshold = TF(threshold); A.nmasks = nmasks; A.half = loc;
    A.dom = level_domain(g); A.kstart = g->kstart; A.kend = g->kend; A.nbx = (g->imax + BX-1)/BX;
    const int nblocks = stats_col_blocks(g);
    const dim3 grid(nblocks), block(BX, BY, 1);
    with_mask_width(nmasks, [&](auto nm) { hipLaunchKernelGGL((stats_column_kernel<TF, decltype(nm)::value>), grid, block, 0, st, A, scratch); });
    MHH_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_column_sums_kernel, dim3(1), dim3(64), 0, st, scratch, sums, nblocks, nmasks);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

MHH_API int mhh_stats_chunk_rows(void) { return LEVEL_ROWS; }
MHH_API unsigned long long mhh_stats_scratch_elems(const mhh_grid* g, int nmasks, int njobs)
{
    if (!g || nmasks < 1 || njobs < 1) return 0;
    const unsigned long long a = (unsigned long long)njobs * nmasks * g->kcells * level_chunks(g);
    const unsigned long long b = (unsigned long long)stats_col_blocks(g) * nmasks * 3;
    return a > b ? a : b;
}

// Stats::initialize_masks (src/stats.cxx:1214-1227)
MHH_API int mhh_stats_mask_init(const mhh_grid* g, void* mfield, void* mfield_bot, int nmasks, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(mfield && mfield_bot, "null pointer");
    const unsigned int flagmax = (1u << (2*nmasks)) - 1u;         // the sum of flag + flagh of every mask (nmasks <= 8)
    const long long n3 = (long long)g->ijcells * g->kcells, n2 = g->ijcells;
    hipLaunchKernelGGL(stats_mask_init_kernel, dim3((unsigned)((n3 + 255)/256)), dim3(256), 0, as_stream(stream), static_cast<unsigned int*>(mfield), n3, flagmax);
    MHH_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_mask_init_kernel, dim3((unsigned)((n2 + 255)/256)), dim3(256), 0, as_stream(stream), static_cast<unsigned int*>(mfield_bot), n2, flagmax);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// Stats::set_mask_thres / calc_mask_thres (src/stats.cxx:95-172, 1264-1301)
MHH_API int mhh_stats_mask_thres(const mhh_grid* g, void* mfield, void* mfield_bot, int mask, const void* fld, const void* fldh, const void* fld_bot,
                                 double threshold, int mode, void* stream)
{
    if (int e = stats_check(g, 1)) return e;
    MHH_REQUIRE(mask >= 0 && mask < SNM, "Invalid mask name in set_mask_thres()");
    MHH_REQUIRE(mode == MHH_STATS_MASK_PLUS || mode == MHH_STATS_MASK_MIN, "Invalid mask type in set_mask_thres()");
    MHH_REQUIRE(mfield && mfield_bot && fld && fldh && fld_bot, "null pointer");
#define CALL(TF) stats_thres_launch<TF>(g, mfield, mfield_bot, mask, fld, fldh, fld_bot, threshold, mode, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// Stats::finalize_masks, first half (src/stats.cxx:1234-1245): the two cyclic fills and calc_nmask over 0 .. kcells, as double
// sums csums[2][nmasks][kcells] (full, half) that a slab rank adds over the ranks before mhh_stats_mask_finish
MHH_API int mhh_stats_mask_count(const mhh_grid* g, void* mfield, void* mfield_bot, int nmasks, void* csums, void* scratch, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(mfield && mfield_bot && csums && scratch, "null pointer");
    if (int e = mhh_boundary_cyclic_u32(g, mfield, g->npy == 1 ? MHH_EDGE_BOTH : MHH_EDGE_EW, stream)) return e;
    if (g->npy == 1) if (int e = mhh_boundary_cyclic_2d_u32(g, mfield_bot, stream)) return e;
    mhh_stats_job jobs[2] = {};
    jobs[0].op = jobs[1].op = MHH_STATS_COUNT; jobs[1].loc = 1;
#define CALL(TF) stats_sums_launch<TF>(g, mfield, nmasks, jobs, 2, static_cast<double*>(csums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// Stats::finalize_masks, second half (src/stats.cxx:1247-1260): nmask[mask][2][kcells] (int; full, half), nmask_bot[mask] =
// nmaskh[kstart], area and areah [mask][kcells]
MHH_API int mhh_stats_mask_finish(const mhh_grid* g, int nmasks, const void* csums, void* nmask, void* nmask_bot, void* area, void* areah, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(csums && nmask && nmask_bot && area && areah, "null pointer");
    const dim3 grid((g->kcells + 255)/256, nmasks);
    if (g->dtype == MHH_F64) hipLaunchKernelGGL(stats_mask_finish_kernel<double>, grid, dim3(256), 0, as_stream(stream), static_cast<const double*>(csums), nmasks, g->kcells,
                                                g->kstart, g->kend, g->itot*g->jtot, static_cast<int*>(nmask), static_cast<int*>(nmask_bot), mp<double>(area), mp<double>(areah));
    else                     hipLaunchKernelGGL(stats_mask_finish_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const double*>(csums), nmasks, g->kcells,
                                                g->kstart, g->kend, g->itot*g->jtot, static_cast<int*>(nmask), static_cast<int*>(nmask_bot), mp<float>(area), mp<float>(areah));
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// the loops of Stats::calc_stats, calc_tend and calc_stats_2d (src/stats.cxx:1607-1937) as per-level double sums
// sums[job][mask][kcells]; a slab rank adds them over the ranks before mhh_stats_finish
MHH_API int mhh_stats_sums(const mhh_grid* g, const void* mfield, int nmasks, const mhh_stats_job* jobs, int njobs, void* sums, void* scratch, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(njobs >= 1 && njobs <= SNJ, "1 .. MHH_STATS_MAX_JOBS jobs per call");
    MHH_REQUIRE(mfield && jobs && sums && scratch, "null pointer");
#define CALL(TF) stats_sums_launch<TF>(g, mfield, nmasks, jobs, njobs, static_cast<double*>(sums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// sums and counts to profiles out[job][mask][kcells] of the grid's dtype: the division by nmask, the offset of a mean, the fill value
MHH_API int mhh_stats_finish(const mhh_grid* g, int nmasks, const mhh_stats_job* jobs, int njobs, const void* sums, const void* nmask, void* out, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(njobs >= 1 && njobs <= SNJ, "1 .. MHH_STATS_MAX_JOBS jobs per call");
    MHH_REQUIRE(jobs && sums && nmask && out, "null pointer");
#define CALL(TF) stats_finish_launch<TF>(g, nmasks, jobs, njobs, static_cast<const double*>(sums), static_cast<const int*>(nmask), out, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_cover and calc_path (src/stats.cxx:435-507) of one variable: sums[mask][3] = cover, nmaskcover, path as doubles
MHH_API int mhh_stats_columns(const mhh_grid* g, const void* mfield, int nmasks, const void* fld, int loc, double offset, double threshold,
                              const void* rhoref, void* sums, void* scratch, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(loc == 0 || loc == 1, "loc: 0 full level, 1 half level");
    MHH_REQUIRE(mfield && fld && rhoref && g->dz && sums && scratch, "null pointer");
#define CALL(TF) stats_columns_launch<TF>(g, mfield, nmasks, fld, loc, offset, threshold, rhoref, static_cast<double*>(sums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// out[mask][2] = cover, path of the grid's dtype (src/stats.cxx:1837, 1863)
MHH_API int mhh_stats_columns_finish(const mhh_grid* g, int nmasks, const void* sums, void* out, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(sums && out, "null pointer");
    if (g->dtype == MHH_F64) hipLaunchKernelGGL(stats_column_finish_kernel<double>, dim3(1), dim3(64), 0, as_stream(stream), static_cast<const double*>(sums), mp<double>(out), nmasks);
    else                     hipLaunchKernelGGL(stats_column_finish_kernel<float>, dim3(1), dim3(64), 0, as_stream(stream), static_cast<const double*>(sums), mp<float>(out), nmasks);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// Grid::interpolate_2nd of w to the full level for the wplus / wmin masks (src/fields.cxx:631-643, src/grid.cxx:455-486). The
// reference leaves level kcells-1 and the ghost columns of its tmp field as they were; here wf is zeroed first, so that what
// set_mask_thres reads of them (the flux level kend where kgc == 1) is defined: 0 leaves mode Plus and stays in mode Min.
MHH_API int mhh_stats_interpolate_w(const mhh_grid* g, const void* w, void* wf, void* stream)
{
    if (int e = stats_check(g, 1)) return e;
    MHH_REQUIRE(w && wf, "null pointer");
    const size_t bytes = (size_t)g->ijcells * g->kcells * (g->dtype == MHH_F64 ? 8 : 4);
    MHH_HIP_TRY(hipMemsetAsync(wf, 0, bytes, as_stream(stream)));
#define CALL(TF) [&]{ const StatsInterpWOp<TF> op{mp<TF>(wf), cp<TF>(w), g->ijcells}; \
                      return launch_cells(as_stream(stream), op, g->istart, g->iend, g->jstart, g->jend, 0, g->kcells-1, g->icells, g->ijcells); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
