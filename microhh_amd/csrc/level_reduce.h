// level_reduce.h -- how a level is reduced, and nothing about what is summed: the deterministic two-stage reduction under the
// horizontal means (force_means.h), the masked sums of Stats (stats.h) and of Budget_2 (budget_2.h).
// A block of BX x BY threads owns one level and a chunk of LEVEL_ROWS rows. Thread (ty, tx) adds the cells j = j0 + ty step BY,
// i = istart + tx step BX, in that order, into doubles. The block adds its 256 accumulators through LDS in one of two fixed orders
// (block_tree_sum for the means, block_sums for the masked sums) and writes ONE partial per sum. A second kernel adds the chunks of
// a level in index order. No floating-point atomics: the same bits on every run; tests/test_reduction_order.py restates both orders
// and compares bits. A kernel adds the per-level uniforms it loads, the term of a cell, its accumulator and where the partial goes.
#pragma once
#include "k_common.h"
#include <type_traits>

namespace mhh
{
constexpr int LEVEL_ROWS = 32;                 // rows of a chunk: mhh_field_mean_chunk_rows, mhh_stats_chunk_rows
constexpr int LEVEL_THREADS = BX*BY;

// the interior columns a reduction runs over and the strides of the fields
struct LevelDomain { int icells, ijcells, istart, iend, jstart, jend; };
inline LevelDomain level_domain(const mhh_grid* g) { return {g->icells, g->ijcells, g->istart, g->iend, g->jstart, g->jend}; }

// ---- the launch: one block column, level_chunks block rows, nk levels, so that k is fixed per block -------------------------
inline int level_chunks(const mhh_grid* g) { return (g->jmax + LEVEL_ROWS-1)/LEVEL_ROWS; }
inline Tiling level_tiling(const mhh_grid* g, int nk) { return make_tiling(BX, level_chunks(g)*BY, nk); }

// the block's level k = k0 + kz, its chunk `by` and the rows [j0, j1) of the chunk
struct LevelTile { int k, kz, by, j0, j1; };
__device__ __forceinline__ bool level_tile(const Tiling& t, unsigned L, int k0, const LevelDomain& D, LevelTile& T)
{
    int bx;
    if (!decode_tile(t, L, bx, T.by, T.kz)) return false;         // the whole block leaves: no thread is left at a barrier
    T.k = k0 + T.kz;
    T.j0 = D.jstart + T.by*LEVEL_ROWS;
    T.j1 = (T.j0 + LEVEL_ROWS < D.jend) ? T.j0 + LEVEL_ROWS : D.jend;
    return true;
}

// f(i, j, ij) over this thread's cells of the rows [j0, j1), ij = i + j*icells: the order every accumulator is filled in.
// UNROLL > 1 keeps that many loads of a row in flight where the term is a single load (the adds stay in order).
template<int UNROLL = 1, class F>
__device__ __forceinline__ void for_chunk_cells(const LevelDomain& D, int j0, int j1, F&& f)
{
    for (int j=j0+(int)threadIdx.y; j<j1; j+=BY)
#pragma unroll UNROLL
        for (int i=D.istart+(int)threadIdx.x; i<D.iend; i+=BX)
            f(i, j, i + j*D.icells);
}

// ---- the block's sum, two orders ----------------------------------------------------------------------------------------------
// The binary tree over the 256 values of a block: red[t] += red[t+s] for s = 128, 64, .. 1. The order of mhh_field_mean_profile and
// mhh_field_mean_sum (mean_partial_kernel, mean_sum_finish_kernel). The result is thread 0's; one call per kernel (the LDS is not
// guarded against a second). Every thread of the block calls it.
__device__ __forceinline__ double block_tree_sum(double v)
{
    __shared__ double red[LEVEL_THREADS];
    const int tid = threadIdx.x + threadIdx.y*BX;
    red[tid] = v;
    __syncthreads();
    for (int s=LEVEL_THREADS/2; s>0; s>>=1)
    {
        if (tid < s) red[tid] += red[tid+s];
        __syncthreads();
    }
    return red[0];
}

// The block's sums of NM values per thread: out, valid in thread n < NM, is the sum of v[n] over the 256 threads in a fixed order
// (sixteen runs of sixteen consecutive thread ids, then the sixteen runs). The order of every masked sum: mhh_stats_sums,
// mhh_stats_columns, mhh_budget_2_sums, mhh_budget_2_model_sums. Three barriers whatever NM is; every thread of the block calls it,
// any number of times.
template<int NM>
__device__ __forceinline__ double block_sums(const double (&v)[NM])
{
    __shared__ double red[NM*LEVEL_THREADS];
    __shared__ double red2[NM*16];
    const int tid = threadIdx.x + threadIdx.y*BX;
    __syncthreads();                                               // the previous use of red and red2 is over
#pragma unroll
    for (int n=0; n<NM; ++n) red[n*LEVEL_THREADS + tid] = v[n];
    __syncthreads();
    if (tid < NM*16)
    {
        const double* q = red + (tid >> 4)*LEVEL_THREADS + (tid & 15)*16;
        double t = 0.;
        for (int c=0; c<16; ++c) t += q[c];
        red2[tid] = t;
    }
    __syncthreads();
    double out = 0.;
    if (tid < NM)
        for (int c=0; c<16; ++c) out += red2[tid*16 + c];
    return out;
}

// Masks are spread over NM accumulators per thread, NM = 1, 2, 4, 8: the next power of two at or above nmasks (bits of masks that
// do not exist are never set). f(std::integral_constant<int, NM>{}) runs with that width as a compile-time constant.
template<class F>
inline void with_mask_width(int nmasks, F&& f)
{
    if (nmasks == 1)      f(std::integral_constant<int, 1>{});
    else if (nmasks == 2) f(std::integral_constant<int, 2>{});
    else if (nmasks <= 4) f(std::integral_constant<int, 4>{});
    else                  f(std::integral_constant<int, 8>{});
}

// ---- the chunks of a level ------------------------------------------------------------------------------------------------------
// part[row][kcells][nchunks] -> sums[row][kcells], row = blockIdx.y: the chunks of a level in index order, zero outside the levels
// k0 .. k0+nk-1 of the row's range. `rows` consecutive rows share a range (the masks of a Stats job; every row of a Budget_2 call).
constexpr int LEVEL_MAX_RANGES = 16;
struct LevelRanges { int rows, k0[LEVEL_MAX_RANGES], nk[LEVEL_MAX_RANGES]; };
__global__ void __launch_bounds__(256) level_sums_kernel(const double* __restrict__ part, double* __restrict__ sums, int kcells, int nchunks, const LevelRanges R)
{
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= kcells) return;
    const size_t o = (size_t)blockIdx.y*kcells + k;
    const int r = blockIdx.y / R.rows;
    double tmp = 0.;
    if (k >= R.k0[r] && k < R.k0[r] + R.nk[r])
        for (int c=0; c<nchunks; ++c) tmp += part[o*nchunks + c];
    sums[o] = tmp;
}
inline int level_sums_launch(const mhh_grid* g, const double* part, double* sums, int nrows, const LevelRanges& R, hipStream_t st)
{
    hipLaunchKernelGGL(level_sums_kernel, dim3((g->kcells + 255)/256, nrows), dim3(256), 0, st, part, sums, g->kcells, level_chunks(g), R);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
} // namespace mhh
