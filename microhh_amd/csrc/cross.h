// cross.h -- the sampling of Cross<TF> (src/cross.cxx) with the fields left on the device: the gather of the planes the slice writers
// of src/field3d_io.cxx (:754-861) copy out, calc_lngrad_2nd / calc_lngrad_4th on the cells of the requested planes only,
// calc_cross_path and calc_cross_height_threshold per column, and the index search of Cross::create on the host.
// Kernels and C-ABI entry points; included from k_stencil.hip. Every kernel writes interior cells PACKED, in the layout the
// writers put on disk (XY and PLANE [jmax][imax], XZ [k1-k0][imax], YZ [k1-k0][jmax]), so that one contiguous staging buffer
// goes to the host in one copy. Plain loads and vector stores; no reduction, no atomics.
#pragma once
#include <algorithm>
#include <vector>

namespace mhh
{
constexpr int CNJ = MHH_CROSS_MAX_JOBS;

template<class TF> struct CrossJob { const TF* fld; TF* out; TF offset; int kind, index, k0, k1; };
template<class TF> struct CrossArgs
{
    CrossJob<TF> job[CNJ];
    int imax, jmax, igc, jgc, icells, ijcells, kstart, kend;
    TF dxi, dyi; const TF* dzi;                 // lngrad only: gd.dxi, gd.dyi (1./dx narrowed, src/grid.cxx:244), dzi or dzi4
};

// Element n of a job's packed plane -> the cell (i, j, k) it is taken from. Consecutive n are consecutive i for XY, XZ and PLANE
// (coalesced) and consecutive j for YZ: a column of a row-major field is strided by nature, over jmax*(k1-k0) elements.
template<class TF>
__device__ __forceinline__ bool cross_cell(const CrossArgs<TF>& A, const CrossJob<TF>& J, unsigned n, int& i, int& j, int& k)
{
    const bool flat = (J.kind == MHH_CROSS_XY || J.kind == MHH_CROSS_PLANE);
    const int ncol = (J.kind == MHH_CROSS_YZ) ? A.jmax : A.imax;
    const int nrow = flat ? A.jmax : J.k1 - J.k0;
    if (n >= (unsigned)ncol * (unsigned)nrow) return false;
    const int row = (int)(n / (unsigned)ncol), col = (int)(n - (unsigned)row * (unsigned)ncol);
    if (flat)                          { i = col + A.igc; j = row + A.jgc; k = (J.kind == MHH_CROSS_XY) ? J.index : 0; }
    else if (J.kind == MHH_CROSS_XZ)   { i = col + A.igc; j = J.index;     k = J.k0 + row; }
    else                               { i = J.index;     j = col + A.jgc; k = J.k0 + row; }
    return true;
}

// save_xy_slice / save_xz_slice / save_yz_slice (src/field3d_io.cxx:754-861): tmp[ijkb] = data[ijk] + data0
template<class TF>
__global__ void __launch_bounds__(256) cross_gather_kernel(const CrossArgs<TF> A)
{
    const CrossJob<TF>& J = A.job[blockIdx.y];
    const unsigned n = blockIdx.x*256u + threadIdx.x;
    int i, j, k;
    if (!cross_cell(A, J, n, i, j, k)) return;
    J.out[n] = J.fld[(size_t)i + (size_t)j*A.icells + (size_t)k*A.ijcells] + J.offset;
}

// calc_lngrad_2nd (src/cross.cxx:136-167): the squares in TF (pow(x, TF(2))), the sum with Constants::dtiny (a double) and the log in
// double, narrowed last. calc_lngrad_4th (:42-133): the exponent is `2.`, so the squares are in double as well; the vertical
// interpolation has its own first row bi* at kstart and its own last row ti* at kend-1 (the top loop runs last: it wins on one level).
template<class TF> __device__ __forceinline__ TF cross_i4(TF c0, TF c1, TF c2, TF c3, TF a, TF b, TF c, TF d) { return c0*a + c1*b + c2*c + c3*d; }
template<class TF> __device__ __forceinline__ TF cross_grad4(const TF* __restrict__ a, size_t c, size_t s)
{
    const TF ci0 = TF(-1./16.), ci1 = TF(9./16.), ci2 = TF(9./16.), ci3 = TF(-1./16.);
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    return cg0*cross_i4(ci0, ci1, ci2, ci3, a[c-3*s], a[c-2*s], a[c-s  ], a[c    ])
         + cg1*cross_i4(ci0, ci1, ci2, ci3, a[c-2*s], a[c-s  ], a[c    ], a[c+s  ])
         + cg2*cross_i4(ci0, ci1, ci2, ci3, a[c-s  ], a[c    ], a[c+s  ], a[c+2*s])
         + cg3*cross_i4(ci0, ci1, ci2, ci3, a[c    ], a[c+s  ], a[c+2*s], a[c+3*s]);
}
template<class TF> __device__ __forceinline__ TF cross_grad4_z(const TF* __restrict__ a, size_t c, size_t s, bool bot, bool top)
{
    const TF ci0 = TF(-1./16.), ci1 = TF(9./16.), ci2 = TF(9./16.), ci3 = TF(-1./16.);
    const TF bi0 = TF(5./16.), bi1 = TF(15./16.), bi2 = TF(-5./16.), bi3 = TF(1./16.);
    const TF ti0 = TF(1./16.), ti1 = TF(-5./16.), ti2 = TF(15./16.), ti3 = TF(5./16.);
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    const TF first = bot ? cross_i4(bi0, bi1, bi2, bi3, a[c-2*s], a[c-s  ], a[c    ], a[c+s  ])
                         : cross_i4(ci0, ci1, ci2, ci3, a[c-3*s], a[c-2*s], a[c-s  ], a[c    ]);
    const TF last  = top ? cross_i4(ti0, ti1, ti2, ti3, a[c-s  ], a[c    ], a[c+s  ], a[c+2*s])
                         : cross_i4(ci0, ci1, ci2, ci3, a[c    ], a[c+s  ], a[c+2*s], a[c+3*s]);
    return cg0*first
         + cg1*cross_i4(ci0, ci1, ci2, ci3, a[c-2*s], a[c-s  ], a[c    ], a[c+s  ])
         + cg2*cross_i4(ci0, ci1, ci2, ci3, a[c-s  ], a[c    ], a[c+s  ], a[c+2*s])
         + cg3*last;
}
template<class TF> __device__ __forceinline__ TF cross_interp2(TF a, TF b) { return TF(0.5) * (a + b); }

template<class TF, int ORDER>
__global__ void __launch_bounds__(256) cross_lngrad_kernel(const CrossArgs<TF> A)
{
    const CrossJob<TF>& J = A.job[blockIdx.y];
    const unsigned n = blockIdx.x*256u + threadIdx.x;
    int i, j, k;
    if (!cross_cell(A, J, n, i, j, k)) return;
    const TF* __restrict__ a = J.fld;
    const size_t jj = A.icells, kk = A.ijcells, c = (size_t)i + (size_t)j*jj + (size_t)k*kk;
    const double dtiny = 1.e-30;                                   // Constants::dtiny (include/constants.h:95)
    const TF dzik = A.dzi[k];
    double sum;
    if constexpr (ORDER == 2)
    {
        const TF gx = ( cross_interp2(a[c], a[c+1 ]) - cross_interp2(a[c-1 ], a[c]) ) * A.dxi;
        const TF gy = ( cross_interp2(a[c], a[c+jj]) - cross_interp2(a[c-jj], a[c]) ) * A.dyi;
        const TF gz = ( cross_interp2(a[c], a[c+kk]) - cross_interp2(a[c-kk], a[c]) ) * dzik;
        const TF px = gx*gx, py = gy*gy, pz = gz*gz;
        sum = dtiny + px + py + pz;
    }
    else
    {
        const bool top = (k == A.kend-1), bot = (k == A.kstart) && !top;
        const double gx = cross_grad4(a, c, (size_t)1) * A.dxi;
        const double gy = cross_grad4(a, c, jj) * A.dyi;
        const double gz = cross_grad4_z(a, c, kk, bot, top) * dzik;
        sum = dtiny + gx*gx + gy*gy + gz*gz;
    }
    J.out[n] = TF(::log(sum));
}

// calc_cross_path (src/cross.cxx:170-197): one thread per column marching up, tmp += rhoref[k] * data[ijk] * dz[k] serially in TF in
// exactly that operand order ((rho*data)*dz; Stats' calc_path multiplies data*rho*dz, which rounds differently). out [jmax][imax].
template<class TF>
struct CrossPathOp
{
    const TF* __restrict__ data; const TF* __restrict__ rho; const TF* __restrict__ dz; TF* __restrict__ out;
    int istart, jstart, imax, ijcells, kstart, kend;
    __device__ void operator()(int i, int j, int, int col) const
    {
        const size_t ij = (size_t)col;
        TF acc = TF(0.);
        for (int k=kstart; k<kend; ++k)
            acc += rho[k] * data[ij + (size_t)k*ijcells] * dz[k];
        out[(size_t)(i-istart) + (size_t)(j-jstart)*imax] = acc;
    }
};

// calc_cross_height_threshold (src/cross.cxx:200-250): z[k] of the lowest (upward) or highest level with data > threshold, the
// fill value where no level qualifies. out [jmax][imax].
template<class TF>
struct CrossHeightOp
{
    const TF* __restrict__ data; const TF* __restrict__ z; TF* __restrict__ out; TF threshold; int upward; TF fillvalue;
    int istart, jstart, imax, ijcells, kstart, kend;
    __device__ void operator()(int i, int j, int, int col) const
    {
        const size_t ij = (size_t)col;
        TF h = fillvalue;
        if (upward)
        {
            for (int k=kstart; k<kend; ++k)
                if (data[ij + (size_t)k*ijcells] > threshold) { h = z[k]; break; }
        }
        else
        {
            for (int k=kend-1; k>kstart-1; --k)
                if (data[ij + (size_t)k*ijcells] > threshold) { h = z[k]; break; }
        }
        out[(size_t)(i-istart) + (size_t)(j-jstart)*imax] = h;
    }
};

// ---- host side ----------------------------------------------------------------------------------------------------------------
// What every job must satisfy before a kernel indexes with it; lngrad: the planes lie in the interior, where the stencils of
// the order stay inside the array (checked against the ghost cells by the caller).
inline int cross_check_jobs(const mhh_grid* g, const mhh_cross_job* jobs, int njobs, bool lngrad)
{
    MHH_REQUIRE(jobs && njobs >= 1, "at least one job");
    for (int n=0; n<njobs; ++n)
    {
        const mhh_cross_job& j = jobs[n];
        if (j.kind != MHH_CROSS_XY && j.kind != MHH_CROSS_XZ && j.kind != MHH_CROSS_YZ && !(j.kind == MHH_CROSS_PLANE && !lngrad))
        { set_error("%s: job %d: unknown kind %d (MHH_CROSS_XY | XZ | YZ%s)", lngrad ? "mhh_cross_lngrad" : "mhh_cross_gather", n, j.kind, lngrad ? "" : " | PLANE"); return MHH_EINVAL; }
        if (!j.fld || !j.out) { set_error("cross job %d: null pointer", n); return MHH_EINVAL; }
        if (j.kind == MHH_CROSS_PLANE) continue;
        const int lo[3] = {lngrad ? g->kstart : 0, lngrad ? g->jstart : 0, lngrad ? g->istart : 0};
        const int hi[3] = {lngrad ? g->kend : g->kcells, lngrad ? g->jend : g->jcells, lngrad ? g->iend : g->icells};
        if (j.index < lo[j.kind] || j.index >= hi[j.kind])
        { set_error("cross job %d: index %d outside the rank's range [%d, %d)", n, j.index, lo[j.kind], hi[j.kind]); return MHH_EINVAL; }
        if (j.kind != MHH_CROSS_XY && (j.k0 < lo[0] || j.k1 > hi[0] || j.k0 > j.k1))
        { set_error("cross job %d: k0 = %d, k1 = %d outside [%d, %d]", n, j.k0, j.k1, lo[0], hi[0]); return MHH_EINVAL; }
    }
    return MHH_OK;
}

template<class TF, int ORDER>          // ORDER 0: the gather
static int cross_launch(const mhh_grid* g, const mhh_cross_job* jobs, int njobs, hipStream_t st)
{
    for (int b=0; b<njobs; b+=CNJ)      // a batch of CNJ jobs travels by value with its launch
    {
        const int nb = std::min(CNJ, njobs - b);
        CrossArgs<TF> A{};
        A.imax = g->imax; A.jmax = g->jmax; A.igc = g->igc; A.jgc = g->jgc; A.icells = g->icells; A.ijcells = g->ijcells;
        A.kstart = g->kstart; A.kend = g->kend;
        A.dxi = TF(1./TF(g->dx)); A.dyi = TF(1./TF(g->dy)); A.dzi = cp<TF>(ORDER == 4 ? g->dzi4 : g->dzi);
        unsigned most = 0;
        for (int n=0; n<nb; ++n)
        {
            const mhh_cross_job& j = jobs[b + n];
            // the offset is narrowed before the add (TF data0, src/field3d_io.cxx:756)
            A.job[n] = CrossJob<TF>{cp<TF>(j.fld), mp<TF>(j.out), TF(j.offset), j.kind, j.index, j.k0, j.k1};
            const bool flat = (j.kind == MHH_CROSS_XY || j.kind == MHH_CROSS_PLANE);
            const unsigned cells = (unsigned)(j.kind == MHH_CROSS_YZ ? g->jmax : g->imax) * (unsigned)(flat ? g->jmax : j.k1 - j.k0);
            most = std::max(most, cells);
        }
        if (!most) continue;
        const dim3 grid((most + 255u)/256u, nb), block(256);
        if (ORDER == 0)      hipLaunchKernelGGL(cross_gather_kernel<TF>, grid, block, 0, st, A);
        else if (ORDER == 2) hipLaunchKernelGGL((cross_lngrad_kernel<TF, 2>), grid, block, 0, st, A);
        else                 hipLaunchKernelGGL((cross_lngrad_kernel<TF, 4>), grid, block, 0, st, A);
        MHH_LAUNCH_CHECK();
    }
    return MHH_OK;
}

// Cross::create (src/cross.cxx:323-460) for one direction, in global indices. `it` and the grid spacing are TF as there: the full
// index is floor of a TF quotient, the half index floor of a double one ((it + d/2.)/d).
template<class TF>
static int cross_indices(const mhh_grid* g, int kind, const double* loc, int nloc, std::vector<int>& full, std::vector<int>& half)
{
    auto add = [](std::vector<int>& v, int x) { if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x); };
    const char* sect = (kind == MHH_CROSS_XY) ? "xy" : (kind == MHH_CROSS_XZ) ? "xz" : "yz";
    for (int n=0; n<nloc; ++n)
    {
        const TF it = TF(loc[n]);
        const TF size = TF(kind == MHH_CROSS_XY ? g->zsize : kind == MHH_CROSS_XZ ? g->ysize : g->xsize);
        if (it < 0 || it > size)
        { set_error("%f in [cross][%s] is outside domain", double(it), sect); return MHH_EINVAL; }
        if (kind != MHH_CROSS_XY)
        {
            const TF d = TF(kind == MHH_CROSS_XZ ? g->dy : g->dx);
            int temploc = (int) floor(it/d);
            const int temploch = (int) floor((it+(d/2.))/d);
            if (it == size) --temploc;                       // exception for the full level when requesting the domain size
            add(full, temploc); add(half, temploch);
            continue;
        }
        const TF* z = cp<TF>(g->z); const TF* zh = cp<TF>(g->zh);
        int temploc = 0, hoffset = 0;
        if (it == size) { temploc = g->kmax-1; hoffset = 1; }  // the domain top: the half level at the top, the full level below
        else
            for (int k=g->kstart; k<g->kend; ++k)
                if ((it >= zh[k]) && (it < zh[k+1]))
                {
                    temploc = k - g->kgc;
                    if (it >= z[k]) hoffset = 1;
                    break;
                }
        add(full, temploc); add(half, temploc + hoffset);
    }
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

// save_xy_slice, save_xz_slice, save_yz_slice (src/field3d_io.cxx:754-861) of Cross::cross_simple and cross_plane
// (src/cross.cxx:564-651) without the write: every job's plane, packed, at its own place of the staging buffer
MHH_API int mhh_cross_gather(const mhh_grid* g, const mhh_cross_job* jobs, int njobs, void* stream)
{
    if (int e = check_grid(g)) return e;
    if (int e = cross_check_jobs(g, jobs, njobs, false)) return e;
#define CALL(TF) cross_launch<TF, 0>(g, jobs, njobs, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_lngrad_2nd (src/cross.cxx:136-167) / calc_lngrad_4th (:42-133) of Cross::cross_lngrad (:653-703) on the cells of the jobs'
// planes; the offset of a job is not read (no_offset, :676)
MHH_API int mhh_cross_lngrad(const mhh_grid* g, int order, const mhh_cross_job* jobs, int njobs, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(order == 2 || order == 4, "order: 2 (calc_lngrad_2nd) or 4 (calc_lngrad_4th)");
    const int need = (order == 2) ? 1 : 3;
    MHH_REQUIRE(g->igc >= need && g->jgc >= need && g->kgc >= need, "lngrad reads one ghost cell in every direction (order 2), three (order 4)");
    MHH_REQUIRE(order == 2 ? g->dzi != NULL : g->dzi4 != NULL, "null metric: dzi (order 2), dzi4 (order 4)");
    if (int e = cross_check_jobs(g, jobs, njobs, true)) return e;
    if (order == 2)
    {
#define CALL(TF) cross_launch<TF, 2>(g, jobs, njobs, as_stream(stream))
        return MHH_DISPATCH(g, CALL);
#undef CALL
    }
#define CALL(TF) cross_launch<TF, 4>(g, jobs, njobs, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_cross_path (src/cross.cxx:170-197) of Cross::cross_path (:705-725): out [jmax][imax], what cross_plane then writes
MHH_API int mhh_cross_path(const mhh_grid* g, const void* fld, const void* rhoref, void* out, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(fld && rhoref && g->dz && out, "null pointer");
#define CALL(TF) launch_columns(as_stream(stream), make_grid<TF>(g), 1, CrossPathOp<TF>{cp<TF>(fld), cp<TF>(rhoref), cp<TF>(g->dz), mp<TF>(out), \
                                g->istart, g->jstart, g->imax, g->ijcells, g->kstart, g->kend})
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_cross_height_threshold (src/cross.cxx:200-250) with the fill value TF(-1e-9) of Cross::cross_height_threshold (:738-760);
// upward != 0: Cross_direction::Bottom_to_top. out [jmax][imax]
MHH_API int mhh_cross_height_threshold(const mhh_grid* g, const void* fld, double threshold, int upward, void* out, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(fld && g->z && out, "null pointer");
#define CALL(TF) launch_columns(as_stream(stream), make_grid<TF>(g), 1, CrossHeightOp<TF>{cp<TF>(fld), cp<TF>(g->z), mp<TF>(out), TF(threshold), \
                                upward ? 1 : 0, TF(-1e-9), g->istart, g->jstart, g->imax, g->ijcells, g->kstart, g->kend})
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// The search of Cross::create (src/cross.cxx:323-460) for the locations of one direction (MHH_CROSS_XY: [cross] xy, heights; XZ: xz,
// y locations; YZ: yz, x locations), in GLOBAL interior indices. The metric pointers of g are HOST pointers (z and zh are read
// for XY). full / half hold up to nloc indices each, duplicates dropped per list; a location outside the domain is refused by name.
MHH_API int mhh_cross_indices_host(const mhh_grid* g, int kind, const double* loc, int nloc, int* full, int* nfull, int* half, int* nhalf)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(kind == MHH_CROSS_XY || kind == MHH_CROSS_XZ || kind == MHH_CROSS_YZ, "unknown kind (MHH_CROSS_XY | XZ | YZ)");
    MHH_REQUIRE(nloc >= 0 && (nloc == 0 || (loc && full && half)) && nfull && nhalf, "null pointer");
    MHH_REQUIRE(kind != MHH_CROSS_XY || (g->z && g->zh), "null metric: z, zh");
    std::vector<int> f, h;
#define CALL(TF) cross_indices<TF>(g, kind, loc, nloc, f, h)
    if (int e = MHH_DISPATCH(g, CALL)) return e;
#undef CALL
    std::copy(f.begin(), f.end(), full); std::copy(h.begin(), h.end(), half);
    *nfull = (int)f.size(); *nhalf = (int)h.size();
    return MHH_OK;
}
