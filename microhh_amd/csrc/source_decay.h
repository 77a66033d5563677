// source_decay.h -- Source<TF> (src/source.cxx) and Decay<TF>::exec (src/decay.cxx): tracer emissions and exponential decay.
// Kernels and C-ABI entry points; included from k_stencil.hip.
//
// Source: the set-up of Source::create on the HOST (calc_shape, calc_shape_profile, calc_norm; no GPU is read), and ONE launch per
// sub-step for all sources of all scalars. The pass is cell-centric: the interior is cut into tiles of 16 x 4 x 4 cells that sit on
// a fixed lattice (so the boxes of different sources meet in the same tiles), a tile is one block of 256 threads, and the job table
// holds the tiles that at least one box touches, each with its slice of an ordered source list. A thread owns one cell, reads its
// tendency once, adds the contributions of the tile's sources whose box holds the cell IN SOURCE ORDER and writes it once: the bits
// of the reference's sequential st[ijk] += ... loops where sources overlap on one scalar. A wave covers 16 consecutive i of 4 rows
// (fp64: four whole 128-byte lines) at one level, so k and everything that depends on it is wave-uniform.
//
// Nothing is divided in the cell loop: pow2(coordinate - centre - line)/pow2(sigma) depends on one index, so each source has three
// axis tables made here with the host's (correctly rounded) division. The three-branch choice of a line source depends on the
// coordinate along the line alone and lives in that axis's table; inside the segment the entry is +0, and (-0 - B) - C, (-A - 0) - C,
// (-A - B) - 0 have the bits of the reference's expressions with the term left out. strength/norm is one division per source, made
// where the table is built. The source descriptors, the tile table and the order list are indexed with block-uniform values only.
#pragma once
#include "level_reduce.h"
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <tuple>
#include <vector>

struct mhh_source                      // the opaque handle of include/mhh_hip.h
{
    virtual ~mhh_source() {}
    int dtype = 0;
};

namespace mhh
{
constexpr int STX = 16, STY = 4, STZ = 4;          // the tile: 16 x 4 cells of a level per wave, 4 levels per block

template<class TF> struct SrcDev { TF c; int i0, i1, j0, j1, k0, k1, ox, oy, oz, profile; };
struct SrcTile { int i0, j0, k0, fld, s0, s1; };
template<class TF> struct SrcArgs
{
    TF* st[MHH_MAX_SCALARS];
    const SrcDev<TF>* src; const SrcTile* tile; const int* order; const TF* tab;
    int icells, ijcells, iend, jend, kend;
};

// calc_source (src/source.cxx:100-190): strength/norm * exp(((-ax) - ay) - az), or strength/norm * (exp((-ax) - ay) * profile[k]).
// The reference's `exp` is unqualified in a translation unit that includes <cmath> alone, so it is C's exp(double) for float as
// well: the exponent is formed in TF, widened, and the product with strength/norm and the sum with st[ijk] are DOUBLE operations
// narrowed by the assignment. C++'s own promotions of the expressions below say the same for both dtypes.
template<class TF>
__global__ void __launch_bounds__(256) source_kernel(const SrcArgs<TF> A)
{
    const SrcTile T = A.tile[blockIdx.x];
    const int t = (int)threadIdx.x;
    const int i = T.i0 + (t & (STX-1)), j = T.j0 + ((t >> 4) & (STY-1)), k = T.k0 + (t >> 6);
    if (i >= A.iend || j >= A.jend || k >= A.kend) return;           // a ragged tile: the lane sits out (no barrier below)
    TF* __restrict__ st = A.st[T.fld];
    const TF* __restrict__ tab = A.tab;
    const size_t ijk = (size_t)i + (size_t)j*A.icells + (size_t)k*A.ijcells;
    TF acc = st[ijk];
    bool hit = false;
    for (int m=T.s0; m<T.s1; ++m)
    {
        const SrcDev<TF>& S = A.src[A.order[m]];
        if (i < S.i0 || i >= S.i1 || j < S.j0 || j >= S.j1 || k < S.k0 || k >= S.k1) continue;
        const TF ax = tab[S.ox + i], ay = tab[S.oy + j], az = tab[S.oz + k];
        const TF arg = S.profile ? -ax - ay : (-ax - ay) - az;
        const double e = ::exp((double)arg);
        acc = S.profile ? TF(acc + S.c*(e*az)) : TF(acc + S.c*e);
        hit = true;
    }
    if (hit) st[ijk] = acc;
}

// enforce_exponential_decay (src/decay.cxx:35-51) for every decaying scalar of the launch
template<class TF>
struct DecayOp
{
    TF* st[MHH_MAX_SCALARS]; const TF* s[MHH_MAX_SCALARS]; TF rate[MHH_MAX_SCALARS]; int n;
    __device__ void operator()(int, int, int, int ijk) const
    {
        for (int m=0; m<n; ++m)
            st[m][ijk] -= rate[m] * s[m][ijk];
    }
};

// Decay::get_mask("couvreux") (src/decay.cxx:123-187). The sums of s and s*s (the square in TF, as there) per level through the
// level_reduce.h skeleton: doubles, the cells of a chunk in the skeleton's order, block_sums, then the chunks in index order.
template<class TF>
__global__ void __launch_bounds__(LEVEL_THREADS) couvreux_partial_kernel(const TF* __restrict__ s, const LevelDomain dom, const Tiling t, int k0,
                                                                         double* __restrict__ part, int kcells, int nchunks)
{
    LevelTile T;
    if (!level_tile(t, blockIdx.x, k0, dom, T)) return;
    const TF* __restrict__ fld = s + (size_t)T.k*dom.ijcells;
    double v[2] = {0., 0.};
    for_chunk_cells(dom, T.j0, T.j1, [&](int, int, int ij) { const TF x = fld[ij]; v[0] += double(x); v[1] += double(x*x); });
    const double sum = block_sums<2>(v);
    const int tid = threadIdx.x + threadIdx.y*BX;
    if (tid < 2) part[((size_t)tid*kcells + T.k)*nchunks + T.by] = sum;
}

// couvreux = s - mean - nstd*sqrt(mean(s*s) - mean*mean) on the interior (:158-171), in TF from the narrowed quotients
template<class TF>
struct CouvreuxOp
{
    TF* __restrict__ out; const TF* __restrict__ s; const double* __restrict__ sums; TF nstd; double ijtot; int kcells;
    __device__ void operator()(int, int, int k, int ijk) const
    {
        const TF mean = TF(sums[k] / ijtot);
        TF var = TF(sums[kcells + k] / ijtot);
        var -= mean*mean;
        const TF sd = sqrt(var);
        out[ijk] = s[ijk] - mean - nstd * sd;
    }
};
// grid.interpolate_2nd(couvreuxh, couvreux, sloc, wloc) (src/grid.cxx:455-499): iih = jjh = 0, kkh = -kk; the literals are doubles
template<class TF>
struct CouvreuxHalfOp
{
    TF* __restrict__ outh; const TF* __restrict__ in; int kk;
    __device__ void operator()(int, int, int k, int ijk) const
    {
        const TF a = in[ijk];
        if (k == 0) { outh[ijk] = 0.25*(0.5*a + 0.5*a) + 0.25*(0.5*a + 0.5*a); return; }
        const TF b = in[ijk-kk];
        outh[ijk] = 0.25*(0.5*a + 0.5*a) + 0.25*(0.5*a + 0.5*a) + 0.25*(0.5*b + 0.5*b) + 0.25*(0.5*b + 0.5*b);
    }
};

// ---- host side: the set-up of Source::create ----------------------------------------------------------------------------------
// calc_shape (src/source.cxx:44-75): no periodic wrap, clipped to [start, end)
template<class TF>
inline void src_shape(const TF* x, TF x0, TF sigma, TF line, int start, int end, int* range)
{
    range[0] = end; range[1] = end;
    for (int i=start; i<end; ++i)
        if (x[i]-x0 + TF(4)*sigma > TF(0)) { range[0] = i; break; }
    for (int i=start; i<end; ++i)
        if (x[i]-x0-line - TF(4)*sigma > TF(0)) { range[1] = i; break; }
}

// calc_shape_profile (:77-98): the levels with profile > Constants::dsmall; none: the vector's zeroes, an empty range
template<class TF>
inline void src_shape_profile(const TF* prof, int kstart, int kend, int* range)
{
    range[0] = 0; range[1] = 0;
    for (int k=kstart; k<kend; ++k)
        if (prof[k] > 1.e-9) { range[0] = k; break; }
    for (int k=kend-1; k>=kstart; --k)
        if (prof[k] > 1.e-9) { range[1] = k+1; break; }
}

// One quotient of the exponent. segment: this axis carries the three-branch treatment of a line source (:125-175)
template<class TF>
inline TF src_axis(TF x, TF x0, TF sigma, TF line, bool segment)
{
    if (segment)
    {
        if (x >= x0+line) { const TF d = x-x0-line; return (d*d)/(sigma*sigma); }
        if (x <= x0)      { const TF d = x-x0;      return (d*d)/(sigma*sigma); }
        return TF(0);
    }
    const TF d = x-x0-line;
    return (d*d)/(sigma*sigma);
}

template<class TF>
struct Source : mhh_source
{
    struct One
    {
        int scalar, swvmr, prof;
        TF x0, y0, z0, sx, sy, sz, lx, ly, lz, strength, norm;
        int r[6];                  // this rank's range_x, range_y, range_z
        int gy[2];                 // range_y of the whole domain (rows of the one-rank grid)
    };
    mhh_grid g;                    // the index bundle; its metric pointers are not kept
    int joff = 0;                  // first row of this rank in the one-rank grid
    std::vector<TF> x, yg, z, dz, rhoref, prof;         // yg: [jtot + 2 jgc], the one-rank grid's y
    int nprof = 0;
    std::vector<One> src;
    // the device image: descriptors, tiles, order, tables in one allocation
    std::vector<char> image;
    char* dev = nullptr; size_t cap = 0;
    size_t off_tile = 0, off_order = 0, off_tab = 0;
    int ntiles = 0;

    ~Source() override { if (dev) (void)hipFree(dev); }

    int segment_axis(const One& s) const { return s.lx != 0 ? 0 : s.ly != 0 ? 1 : s.lz != 0 ? 2 : -1; }
    const TF* profile_of(const One& s) const { return s.prof < 0 ? nullptr : prof.data() + (size_t)s.prof*g.kcells; }

    void shape(One& s)
    {
        src_shape(x.data(), s.x0, s.sx, s.lx, g.istart, g.iend, s.r);
        src_shape(yg.data(), s.y0, s.sy, s.ly, g.jgc, g.jgc + g.jtot, s.gy);
        s.r[2] = std::min(std::max(s.gy[0] - joff, g.jstart), g.jend);
        s.r[3] = std::min(std::max(s.gy[1] - joff, g.jstart), g.jend);
        if (s.prof >= 0) src_shape_profile(profile_of(s), g.kstart, g.kend, s.r + 4);
        else             src_shape(z.data(), s.z0, s.sz, s.lz, g.kstart, g.kend, s.r + 4);
    }

    // Source::calc_norm (:435-547) over the box alone, in its k, j, i order: outside the box the reference adds +0 to a non-negative
    // sum. The test is INCLUSIVE (i <= range[1]) where the emission loop is exclusive. Whole domain: every rank finds the same number.
    void calc_norm(One& s)
    {
        const int seg = segment_axis(s);
        const TF* p = profile_of(s);
        const TF dx = TF(g.dx), dy = TF(g.dy);
        const int i1 = std::min(s.r[1], g.iend-1), j1 = std::min(s.gy[1], g.jgc + g.jtot - 1), k1 = std::min(s.r[5], g.kend-1);
        TF sum = 0.;
        for (int k=std::max(s.r[4], g.kstart); k<=k1; ++k)
        {
            const TF scaling = s.swvmr ? rhoref[k]/TF(28.9647) : rhoref[k];          // Constants::xmair<TF>
            const TF az = p ? p[k] : src_axis(z[k], s.z0, s.sz, s.lz, seg == 2);
            for (int j=s.gy[0]; j<=j1; ++j)
            {
                const TF ay = src_axis(yg[j], s.y0, s.sy, s.ly, seg == 1);
                for (int i=s.r[0]; i<=i1; ++i)
                {
                    const TF ax = src_axis(x[i], s.x0, s.sx, s.lx, seg == 0);
                    const TF blob = p ? TF(::exp((double)(-ax - ay)) * az) : TF(::exp((double)((-ax - ay) - az)));      // C's exp(double), as above
                    sum += blob*dx*dy*dz[k]*scaling;
                }
            }
        }
        s.norm = sum;
    }

    // descriptors, axis tables, tiles and the ordered source list, then the upload on the stream
    int upload(hipStream_t st)
    {
        const int ns = (int)src.size();
        std::vector<SrcDev<TF>> D(ns);
        std::vector<TF> tab(prof);                 // the profiles first: entry p*kcells + k
        std::map<std::tuple<int, int, int, int>, std::vector<int>> tiles;      // (scalar, tk, tj, ti) -> sources in source order
        for (int n=0; n<ns; ++n)
        {
            const One& s = src[n];
            SrcDev<TF>& d = D[n];
            d = SrcDev<TF>{s.strength/s.norm, s.r[0], s.r[1], s.r[2], s.r[3], s.r[4], s.r[5], 0, 0, 0, s.prof >= 0};
            if (s.r[1] <= s.r[0] || s.r[3] <= s.r[2] || s.r[5] <= s.r[4])      // calc_source returns early (:116)
            { d.i1 = d.i0; continue; }
            const int seg = segment_axis(s);
            d.ox = (int)tab.size() - s.r[0];
            for (int i=s.r[0]; i<s.r[1]; ++i) tab.push_back(src_axis(x[i], s.x0, s.sx, s.lx, seg == 0));
            d.oy = (int)tab.size() - s.r[2];
            for (int j=s.r[2]; j<s.r[3]; ++j) tab.push_back(src_axis(yg[j + joff], s.y0, s.sy, s.ly, seg == 1));
            if (s.prof >= 0) d.oz = s.prof*g.kcells;
            else
            {
                d.oz = (int)tab.size() - s.r[4];
                for (int k=s.r[4]; k<s.r[5]; ++k) tab.push_back(src_axis(z[k], s.z0, s.sz, s.lz, seg == 2));
            }
            for (int tk=(s.r[4]-g.kstart)/STZ; tk<=(s.r[5]-1-g.kstart)/STZ; ++tk)
                for (int tj=(s.r[2]-g.jstart)/STY; tj<=(s.r[3]-1-g.jstart)/STY; ++tj)
                    for (int ti=(s.r[0]-g.istart)/STX; ti<=(s.r[1]-1-g.istart)/STX; ++ti)
                        tiles[std::make_tuple(s.scalar, tk, tj, ti)].push_back(n);
        }
        std::vector<SrcTile> T; std::vector<int> order;
        for (const auto& kv : tiles)
        {
            const int s0 = (int)order.size();
            order.insert(order.end(), kv.second.begin(), kv.second.end());
            T.push_back(SrcTile{g.istart + std::get<3>(kv.first)*STX, g.jstart + std::get<2>(kv.first)*STY, g.kstart + std::get<1>(kv.first)*STZ,
                                std::get<0>(kv.first), s0, (int)order.size()});
        }
        ntiles = (int)T.size();
        auto pad = [](size_t n) { return (n + 15) & ~size_t(15); };
        off_tile = pad(D.size()*sizeof(SrcDev<TF>));
        off_order = off_tile + pad(T.size()*sizeof(SrcTile));
        off_tab = off_order + pad(order.size()*sizeof(int));
        image.assign(off_tab + pad(tab.size()*sizeof(TF)) + 16, 0);
        auto put = [&](size_t off, const void* p, size_t n) { if (n) memcpy(image.data() + off, p, n); };
        put(0, D.data(), D.size()*sizeof(SrcDev<TF>)); put(off_tile, T.data(), T.size()*sizeof(SrcTile));
        put(off_order, order.data(), order.size()*sizeof(int)); put(off_tab, tab.data(), tab.size()*sizeof(TF));
        if (image.size() > cap)
        {
            if (dev) MHH_HIP_TRY(hipFree(dev));
            dev = nullptr; cap = 0;
            MHH_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), image.size()));
            cap = image.size();
        }
        MHH_HIP_TRY(hipMemcpyAsync(dev, image.data(), image.size(), hipMemcpyHostToDevice, st));
        MHH_HIP_TRY(hipStreamSynchronize(st));      // the image may be rebuilt by the next update: the copy has left it by then
        return MHH_OK;
    }

    int exec(const mhh_fields* f, hipStream_t st)
    {
        if (!ntiles) return MHH_OK;
        SrcArgs<TF> A{};
        for (int n=0; n<MHH_MAX_SCALARS; ++n) A.st[n] = mp<TF>(f->st[n]);
        A.src = reinterpret_cast<const SrcDev<TF>*>(dev);
        A.tile = reinterpret_cast<const SrcTile*>(dev + off_tile);
        A.order = reinterpret_cast<const int*>(dev + off_order);
        A.tab = reinterpret_cast<const TF*>(dev + off_tab);
        A.icells = g.icells; A.ijcells = g.ijcells; A.iend = g.iend; A.jend = g.jend; A.kend = g.kend;
        hipLaunchKernelGGL(source_kernel<TF>, dim3(ntiles), dim3(256), 0, st, A);
        MHH_LAUNCH_CHECK();
        return MHH_OK;
    }
};

template<class TF>
static int source_create(const mhh_grid* g, const mhh_source_desc* d, int nsrc, const void* profiles, int nprofiles, const void* rhoref,
                         hipStream_t st, mhh_source** out)
{
    auto* S = new Source<TF>();
    S->dtype = g->dtype;
    S->g = *g;
    S->joff = g->mpicoordy * g->jmax;
    // gd.x, gd.y (src/grid.cxx:252-262) of the ONE-RANK grid: (i-igc)*dx is a product in TF, the sums are in double, narrowed last
    const TF dx = TF(g->dx), dy = TF(g->dy);
    S->x.resize(g->icells); S->yg.resize(g->jtot + 2*g->jgc);
    for (int i=0; i<g->icells; ++i) S->x[i] = TF(0.5*dx + (i-g->igc)*dx + 0.);
    for (int j=0; j<(int)S->yg.size(); ++j) S->yg[j] = TF(0.5*dy + (j-g->jgc)*dy + 0.);
    S->z.assign(cp<TF>(g->z), cp<TF>(g->z) + g->kcells);
    S->dz.assign(cp<TF>(g->dz), cp<TF>(g->dz) + g->kcells);
    S->rhoref.assign(cp<TF>(rhoref), cp<TF>(rhoref) + g->kcells);
    S->nprof = nprofiles;
    if (nprofiles) S->prof.assign(cp<TF>(profiles), cp<TF>(profiles) + (size_t)nprofiles*g->kcells);
    S->src.resize(nsrc);
    for (int n=0; n<nsrc; ++n)
    {
        typename Source<TF>::One& s = S->src[n];
        s.scalar = d[n].scalar; s.swvmr = d[n].swvmr; s.prof = d[n].profile_index;
        s.x0 = TF(d[n].x0); s.y0 = TF(d[n].y0); s.z0 = TF(d[n].z0);
        s.sx = TF(d[n].sigma_x); s.sy = TF(d[n].sigma_y); s.sz = TF(d[n].sigma_z);
        s.lx = TF(d[n].line_x); s.ly = TF(d[n].line_y); s.lz = TF(d[n].line_z);
        s.strength = TF(d[n].strength);
        S->shape(s);
        S->calc_norm(s);
    }
    if (int e = S->upload(st)) { delete S; return e; }
    *out = S;
    return MHH_OK;
}

template<class TF>
static int source_update(mhh_source* h, int n, const double* x0, const double* y0, const double* z0, const double* strength, hipStream_t st)
{
    auto* S = static_cast<Source<TF>*>(h);
    const int ns = (int)S->src.size();
    const bool move = x0 || y0 || z0;
    const int a = n < 0 ? 0 : n, b = n < 0 ? ns : n+1;
    for (int m=a; m<b; ++m)
        if (S->src[m].prof >= 0)      // the reference refuses swtimedep_location and swtimedep_strength alike (:236)
        {
            set_error("mhh_source_update: source %d: Emission profiles with time dependent location/strength are not (yet) supported!", m);
            return MHH_EINVAL;
        }
    for (int m=a; m<b; ++m)
    {
        typename Source<TF>::One& s = S->src[m];
        const int q = m - a;
        if (x0) s.x0 = TF(x0[q]);
        if (y0) s.y0 = TF(y0[q]);
        if (z0) s.z0 = TF(z0[q]);
        if (strength) s.strength = TF(strength[q]);
        if (move) { S->shape(s); S->calc_norm(s); }       // as Source::exec under swtimedep_location (:362-391)
    }
    return S->upload(st);
}
} // namespace mhh
using namespace mhh;

// Source::create (src/source.cxx:266-316): calc_shape / calc_shape_profile and calc_norm per source on the host, the tables uploaded
MHH_API int mhh_source_create(const mhh_grid* g, const mhh_source_desc* src, int nsrc, const void* profiles, int nprofiles, const void* rhoref,
                              void* stream, mhh_source** out)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(out && nsrc >= 0 && (nsrc == 0 || src) && rhoref && g->z && g->dz, "null pointer");
    MHH_REQUIRE(nprofiles >= 0 && (nprofiles == 0 || profiles), "null profiles");
    MHH_REQUIRE(g->mpicoordy >= 0 && g->mpicoordy < g->npy && g->jmax*g->npy == g->jtot, "the slab is not a rank's rows of the whole grid");
    for (int n=0; n<nsrc; ++n)
    {
        const mhh_source_desc& d = src[n];
        if (d.scalar < 0 || d.scalar >= MHH_MAX_SCALARS) { set_error("mhh_source_create: source %d: scalar %d outside [0, %d)", n, d.scalar, MHH_MAX_SCALARS); return MHH_EINVAL; }
        if (d.profile_index >= nprofiles) { set_error("mhh_source_create: source %d: profile_index %d of %d profiles", n, d.profile_index, nprofiles); return MHH_EINVAL; }
        // the reference refuses line > 0 (:242); with a negative length its calc_source would take the line branch and drop the profile
        if (d.profile_index >= 0 && (d.line_x != 0 || d.line_y != 0 || d.line_z != 0))
        { set_error("mhh_source_create: source %d: Emission profiles with line emissions are not (yet) supported!", n); return MHH_EINVAL; }
        if (!(d.sigma_x > 0 && d.sigma_y > 0 && (d.profile_index >= 0 || d.sigma_z > 0))) { set_error("mhh_source_create: source %d: sigma must be positive", n); return MHH_EINVAL; }
    }
    *out = nullptr;
#define CALL(TF) source_create<TF>(g, src, nsrc, profiles, nprofiles, rhoref, as_stream(stream), out)
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

MHH_API void mhh_source_destroy(mhh_source* h) { delete h; }

// Source::exec under swtimedep_location / swtimedep_strength (src/source.cxx:362-401) without the Timedep interpolation, which is the
// caller's: new centres and / or strengths for source n (one value each) or for all (n < 0: arrays of every source); NULL keeps
MHH_API int mhh_source_update(mhh_source* h, int n, const double* x0, const double* y0, const double* z0, const double* strength, void* stream)
{
    MHH_REQUIRE(h, "null handle");
#define CALL(TF) [&]{ if (n >= (int)static_cast<Source<TF>*>(h)->src.size()) { set_error("mhh_source_update: no source %d", n); return (int)MHH_EINVAL; } \
                      return source_update<TF>(h, n, x0, y0, z0, strength, as_stream(stream)); }()
    return h->dtype == MHH_F64 ? CALL(double) : CALL(float);
#undef CALL
}

MHH_API int mhh_source_count(const mhh_source* h)
{
    if (!h) return -1;
    return h->dtype == MHH_F64 ? (int)static_cast<const Source<double>*>(h)->src.size() : (int)static_cast<const Source<float>*>(h)->src.size();
}

// tiles of the job table = blocks of the launch
MHH_API int mhh_source_tiles(const mhh_source* h)
{
    if (!h) return -1;
    return h->dtype == MHH_F64 ? static_cast<const Source<double>*>(h)->ntiles : static_cast<const Source<float>*>(h)->ntiles;
}

// shape[n].range_x, range_y, range_z (this rank's) and norm[n] as Source::create leaves them
MHH_API int mhh_source_ranges(const mhh_source* h, int n, int* range6)
{
    MHH_REQUIRE(h && range6 && n >= 0 && n < mhh_source_count(h), "no such source");
    if (h->dtype == MHH_F64) std::copy(static_cast<const Source<double>*>(h)->src[n].r, static_cast<const Source<double>*>(h)->src[n].r + 6, range6);
    else                     std::copy(static_cast<const Source<float>*>(h)->src[n].r, static_cast<const Source<float>*>(h)->src[n].r + 6, range6);
    return MHH_OK;
}
MHH_API int mhh_source_norm(const mhh_source* h, int n, double* norm)
{
    MHH_REQUIRE(h && norm && n >= 0 && n < mhh_source_count(h), "no such source");
    *norm = h->dtype == MHH_F64 ? static_cast<const Source<double>*>(h)->src[n].norm : (double)static_cast<const Source<float>*>(h)->src[n].norm;
    return MHH_OK;
}

// calc_source (src/source.cxx:100-190) of Source::exec (:403-431) for every source in ONE launch; the reference's GPU path launches
// once per source (src/source.cu). Only enqueues.
MHH_API int mhh_source_exec(mhh_source* h, const mhh_grid* g, const mhh_fields* f, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(h && f, "null pointer");
    MHH_REQUIRE(h->dtype == g->dtype, "the handle was made for the other dtype");
#define CALL(TF) [&]{ auto* S = static_cast<Source<TF>*>(h); \
        if (S->g.icells != g->icells || S->g.jcells != g->jcells || S->g.kcells != g->kcells || S->g.igc != g->igc || S->g.jgc != g->jgc || S->g.kgc != g->kgc) \
        { set_error("mhh_source_exec: the handle was made for another grid"); return (int)MHH_EINVAL; } \
        for (const auto& s : S->src) if (!f->st[s.scalar]) { set_error("mhh_source_exec: scalar %d has no tendency field", s.scalar); return (int)MHH_EINVAL; } \
        return S->exec(f, as_stream(stream)); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// enforce_exponential_decay (src/decay.cxx:35-51) of Decay::exec (:97-111) for every decaying scalar in ONE launch:
// rate = 1./max(timescale, dt) is a double quotient of the narrowed operands, narrowed
MHH_API int mhh_decay_exec(const mhh_grid* g, const mhh_fields* f, const mhh_decay_params* p, double dt_sub, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(f && p, "null pointer");
    for (int n=0; n<MHH_MAX_SCALARS; ++n)
        if (p->exponential[n] && (n >= f->nscalars || !f->s[n] || !f->st[n])) { set_error("mhh_decay_exec: scalar %d decays but has no field", n); return MHH_EINVAL; }
#define CALL(TF) [&]{ DecayOp<TF> op{}; \
        for (int n=0; n<MHH_MAX_SCALARS; ++n) if (p->exponential[n]) \
        { op.st[op.n] = mp<TF>(f->st[n]); op.s[op.n] = cp<TF>(f->s[n]); op.rate[op.n] = TF(1./std::max(TF(p->timescale[n]), TF(dt_sub))); ++op.n; } \
        if (!op.n) return (int)MHH_OK; \
        return launch_interior(as_stream(stream), make_grid<TF>(g), g->kstart, g->kend, op); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// Decay::get_mask("couvreux"), first half (src/decay.cxx:142-157): sums [2][kcells] doubles = the sums of s and of s*s over this
// rank's interior of every level, deterministic; scratch: mhh_decay_couvreux_scratch_elems(g) doubles. A slab sums `sums` over its
// ranks before the second half, as master.sum does.
MHH_API unsigned long long mhh_decay_couvreux_scratch_elems(const mhh_grid* g)
{
    if (!g) return 0;
    return 2ull * (unsigned long long)g->kcells * (unsigned long long)level_chunks(g);
}
MHH_API int mhh_decay_couvreux_sums(const mhh_grid* g, const void* s, void* scratch, void* sums, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(s && scratch && sums, "null pointer");
    const Tiling t = level_tiling(g, g->kmax);
    LevelRanges R{}; R.rows = 2; R.k0[0] = g->kstart; R.nk[0] = g->kmax;
#define CALL(TF) [&]{ hipLaunchKernelGGL(couvreux_partial_kernel<TF>, dim3(tiling_blocks(t)), dim3(BX, BY, 1), 0, as_stream(stream), cp<TF>(s), level_domain(g), t, \
                                         g->kstart, static_cast<double*>(scratch), g->kcells, level_chunks(g)); \
                      MHH_LAUNCH_CHECK(); return (int)MHH_OK; }()
    if (int e = MHH_DISPATCH(g, CALL)) return e;
#undef CALL
    return level_sums_launch(g, static_cast<const double*>(scratch), static_cast<double*>(sums), 2, R, as_stream(stream));
}
// Second half (:158-173): out = s - mean - nstd*std on the interior, zero elsewhere (the reference's tmp field holds what it held);
// outh = interpolate_2nd of it to the half levels k >= 1. What set_mask_thres(name, out, outh, 0, Plus) then reads.
MHH_API int mhh_decay_couvreux_field(const mhh_grid* g, const void* s, const void* sums, double nstd, void* out, void* outh, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(s && sums && out && outh && out != outh, "null pointer");
    const double n = double(g->itot) * double(g->jtot);
#define CALL(TF) [&]{ MHH_HIP_TRY(hipMemsetAsync(out, 0, (size_t)g->ncells*sizeof(TF), as_stream(stream))); \
        MHH_HIP_TRY(hipMemsetAsync(outh, 0, (size_t)g->ncells*sizeof(TF), as_stream(stream))); \
        if (int e = launch_interior(as_stream(stream), make_grid<TF>(g), g->kstart, g->kend, \
                                    CouvreuxOp<TF>{mp<TF>(out), cp<TF>(s), static_cast<const double*>(sums), TF(nstd), n, g->kcells})) return e; \
        return launch_interior(as_stream(stream), make_grid<TF>(g), 0, g->kcells, CouvreuxHalfOp<TF>{mp<TF>(outh), cp<TF>(out), g->ijcells}); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
