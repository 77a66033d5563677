// k_march_common.h -- what the k-marching kernels (k_march.hip, k_march4.hip, k_visc.hip) share: 64 x NJ column tiles that
// walk up in k over chunks of kc levels, dealt to the 8 XCDs so that tiles sharing halos run next to each other on one L2;
// the host helpers of their launchers; their internal entry points (k_rhs.hip and k_stencil.hip call them).
#pragma once
#include <cstdint>
#include <type_traits>
#include "k_common.h"
#include <gfx950_prims.h>

namespace mhh
{
// The rows of a marching launch: [j0, j1), optionally a second range [j2, j3) in the same launch (the two edge strips of a
// slab); the default, j0 < 0, is the whole interior
struct MarchRows
{
    int j0 = -1, j1 = -1, j2 = -1, j3 = -1;
    bool whole() const { return j0 < 0; }
    bool second() const { return j2 >= 0 && j3 > j2; }
    int count() const { return (j1 - j0) + (second() ? j3 - j2 : 0); }     // not for the whole interior
};
// The operators of a marching launch: both (the fused pass), advection only, diffusion only
enum MarchOps { MARCH_BOTH = 0, MARCH_ADVEC = 1, MARCH_DIFF = 2 };

// rows [jbase, jlim) are worked, in tiles from jbase; optionally a SECOND range [jbase2, jlim2) in the same launch (the two edge
// strips of a slab once its north-south halos have arrived: one launch instead of two): tile rows by >= nby1 belong to it
struct MarchTiling { int nbx, nby, nkc, sr, ns, kc, jbase, jlim, nby1, jbase2, jlim2; };
__device__ __forceinline__ void march_tile_rows(const MarchTiling& t, int by, int NJ, int& j0, int& jlim)
{
    if (by < t.nby1) { j0 = t.jbase + by*NJ; jlim = t.jlim; }
    else             { j0 = t.jbase2 + (by - t.nby1)*NJ; jlim = t.jlim2; }
}

__device__ __forceinline__ bool decode_march(const MarchTiling& t, unsigned L, int& bx, int& by, int& kc)
{
    // XCD-aware order as decode_tile (k_common.h): a unit = one strip of tiles over one k-chunk; units are dealt to the
    // XCDs round-robin, so the tiles that share halos run next to each other on one L2.
    const int xcd = L & 7u;
    const unsigned tt = L >> 3;
    const unsigned per_unit = (unsigned)t.sr * t.nbx;
    const unsigned round = tt / per_unit;
    unsigned r = tt - round * per_unit;
    const int unit = (int)round * 8 + xcd;
    if (unit >= t.ns * t.nkc) return false;
    const int strip = unit % t.ns;
    kc = unit / t.ns;
    const int byl = (int)(r / t.nbx);
    bx = (int)(r - (unsigned)byl * t.nbx);
    by = strip * t.sr + byl;
    return by < t.nby;
}

// strips of sr tile rows; (strip, k-chunk) units are dealt round-robin to the XCDs; sr shrinks on thin slabs so that all
// 8 XCDs get work
// tw = cells of a row per tile (a wave's 64 lanes times the cells per lane)
inline MarchTiling make_march_tiling(const mhh_grid* g, int NJ, int kc, int tw = 64, const MarchRows& rows = MarchRows{})
{
    MarchTiling t;
    t.jbase = rows.whole() ? g->jstart : rows.j0; t.jlim = rows.whole() ? g->jend : rows.j1;
    t.nbx = (g->imax + tw-1)/tw; t.nby1 = (t.jlim - t.jbase + NJ-1)/NJ; t.nby = t.nby1;
    t.jbase2 = t.jlim2 = t.jlim;
    if (rows.second()) { t.jbase2 = rows.j2; t.jlim2 = rows.j3; t.nby += (rows.j3 - rows.j2 + NJ-1)/NJ; }
    t.kc = kc; t.nkc = (g->kmax + t.kc - 1)/t.kc;
    t.sr = (MHH_STRIP_ROWS + NJ-1)/NJ;
    if (t.sr * 8 > t.nby * t.nkc) t.sr = (t.nby * t.nkc) / 8;
    if (t.sr < 1) t.sr = 1;
    t.ns = (t.nby + t.sr-1)/t.sr;
    return t;
}
inline unsigned march_blocks(const MarchTiling& t)
{
    const int units = t.ns * t.nkc;
    return 8u * (unsigned)((units + 7)/8) * (unsigned)t.sr * t.nbx;
}
// Levels per k-chunk: kc, or 16 on a strip of a few rows (the slab driver's edge rows), enough blocks to fill the GPU; the
// environment variable `tune` (>= 8) overrides both in tuning runs
inline int march_kc(const mhh_grid* g, const MarchRows& rows, int kc, const char* tune)
{
    if (!rows.whole() && rows.count() * 4 <= g->jmax) kc = 16;
    if (const char* e = getenv(tune)) if (atoi(e) >= 8) kc = atoi(e);
    return kc;
}
inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
// The east-edge rule of a tile copied in 16-byte pieces (vec cells each) whose origin lies `off` cells west of istart (the
// tiles of a row are whole pieces apart, rows are whole pieces: icells % vec == 0). A piece that would run past the end of
// the row is moved west onto the row's last piece (the fused 2i5 kernel's clamp) or left out (TileCopy): the LDS cells it
// covers do not hold their own values. With the origin on a piece no piece straddles the end of a row, and the pieces past
// it are read by inactive lanes only (igc >= reach). With the origin r cells past a piece the straddling piece starts at
// icells - vec + r, and the last cell an active lane reads, iend - 1 + reach, must lie west of it.
inline bool pieces16_clear_of_row_end(const mhh_grid* g, int off, int reach, int vec)
{
    if (g->icells % vec != 0) return false;
    const int r = (((g->istart - off) % vec) + vec) % vec;     // (off > istart: the first piece of a row starts in the row before it)
    return r == 0 ? (g->igc >= reach) : (g->iend - 1 + reach < g->icells - vec + r);
}
// Diagnostics (mhh_stat_march_form): the copy form of the last launch of each marching kernel. pb = bytes per LDS-DMA piece;
// hx = cells the tile of the fields starts west of the block's first cell; ex = the same for the evisc tile (0: the kernel has
// none); cw = cells per lane
enum MarchKernelId { MARCH_K_RHS25 = 0, MARCH_K_SCALARS = 1, MARCH_K_RHS44 = 2, MARCH_K_VISC = 3, MARCH_K_SCALARS4 = 4, MARCH_K_COUNT = 5 };
void note_march_form(MarchKernelId kernel, int pb, int hx, int ex, int cw);
// Calls fn(PB, ADV, DIF) with the run-time operators and piece size (4 or 16 bytes) as std::integral_constants: the template
// arguments of a marching kernel
template<class Fn> void march_variant(MarchOps ops, int pb, Fn&& fn)
{
    using std::true_type; using std::false_type;
    auto pieces = [&](auto adv, auto dif) {
        if (pb == 16) fn(std::integral_constant<int, 16>{}, adv, dif);
        else          fn(std::integral_constant<int, 4>{}, adv, dif);
    };
    if (ops == MARCH_BOTH)       pieces(true_type{}, true_type{});
    else if (ops == MARCH_ADVEC) pieces(true_type{}, false_type{});
    else                         pieces(false_type{}, true_type{});
}

// LDS-DMA copy of one TI x TJ tile of a plane (origin gi0, gj0 in grid cells) into an LDS slot, in pieces of PB bytes per
// lane: PB = 16 (global_load_lds_dwordx4; rows and origin 16-byte aligned) or PB = 4 (global_load_lds_dword; any layout,
// four times the instructions). Piece e = tid + n*NT covers words [tw, tw+PW) of tile row tj; lanes whose piece falls
// outside the tile or the array sit out. lds_dma16 / lds_dma4 come from <gfx950_prims.h> (included by the kernels).
template<class TF, int PB, int TI, int TJ, int NT>
struct TileCopy
{
    static constexpr int EW = (int)sizeof(TF) / 4, PW = PB / 4;
    static constexpr int PPR = TI*EW / PW, NP = PPR*TJ, NLD = (NP + NT - 1) / NT;
    static_assert(PB == 4 || PB == 16, "piece size");
    static_assert((TI*EW) % PW == 0, "tile row must be a whole number of pieces");
    // SV: scalar-base + lane-offset form of the raw copy (see gfx950_prims.h); -DMHH_DMA_NO_SV: the 64-bit-address form (fp64) / builtin (fp32)
#ifdef MHH_DMA_NO_SV
    static constexpr bool SV = false;
#else
    static constexpr bool SV = (MHH_RAW_DMA != 0);
#endif
    int off[NLD]; bool ok[NLD]; int wave_e0; unsigned wave_lds;
    __device__ __forceinline__ void init(int tid, int gi0, int gj0, int icells, int jcells)
    {
        wave_e0 = tid & ~63;
        wave_lds = uniform_u32((unsigned)(wave_e0*PW*4));       // byte offset of this wave's lanes within a slot, as a scalar
#pragma unroll
        for (int n=0; n<NLD; ++n)
        {
            const int e = tid + n*NT;
            const int tj = e / PPR, tw = (e - tj*PPR)*PW;
            const int gw = gi0*EW + tw, gj = gj0 + tj;
            ok[n] = (e < NP) && (gw >= 0) && (gw + PW <= icells*EW) && (gj >= 0) && (gj < jcells);
            off[n] = ok[n] ? gw + gj*icells*EW : 0;
        }
    }
    __device__ __forceinline__ void copy(const TF* __restrict__ plane, TF* __restrict__ lds) const
    {
        const uint32_t* __restrict__ pl = reinterpret_cast<const uint32_t*>(plane);
        uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(lds);
#pragma unroll
        for (int n=0; n<NLD; ++n)
            if (ok[n])
            {
                if constexpr (SV)       lds_dma_sv<PB>(plane, (unsigned)off[n]*4u, lds_address(lds) + (wave_lds + (unsigned)(n*NT*PW*4)));
                else if constexpr (PB == 16) lds_dma16<(sizeof(TF) == 8)>(pl + off[n], dst + (size_t)(wave_e0 + n*NT)*PW);
                else                    lds_dma4<(sizeof(TF) == 8)>(pl + off[n], dst + (size_t)(wave_e0 + n*NT)*PW);
            }
    }
};

// ---- internal entry points (inputs validated by the caller); each returns MHH_OK or an error code ---------------------------
// advec_2i5 and / or diff_smag2 of u, v, w and scalar 0 (if f->nscalars >= 1) in the fused marching kernel (k_march.hip)
int march25(const mhh_grid* g, const mhh_fields* f, const mhh_diff_params* p, MarchOps ops, const MarchRows& rows, void* stream);
// the same for the scalars idx[0 .. n) in the batched scalar pass (k_march.hip)
int march25_scalars(const mhh_grid* g, const mhh_fields* f, const mhh_diff_params* p, const int* idx, int n, MarchOps ops, const MarchRows& rows, void* stream);
// advec_4 and / or diff_4 of u, v, w (k_march4.hip), where march44_takes(g)
int march44(const mhh_grid* g, const mhh_fields* f, MarchOps ops, void* stream, const void* bfold = nullptr);
// the same for the scalars idx[0 .. n) in the batched 4th-order scalar pass (k_march4.hip), where march44_takes(g)
int march44_scalars(const mhh_grid* g, const mhh_fields* f, const int* idx, int n, MarchOps ops, void* stream);
// every scalar of f through that pass (inputs validated by the caller)
inline int march44_all_scalars(const mhh_grid* g, const mhh_fields* f, MarchOps ops, void* stream)
{
    int idx[MHH_MAX_SCALARS];
    for (int n=0; n<f->nscalars; ++n) idx[n] = n;
    return march44_scalars(g, f, idx, f->nscalars, ops, stream);
}
// Diff_smag2::exec_viscosity over the rows (k_visc.hip), where visc_march_takes(g)
int visc_march(const mhh_grid* g, const mhh_fields* f, const mhh_diff_params* p, const void* th, const MarchRows& rows, void* stream);
// The advec_2i5 / diff_smag2 routing of every field (k_rhs.hip): u, v, w and scalar 0 to march25, further scalars to the
// scalar pass (pass) or their own kernels
int route25(const mhh_grid* g, const mhh_fields* f, const mhh_diff_params* p, MarchOps ops, const MarchRows& rows, bool pass, void* stream);

// Does the marching form take the call? The A/B switches (read per call) and the ghost cells the kernels read; otherwise the
// caller takes the one-thread-per-cell kernels. The scalars that the fused kernel does not carry (advec_2i5 / diff_smag2: scalars
// 1, 2, ...) take the scalar pass unless MHH_SCALAR_IMPL=cell; every scalar of advec_4 / diff_4 takes the per-field kernels unless
// MHH_SCALAR_IMPL=march, which selects the 4th-order scalar pass where march44_takes.
inline bool march44_takes(const mhh_grid* g) { return !env_is("MHH_RHS44_IMPL", "cell") && g->igc >= 3 && g->jgc >= 3 && g->kgc >= 3; }
inline bool visc_march_takes(const mhh_grid* g) { return !env_is("MHH_VISC_IMPL", "cell") && g->igc >= 1 && g->jgc >= 1 && g->kgc >= 1; }
inline bool scalar_march_on() { return !env_is("MHH_SCALAR_IMPL", "cell"); }
// The 4th-order scalar pass is opt-in, MHH_SCALAR_IMPL=march: it has the per-field kernels' bits, but no timing on the device shows
// it the faster form yet (profiles/scalar4_pass.md says which runs decide that), so the per-field kernels stay the default there.
inline bool scalar4_march_on() { return env_is("MHH_SCALAR_IMPL", "march"); }
}
