// k_march4.hip -- advec_4 + diff_4 for u, v, w in ONE pass as a k-marching LDS kernel, and for the scalars in a second one (src/advec_4.cxx:88-486,
// src/diff_4.cxx:41-173), the 4th-order sibling of k_march.hip.
//
// The one-thread-per-cell form (Rhs44Op, k_rhs.hip) issues 175 vector loads per cell and is bound by the L1/TA pipe
// (3.3 ms at 512x256x256 fp64 for 72 B/cell of algorithmic traffic). Here a 64 x NJ block walks up in k with the planes
// that are read with horizontal offsets in LDS (halo 3): u, v at k-2..k+1 (the w equation interpolates them vertically
// at x / y offsets), w at k-1..k+2 (the u and v equations interpolate it horizontally at four levels); the 7-level
// column of each thread's own u, v, w sits in registers. The arithmetic is the view-generic code of cell_ops.h
// (advec4_mom_v, diff4_v), i.e. literally the expressions of the cell kernel: same bits.
//
// LDS budget: u and v keep exactly their four planes -- the w equation, the only reader of the oldest one, is computed
// first, then a barrier, then the copy of plane k+2 is issued into that slot and lands while the u and v equations are
// computed; w has a fifth slot for its copy. 13 planes of 70 x (NJ+6) doubles = 72.8 KB: two blocks per CU.
//
// The scalars of fields.st take a second kernel of this file, rhs44_scalar_march_kernel (below): the same skeleton for a batch of
// scalars, one LDS plane per scalar and level, the velocities at the faces from registers.
//
// BUOY: Thermo_buoy's flat 4th-order buoyancy (src/thermo_buoy.cxx:167-184) folded in as the first term of wt. b is read at no
// horizontal offset, so it needs no LDS: a per-lane register window of the own column at k-2 .. k+1, one load per level.
#include <cstdint>
#include "k_common.h"
#include "k_march_common.h"
#include <gfx950_prims.h>

using namespace mhh;

#ifdef MHH_FMA_BUILD     // the named FMA build (build.py): its kernels carry their own name in profiler output
#define rhs44_march_kernel rhs44_march_fma_kernel
#define rhs44_scalar_march_kernel rhs44_scalar_march_fma_kernel
#endif

namespace
{
template<class TF> struct March4Fields
{
    const TF* __restrict__ u; const TF* __restrict__ v; const TF* __restrict__ w;
    TF* __restrict__ ut; TF* __restrict__ vt; TF* __restrict__ wt;
    TF visc;
    const TF* __restrict__ b;        // the buoyancy scalar of the BUOY instantiation
};

// field view of the marching kernel: horizontal offsets from the LDS plane of that level, the own column from registers
template<class TF, int TI> struct MarchView
{
    const TF* pl[5];                 // plane pointers (already at this thread's cell) for level offsets -2..+2
    const TF (&win)[7];              // own column, level offsets -3..+3
    template<int DI, int DJ, int DK> __device__ __forceinline__ TF at() const
    {
        if constexpr (DI == 0 && DJ == 0) return win[3+DK];
        else return pl[DK+2][DI + DJ*TI];
    }
};

template<class TF> __device__ __forceinline__ void shift7(TF (&w)[7], TF nw)
{
    w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4]; w[4] = w[5]; w[5] = w[6]; w[6] = nw;
}

#ifndef MHH_MARCH4_OCC
#define MHH_MARCH4_OCC 2
#endif
#ifndef MHH_MARCH4_KC
#define MHH_MARCH4_KC 64
#endif

// ADV / DIF: both operators (the fused pass) or one of them (Advec_4::exec / Diff_4::exec called separately: same body, same bits)
template<class TF, int NJ, int PB, bool ADV = true, bool DIF = true, bool BUOY = false>
__global__ void __launch_bounds__(64*NJ, MHH_MARCH4_OCC) rhs44_march_kernel(const GridDev<TF> g, const March4Fields<TF> f, const MarchTiling mt)
{
    constexpr int AL = (PB == 16) ? 16 / (int)sizeof(TF) : 1;
    constexpr int TI = ((70 + AL-1)/AL)*AL, TJ = NJ + 6, NT = 64*NJ, NTILE = TI*TJ;
    constexpr int RUV = 4, RW = 5;
    __shared__ __attribute__((aligned(16))) TF U[RUV][NTILE];
    __shared__ __attribute__((aligned(16))) TF V[RUV][NTILE];
    __shared__ __attribute__((aligned(16))) TF W[RW][NTILE];

    int bx, by, kcn;
    if (!decode_march(mt, blockIdx.x, bx, by, kcn)) return;
    const int jj = g.icells, kk = g.ijcells;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty*64 + tx;
    const int i0 = g.istart + bx*64, j0 = g.jstart + by*NJ;
    const int kb = g.kstart + kcn*mt.kc;
    const int ke = (kb + mt.kc < g.kend) ? kb + mt.kc : g.kend;
    const int i = i0 + tx, j = j0 + ty;
    const bool active = (i < g.iend) && (j < g.jend);
    const int ci = (i < g.iend) ? i : g.iend-1, cj = (j < g.jend) ? j : g.jend-1;
    const int col = ci + cj*jj;
    const int l = (ty+3)*TI + (tx+3);
    auto su = [](int p) { return (p + 16) % RUV; };
    auto sw = [](int p) { return (p + 20) % RW; };

    TileCopy<TF, PB, TI, TJ, NT> tc;
    tc.init(tid, i0 - 3, j0 - 3, g.icells, g.jcells);
    auto dma_tile = [&](const TF* __restrict__ fld, int kp, TF* __restrict__ lds)
    {
        if (kp < 0 || kp >= g.kcells) return;                         // wave-uniform
        tc.copy(fld + (size_t)kp*kk, lds);
    };
    auto colval = [&](const TF* __restrict__ fld, int kp) -> TF { return (kp >= 0 && kp < g.kcells) ? fld[col + kp*kk] : TF(0); };

    // ---- prologue: u, v planes kb-2..kb+1, w planes kb-1..kb+2, windows centred on kb ---------------------------------
    for (int p = kb-2; p <= kb+1; ++p) { dma_tile(f.u, p, U[su(p)]); dma_tile(f.v, p, V[su(p)]); }
    for (int p = kb-1; p <= kb+2; ++p) dma_tile(f.w, p, W[sw(p)]);
    TF uw[7], vw[7], ww[7];
#pragma unroll
    for (int n=0; n<7; ++n) { uw[n] = colval(f.u, kb-3+n); vw[n] = colval(f.v, kb-3+n); ww[n] = colval(f.w, kb-3+n); }
    TF bw[4] = {0, 0, 0, 0};                                          // BUOY: b at k-2 .. k+1 of the own column
    if constexpr (BUOY)
    {
#pragma unroll
        for (int n=0; n<4; ++n) bw[n] = colval(f.b, kb-2+n);
    }
    // The tendencies are read one level ahead of their use (MHH_MARCH4_TPREF=0: where they are used); those of the first
    // level here, ahead of the prologue's wait, so that no load is pending when the loop is entered.
#ifndef MHH_MARCH4_TPREF
#define MHH_MARCH4_TPREF 1
#endif
    constexpr bool TPREF = (MHH_MARCH4_TPREF != 0);
    TF tnu = 0, tnv = 0, tnw = 0;
    if (TPREF && active && kb < ke) { const int c0 = col + kb*kk; tnu = stream_load(f.ut + c0); tnv = stream_load(f.vt + c0); tnw = stream_load(f.wt + c0); }
    wait_vmem();
    __syncthreads();

    const TF dxi = g.dxi_t, dyi = g.dyi_t;
    const bool dim3 = g.dim3;
    auto both = [&](TF t, const TF ad[3], const TF df[3]) -> TF
    {
        if constexpr (ADV) { t -= ad[0]; if (dim3) t -= ad[1]; t -= ad[2]; }
        if constexpr (DIF) { t += df[0]; if (dim3) t += df[1]; t += df[2]; }
        return t;
    };

    // the u and v results of level k are stored at the top of iteration k+1: the s_waitcnt vmcnt(0) in front of the
    // end-of-level barrier also waits for stores, and stores issued right before it would expose their latency
    TF ut_pending = 0, vt_pending = 0; int c_pending = -1;
    // vertical face products of the advection and inner vertical gradients of the diffusion, carried to the next level
    // (cell_ops.h, advec4_mom_vc / diff4_vc; MHH_MARCH4_CARRY=0: every level forms all four, as the cell kernels do)
#ifndef MHH_MARCH4_CARRY
#define MHH_MARCH4_CARRY 1
#endif
    constexpr bool CARRY = (MHH_MARCH4_CARRY != 0);
    TF au[3] = {0, 0, 0}, av[3] = {0, 0, 0}, aw[3] = {0, 0, 0}, du[3] = {0, 0, 0}, dv[3] = {0, 0, 0}, dw[3] = {0, 0, 0};
    const int kw0 = (kb > g.kstart) ? kb : g.kstart + 1;            // the first level of this chunk with a w equation
    for (int k = kb; k < ke; ++k)
    {
        const bool fresh = !CARRY || (k == kb), fresh_w = !CARRY || (k == kw0);
        const bool more = (k + 1 < ke);
        if (more) dma_tile(f.w, k+3, W[sw(k+3)]);
        if (c_pending >= 0) { stream_store(f.ut + c_pending, ut_pending); stream_store(f.vt + c_pending, vt_pending); c_pending = -1; }
        const TF tcu = tnu, tcv = tnv, tcw = tnw;
        if (TPREF && more && active) { const int cn = col + (k+1)*kk; tnu = stream_load(f.ut + cn); tnv = stream_load(f.vt + cn); tnw = stream_load(f.wt + cn); }
        const TF nu = more ? colval(f.u, k+4) : TF(0), nv = more ? colval(f.v, k+4) : TF(0), nw = more ? colval(f.w, k+4) : TF(0);
        TF nb = TF(0);
        if constexpr (BUOY) nb = more ? colval(f.b, k+2) : TF(0);

        const MarchView<TF, TI> Uv{{U[su(k-2)]+l, U[su(k-1)]+l, U[su(k)]+l, U[su(k+1)]+l, nullptr}, uw};
        const MarchView<TF, TI> Vv{{V[su(k-2)]+l, V[su(k-1)]+l, V[su(k)]+l, V[su(k+1)]+l, nullptr}, vw};
        const MarchView<TF, TI> Wv{{nullptr, W[sw(k-1)]+l, W[sw(k)]+l, W[sw(k+1)]+l, W[sw(k+2)]+l}, ww};
        const bool bot = (k == g.kstart), top = (k == g.kend-1);
        const int c = col + k*kk;
        TF ad[3], df[3];

        // ---- w equation first: the only reader of the u, v planes k-2 ---------------------------------------------------
        if (active && k > g.kstart)
        {
            const bool botw = (k == g.kstart+1);
            const TF gw4[4] = {uniform_load(g.dzi4, k-2), uniform_load(g.dzi4, k-1), uniform_load(g.dzi4, k), uniform_load(g.dzi4, k+1)};
            if constexpr (ADV) advec4_mom_vc<2>(ad, Wv, Uv, Vv, Wv, botw, top, dxi, dyi, uniform_load(g.dzhi4, k), dim3, aw, fresh_w);
            if constexpr (DIF) diff4_vc(df, Wv, botw, top, f.visc, g.dxidxi_t, g.dyidyi_t, gw4, uniform_load(g.dzhi4, k), dim3, dw, fresh_w);
            TF t = TPREF ? tcw : stream_load(f.wt + c);
            if constexpr (BUOY) t += buoy_w4(bw);                    // wt += interp4c(b[k-2], b[k-1], b[k], b[k+1]) first
            stream_store(f.wt + c, both(t, ad, df));
        }
        if (more)
        {
            __syncthreads();                                          // everyone is done with the u, v planes k-2
            dma_tile(f.u, k+2, U[su(k+2)]); dma_tile(f.v, k+2, V[su(k+2)]);
        }
        // ---- u and v equations (planes k of u, v; k-1..k+2 of w) --------------------------------------------------------
        if (active)
        {
            const TF gc4[4] = {uniform_load(g.dzhi4, k-1), uniform_load(g.dzhi4, k), uniform_load(g.dzhi4, k+1), uniform_load(g.dzhi4, k+2)};
            if constexpr (ADV) advec4_mom_vc<0>(ad, Uv, Uv, Vv, Wv, bot, top, dxi, dyi, uniform_load(g.dzi4, k), dim3, au, fresh);
            if constexpr (DIF) diff4_vc(df, Uv, bot, top, f.visc, g.dxidxi_d, g.dyidyi_d, gc4, uniform_load(g.dzi4, k), dim3, du, fresh);
            ut_pending = both(TPREF ? tcu : stream_load(f.ut + c), ad, df);
            if constexpr (ADV) advec4_mom_vc<1>(ad, Vv, Uv, Vv, Wv, bot, top, dxi, dyi, uniform_load(g.dzi4, k), dim3, av, fresh);
            if constexpr (DIF) diff4_vc(df, Vv, bot, top, f.visc, g.dxidxi_d, g.dyidyi_d, gc4, uniform_load(g.dzi4, k), dim3, dv, fresh);
            vt_pending = both(TPREF ? tcv : stream_load(f.vt + c), ad, df);
            c_pending = c;
        }
        wait_vmem();                  // unconditional: every path back to the loop head carries a vmcnt(0) the compiler can see
        __syncthreads();
        if (more) { shift7(uw, nu); shift7(vw, nv); shift7(ww, nw); }
        if constexpr (BUOY) if (more) { bw[0] = bw[1]; bw[1] = bw[2]; bw[2] = bw[3]; bw[3] = nb; }
    }
    if (c_pending >= 0) { stream_store(f.ut + c_pending, ut_pending); stream_store(f.vt + c_pending, vt_pending); }
}

#ifndef MHH_MARCH4_NJ
#define MHH_MARCH4_NJ 4
#endif
template<class TF>
int march4_launch(const mhh_grid* g, const mhh_fields* f, int pb, MarchOps ops, const void* bfold, hipStream_t st)
{
    constexpr int NJ = MHH_MARCH4_NJ;
    March4Fields<TF> mf;
    mf.u = cp<TF>(f->u); mf.v = cp<TF>(f->v); mf.w = cp<TF>(f->w);
    mf.ut = mp<TF>(f->ut); mf.vt = mp<TF>(f->vt); mf.wt = mp<TF>(f->wt); mf.visc = TF(f->visc); mf.b = cp<TF>(bfold);
    const MarchTiling t = make_march_tiling(g, NJ, MHH_MARCH4_KC);
    const dim3 nb(march_blocks(t)), bs(64, NJ);
    const GridDev<TF> gd = make_grid<TF>(g);
    if (bfold)              // the fused pass only (ops == MARCH_BOTH, checked by the caller)
    {
        if (pb == 16) hipLaunchKernelGGL((rhs44_march_kernel<TF, NJ, 16, true, true, true>), nb, bs, 0, st, gd, mf, t);
        else          hipLaunchKernelGGL((rhs44_march_kernel<TF, NJ, 4, true, true, true>),  nb, bs, 0, st, gd, mf, t);
    }
    else march_variant(ops, pb, [&](auto PB, auto A, auto D) { hipLaunchKernelGGL((rhs44_march_kernel<TF, NJ, PB, A, D>), nb, bs, 0, st, gd, mf, t); });
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
static unsigned long long g_rhs44_march_launches = 0;

// ---- The scalar pass: advec_4 and / or diff_4 of a BATCH of scalars in one k-march (src/advec_4.cxx:360-486, src/diff_4.cxx:41-110) ----
// Opt-in, MHH_SCALAR_IMPL=march (k_march_common.h: scalar4_march_on). The kernel above takes u, v, w; a scalar takes by default
// two one-thread-per-cell launches (mhh_advec_s, mhh_diff_c), which fetch
// every neighbour through L1 and pass over st twice. Here a 64 x NJ block walks up a column tile as above, and per level
//   * each scalar of the batch has the plane of level k with its +-3 halo in LDS, a ring of two slots: the copy of plane k+1 lands
//     under the arithmetic of level k, one barrier per level; the own column k-3 .. k+3 sits in a 7-level register window;
//   * the velocities are read at the faces without interpolation, once per level for the whole batch: u at i-1 .. i+2 and v at
//     j-1 .. j+2 of level k in registers, loaded a level ahead; w of the own column at k-1 .. k+2 in a 4-level register window.
//     The diffusion-only instantiation reads no velocity;
//   * the vertical face products w * ci4(s) and the inner vertical gradients of diff_4 are carried to the next level
//     (cell_ops.h: advec4_s_vc, diff4_vc), formed afresh on a thread's first level of a chunk (the only level of a chunk whose
//     lowest term can be the biased wall form).
// The accumulation into st is Rhs44Op's (k_rhs.hip): the three decrements of the advection, then the three increments of the
// diffusion with the scalar's own svisc: the bits of the per-field kernels and of the oracle.
// How far "a level ahead" reaches: the wait in front of the end-of-level barrier is a full wait_vmem(), so the loads issued at
// the top of level k (the next tendency, the next column values, the next face velocities) overlap the arithmetic of level k
// only; none is still in flight during level k+1. The kernel above has the same limit. It is what a short grid with few blocks
// (the 2-D shape) feels most: one level's memory latency per level of the chain, hidden only by the other blocks of the CU.
template<class TF, int NB> struct Scalar4Fields
{
    const TF* __restrict__ u; const TF* __restrict__ v; const TF* __restrict__ w;
    const TF* s[NB]; TF* st[NB]; TF svisc[NB];
    int ns;                                      // scalars of this launch (<= NB)
};
// horizontal offsets from the LDS plane of level k, the own column from the register window
template<class TF, int TI> struct PlaneView
{
    const TF* pl;                    // the plane of level k, at this thread's cell
    const TF (&win)[7];              // own column, level offsets -3..+3
    template<int DI, int DJ, int DK> __device__ __forceinline__ TF at() const
    {
        static_assert(DK == 0 || (DI == 0 && DJ == 0), "the scalar pass holds one plane per scalar");
        if constexpr (DI == 0 && DJ == 0) return win[3+DK];
        else return pl[DI + DJ*TI];
    }
};
// a velocity along its own axis (0: x, 1: y, 2: z) at offsets -1 .. +2, from registers
template<class TF, int AXIS> struct FaceView
{
    const TF (&a)[4];
    template<int DI, int DJ, int DK> __device__ __forceinline__ TF at() const
    {
        constexpr int D = (AXIS == 0) ? DI : (AXIS == 1) ? DJ : DK;
        static_assert(DI*(AXIS != 0) == 0 && DJ*(AXIS != 1) == 0 && DK*(AXIS != 2) == 0 && D >= -1 && D <= 2, "face velocities: -1 .. +2 along the own axis");
        return a[D+1];
    }
};
#ifndef MHH_SCALAR4_NB
#define MHH_SCALAR4_NB 2
#endif
#ifndef MHH_SCALAR4_KC
#define MHH_SCALAR4_KC 64
#endif

template<class TF, int NJ, int NB, int PB, bool ADV, bool DIF>
__global__ void __launch_bounds__(64*NJ, MHH_MARCH4_OCC) rhs44_scalar_march_kernel(const GridDev<TF> g, const Scalar4Fields<TF, NB> f, const MarchTiling mt)
{
    static_assert(ADV || DIF, "an operator");
    constexpr int AL = (PB == 16) ? 16 / (int)sizeof(TF) : 1;
    constexpr int TI = ((70 + AL-1)/AL)*AL, TJ = NJ + 6, NT = 64*NJ, NTILE = TI*TJ;
    __shared__ __attribute__((aligned(16))) TF S[NB][2][NTILE];

    int bx, by, kcn;
    if (!decode_march(mt, blockIdx.x, bx, by, kcn)) return;        // whole block leaves together: no barrier hazard
    const int jj = g.icells, kk = g.ijcells;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty*64 + tx;
    const int i0 = g.istart + bx*64, j0 = g.jstart + by*NJ;
    const int kb = g.kstart + kcn*mt.kc;
    const int ke = (kb + mt.kc < g.kend) ? kb + mt.kc : g.kend;
    const int i = i0 + tx, j = j0 + ty;
    const bool active = (i < g.iend) && (j < g.jend);
    const int ci = (i < g.iend) ? i : g.iend-1, cj = (j < g.jend) ? j : g.jend-1;   // inactive lanes sit on a valid column
    const int col = ci + cj*jj;
    const int l = (ty+3)*TI + (tx+3);
    const int ns = f.ns;

    TileCopy<TF, PB, TI, TJ, NT> tc;
    tc.init(tid, i0 - 3, j0 - 3, g.icells, g.jcells);
    auto copy_level = [&](int q)                                      // planes kb .. ke-1: always inside the array
    {
#pragma unroll
        for (int n=0; n<NB; ++n) if (n < ns) tc.copy(sgpr(f.s[n] + (size_t)q*kk), S[n][(q - kb) & 1]);   // (pinned: the copy takes its base in scalar registers)
    };
    auto colval = [&](const TF* __restrict__ fld, int kp, int o) -> TF { return (kp >= 0 && kp < g.kcells) ? fld[(size_t)kp*kk + (col + o)] : TF(0); };

    // ---- prologue: plane kb, the windows centred on kb, the velocities and the tendencies of level kb ---------------------
    copy_level(kb);
    TF sw[NB][7], ww[4] = {0, 0, 0, 0}, uf[4] = {0, 0, 0, 0}, vf[4] = {0, 0, 0, 0};
#pragma unroll
    for (int n=0; n<NB; ++n)
#pragma unroll
        for (int m=0; m<7; ++m) sw[n][m] = (n < ns) ? colval(f.s[n], kb-3+m, 0) : TF(0);
    if constexpr (ADV)
    {
#pragma unroll
        for (int m=0; m<4; ++m) { ww[m] = colval(f.w, kb-1+m, 0); uf[m] = colval(f.u, kb, m-1); vf[m] = colval(f.v, kb, (m-1)*jj); }
    }
    TF tn[NB];                                                        // the tendency of the next level, read a level ahead
#pragma unroll
    for (int n=0; n<NB; ++n) tn[n] = (n < ns && active && kb < ke) ? stream_load(f.st[n] + (size_t)kb*kk + col) : TF(0);
    wait_vmem();
    __syncthreads();

    const TF dxi = g.dxi_t, dyi = g.dyi_t;
    const bool dim3 = g.dim3;
    // the results of level k are stored at the top of level k+1: the wait in front of the end-of-level barrier also waits for
    // stores, and stores issued right before it would expose their latency (as the kernel above)
    TF pend[NB]; size_t c_pending = 0; bool pending = false;
    TF ca[NB][3], cd[NB][3];                                          // carried face products and gradients
#pragma unroll
    for (int n=0; n<NB; ++n) { pend[n] = TF(0); for (int m=0; m<3; ++m) { ca[n][m] = TF(0); cd[n][m] = TF(0); } }
    for (int k = kb; k < ke; ++k)
    {
        const bool fresh = (k == kb), more = (k + 1 < ke);
        if (more) copy_level(k+1);                                    // into the slot of plane k-1, retired by the last barrier
        if (pending)
        {
#pragma unroll
            for (int n=0; n<NB; ++n) if (n < ns) stream_store(f.st[n] + c_pending, pend[n]);
            pending = false;
        }
        TF tcur[NB], nsw[NB], nw = TF(0), nuf[4] = {0, 0, 0, 0}, nvf[4] = {0, 0, 0, 0};
#pragma unroll
        for (int n=0; n<NB; ++n)
        {
            tcur[n] = tn[n];
            if (n < ns && more && active) tn[n] = stream_load(f.st[n] + (size_t)(k+1)*kk + col);
            nsw[n] = (n < ns && more) ? colval(f.s[n], k+4, 0) : TF(0);
        }
        if constexpr (ADV)
        {
            if (more)
            {
                nw = colval(f.w, k+3, 0);
#pragma unroll
                for (int m=0; m<4; ++m) { nuf[m] = colval(f.u, k+1, m-1); nvf[m] = colval(f.v, k+1, (m-1)*jj); }
            }
        }
        if (active)
        {
            const bool bot = (k == g.kstart), top = (k == g.kend-1);
            const TF gc4[4] = {uniform_load(g.dzhi4, k-1), uniform_load(g.dzhi4, k), uniform_load(g.dzhi4, k+1), uniform_load(g.dzhi4, k+2)};
            const TF dzi4 = uniform_load(g.dzi4, k);
            const FaceView<TF, 0> Uv{uf}; const FaceView<TF, 1> Vv{vf}; const FaceView<TF, 2> Wv{ww};
#pragma unroll
            for (int n=0; n<NB; ++n)
            {
                if (n < ns)
                {
                    const PlaneView<TF, TI> Sv{S[n][(k - kb) & 1] + l, sw[n]};
                    TF ad[3], df[3], t = tcur[n];
                    if constexpr (ADV)
                    {
                        advec4_s_vc(ad, Sv, Uv, Vv, Wv, bot, top, dxi, dyi, dzi4, dim3, ca[n], fresh);
                        t -= ad[0]; if (dim3) t -= ad[1]; t -= ad[2];
                    }
                    if constexpr (DIF)
                    {
                        diff4_vc(df, Sv, bot, top, f.svisc[n], g.dxidxi_d, g.dyidyi_d, gc4, dzi4, dim3, cd[n], fresh);
                        t += df[0]; if (dim3) t += df[1]; t += df[2];
                    }
                    pend[n] = t;
                }
            }
            c_pending = (size_t)k*kk + col; pending = true;
        }
        wait_vmem();                  // this wave's copies have landed; unconditional, as in the kernel above
        __syncthreads();              // ... everyone's have, and everyone is done with plane k
        if (more)
        {
#pragma unroll
            for (int n=0; n<NB; ++n) shift7(sw[n], nsw[n]);
            if constexpr (ADV)
            {
                ww[0] = ww[1]; ww[1] = ww[2]; ww[2] = ww[3]; ww[3] = nw;
#pragma unroll
                for (int m=0; m<4; ++m) { uf[m] = nuf[m]; vf[m] = nvf[m]; }
            }
        }
    }
    if (pending)
    {
#pragma unroll
        for (int n=0; n<NB; ++n) if (n < ns) stream_store(f.st[n] + c_pending, pend[n]);
    }
}

static unsigned long long g_scalar4_march_launches = 0;

// One launch of the scalar pass over the scalars idx[0 .. ns) (ns <= NB)
template<class TF, int NB>
int scalar4_launch(const mhh_grid* g, const mhh_fields* f, const int* idx, int ns, MarchOps ops, hipStream_t st)
{
    constexpr int NJ = MHH_MARCH4_NJ, VEC = 16 / (int)sizeof(TF);
    Scalar4Fields<TF, NB> sf;
    sf.u = cp<TF>(f->u); sf.v = cp<TF>(f->v); sf.w = cp<TF>(f->w); sf.ns = ns;
    for (int n=0; n<NB; ++n)
    {
        const int m = idx[n < ns ? n : 0];              // slots past ns repeat the first scalar (never read)
        sf.s[n] = cp<TF>(f->s[m]); sf.st[n] = mp<TF>(f->st[m]); sf.svisc[n] = TF(f->svisc[m]);
    }
    // 16-byte pieces need 16-byte aligned rows, arrays and tile origin (i0 - 3 = igc - 3 + 64*bx); other layouts copy in 4-byte
    // pieces. Only the scalars are copied: u, v, w are read per column.
    bool p16 = (g->icells % VEC == 0) && ((g->igc - 3) % VEC == 0) && pieces16_clear_of_row_end(g, 3, 3, VEC);
    for (int n=0; n<ns; ++n) p16 = p16 && al16(f->s[idx[n]]);
    const int pb = p16 ? 16 : 4;
    const MarchTiling t = make_march_tiling(g, NJ, march_kc(g, MarchRows{}, MHH_SCALAR4_KC, "MHH_MARCH_KC_RT"));
    const dim3 nb(march_blocks(t)), bs(64, NJ);
    const GridDev<TF> gd = make_grid<TF>(g);
    note_march_form(MARCH_K_SCALARS4, pb, 3, 0, 1);
    march_variant(ops, pb, [&](auto PB, auto A, auto D) { hipLaunchKernelGGL((rhs44_scalar_march_kernel<TF, NJ, NB, PB, A, D>), nb, bs, 0, st, gd, sf, t); });
    MHH_LAUNCH_CHECK();
    ++g_scalar4_march_launches;
    return MHH_OK;
}
// the scalars idx[0 .. n) in batches of MHH_SCALAR4_NB (MHH_SCALAR_BATCH=1: one per launch)
template<class TF>
int scalar4_batches(const mhh_grid* g, const mhh_fields* f, const int* idx, int n, MarchOps ops, hipStream_t st)
{
    const int nb = env_is("MHH_SCALAR_BATCH", "1") ? 1 : MHH_SCALAR4_NB;
    for (int b = 0; b < n; b += nb)
    {
        const int m = (n - b < nb) ? n - b : nb;
        const int rc = (m == 1) ? scalar4_launch<TF, 1>(g, f, idx + b, 1, ops, st)
                                : scalar4_launch<TF, MHH_SCALAR4_NB>(g, f, idx + b, m, ops, st);
        if (rc) return rc;
    }
    return MHH_OK;
}
} // namespace

MHH_API unsigned long long mhh_stat_rhs44_march_launches(void) { return g_rhs44_march_launches; }
MHH_API unsigned long long mhh_stat_scalar4_march_launches(void) { return g_scalar4_march_launches; }

// advec_4 and / or diff_4 of the scalars idx[0 .. n) in the batched scalar pass, where march44_takes(g)
int mhh::march44_scalars(const mhh_grid* g, const mhh_fields* f, const int* idx, int n, MarchOps ops, void* stream)
{
    if (n <= 0) return MHH_OK;
    if (g->dtype == MHH_F64) return scalar4_batches<double>(g, f, idx, n, ops, as_stream(stream));
    return scalar4_batches<float>(g, f, idx, n, ops, as_stream(stream));
}

// (advec_4, diff_4), Advec_4::exec or Diff_4::exec for u, v, w (the scalars: march44_scalars below); bfold: the buoyancy scalar b
// whose flat Thermo_buoy term is folded into wt (MARCH_BOTH only), or null
int mhh::march44(const mhh_grid* g, const mhh_fields* f, MarchOps ops, void* stream, const void* bfold)
{
    MHH_REQUIRE(!bfold || ops == MARCH_BOTH, "the buoyancy fold belongs to the fused pass");
    const int vec = (g->dtype == MHH_F64) ? 2 : 4;
    // 16-byte pieces need 16-byte aligned rows and tile origin (i0 - 3 = igc - 3 + 64*bx); other layouts copy in 4-byte pieces
    const int pb = (g->icells % vec == 0 && (g->igc - 3) % vec == 0 && al16(f->u) && al16(f->v) && al16(f->w)) ? 16 : 4;
    ++g_rhs44_march_launches;
    note_march_form(MARCH_K_RHS44, pb, 3, 0, 1);
    return (g->dtype == MHH_F64) ? march4_launch<double>(g, f, pb, ops, bfold, as_stream(stream)) : march4_launch<float>(g, f, pb, ops, bfold, as_stream(stream));
}
