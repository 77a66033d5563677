// microphys_nsw6.h -- Microphys_nsw6 (src/microphys_nsw6.cxx: the single-moment six-class ice scheme of Tomita 2008 with the
// Stevens & Seifert 2008 sedimentation of rain, snow and graupel). Kernels and C-ABI entry points; included from k_stencil.hip. The
// per-cell arithmetic is in cell_ops.h (nsw6_*). Everything is column-local: no LDS, no neighbour in i or j, any row length.
//
// Microphys_nsw6::exec (:983-1073) in two kernels:
//   conversion (:125-650): one thread per cell through the generic cell kernel, a block on one level. Five fields read (seven with
//      ql and qi given), five tendencies read-modify-written; a cell without condensate returns before it touches a tendency. Every
//      std::tgamma of the file and D_d are evaluated on the host (Nsw6Tab, in the kernel's argument block); the powers of the three
//      slope parameters have two forms (NSW6_POW / NSW6_SQRT, cell_ops.h).
//   sedimentation_ss08 (:686-825) of the three species in ONE launch, a species per blockIdx.z: one thread per column walking DOWN from
//      kend-1. The CFL number and the minmod slope of a level depend on its own neighbours only, so the thread computes them on the
//      way (w_qc of three levels in registers), stores them to the species' two scratch arrays and reads back those of the levels
//      ABOVE in the gather: its own earlier stores. w_qc and flux_qc never reach memory; the flux above stays in a register.
#pragma once
#include "k_march_common.h"
#include "thermo_moist.h"
#include "microphys_2mom_warm.h"
#include <gfx950_prims.h>
#include <wave_reduce.h>

namespace mhh
{
template<class TF>
struct Nsw6Args
{
    const TF* q[3]; const TF* thl; const TF* qt; const TF* ql; const TF* qi;
    TF* qct[3]; TF* thlt; TF* qtt; TF* bot[3];
    const TF* rho; const TF* p; const TF* exn; const TF* dz; const TF* dzi;
    TF* c_qc[3]; TF* s_qc[3]; int* nonconv;
    Nsw6Tab<TF> H; double dt; int mask;
    int icells, ijcells, istart, iend, jstart, jend, kstart, kend;
};

// ---- conversion: SAT runs sat_adjust inline for ql and qi (get_thermo_field("ql"), ("qi"): sat_adjust(..).ql and .qi) ------------
template<int FORM, bool SAT, class TF>
struct Nsw6ConvOp
{
    Nsw6Args<TF> A;
    __device__ void operator()(int, int, int k, int c) const
    {
        const TF qr = A.q[0][c], qs = A.q[1][c], qg = A.q[2][c], thl = A.thl[c], qt = A.qt[c];
        const TF p = uniform_load(A.p, k), exn = uniform_load(A.exn, k);
        TF ql, qi;
        if (SAT)
        {
            const MoistSat<TF> s = moist_sat_adjust(thl, qt, p, exn);
            moist_count(A.nonconv, s.niter);
            ql = s.ql; qi = s.qi;
        }
        else
        {
            ql = A.ql[c]; qi = A.qi[c];
        }
        if (nsw6_idle(ql, qi, qr, qs, qg))
            return;
        const Nsw6Level<TF> L = nsw6_level(A.H, uniform_load(A.rho, A.kstart), uniform_load(A.rho, k), p, exn);
        Nsw6Tend<TF> t = {A.qct[0][c], A.qct[1][c], A.qct[2][c], A.qtt[c], A.thlt[c]};
        nsw6_conversion<FORM>(t, A.H, L, qr, qs, qg, qt, thl, ql, qi);
        A.qct[0][c] = t.qrt; A.qct[1][c] = t.qst; A.qct[2][c] = t.qgt; A.qtt[c] = t.qtt; A.thlt[c] = t.thlt;
    }
};

// ---- sedimentation_ss08 of species S, one column -----------------------------------------------------------------------------------
// w_qc[kstart-1] = w_qc[kstart] and w_qc[kend] = 0 (:738-745); the slopes read the ghost levels as the caller left them; the update of
// cc reads dzi of the level ABOVE the one just summed (dzi[kend] on the last turn, :796); dt is a double (:754, :800-801).
template<int FORM, int S, class TF>
__device__ __forceinline__ void nsw6_sedi_column(const Nsw6Args<TF>& A, int col)
{
    const int kk = A.ijcells;
    const TF* __restrict__ q = A.q[S];
    TF* c_qc = A.c_qc[S]; TF* s_qc = A.s_qc[S];          // stored and read back by this thread: not __restrict__
    TF* __restrict__ qct = A.qct[S];
    const TF rho_bot = A.rho[A.kstart];
    int k = A.kend-1;
    int c = col + k*kk;
    TF q_up = q[c+kk], q_c = q[c];
    TF w_up = TF(0.), w_c = nsw6_w_sedi<FORM, S>(A.H, q_c, A.rho[k], TF(std::sqrt(rho_bot/A.rho[k])));
    TF f_up = TF(0.), f = TF(0.);                          // the flux at kend is zero (:769-774)
    for (; k>A.kstart-1; --k)
    {
        const TF rho = A.rho[k], dz = A.dz[k], dzi = A.dzi[k];
        const TF q_dn = q[c-kk];
        const TF w_dn = (k > A.kstart) ? nsw6_w_sedi<FORM, S>(A.H, q_dn, A.rho[k-1], TF(std::sqrt(rho_bot/A.rho[k-1]))) : w_c;
        const TF cfl = TF(TF(0.25) * (w_dn + TF(2.)*w_c + w_up) * dzi * A.dt);
        const TF slope = micro_minmod(q_c-q_dn, q_up-q_c);
        c_qc[c] = cfl; s_qc[c] = slope;
        // the gather (:784-797): the first level from registers, the levels above from this thread's own stores
        int kc = k;
        TF ftot = TF(0.), dzz = TF(0.);
        TF cc = tmin(TF(1.), cfl);
        TF qv = q_c, sv = slope, cv = cfl;
        while (cc > 0 && kc < A.kend)
        {
            ftot += A.rho[kc] * (qv + TF(0.5) * sv * (TF(1.)-cc)) * cc * A.dz[kc];
            dzz += A.dz[kc];
            kc += 1;
            cc = tmin(TF(1.), cv - dzz*A.dzi[kc]);
            if (kc < A.kend)
            {
                const int ckk = col + kc*kk;
                qv = q[ckk]; sv = s_qc[ckk]; cv = c_qc[ckk];
            }
        }
        ftot = tmin(ftot, rho * dz * q_c - f_up * TF(A.dt));
        f = TF(-ftot / A.dt);
        qct[c] += -(f_up - f) / rho * dzi;
        f_up = f;
        q_up = q_c; q_c = q_dn; w_up = w_c; w_c = w_dn;
        c -= kk;
    }
    A.bot[S][col] = -f;
}
constexpr int NSW6_NJ = 4;
template<int FORM, class TF>
__global__ void __launch_bounds__(64*NSW6_NJ) nsw6_sedi_kernel(const Nsw6Args<TF> A)
{
    const int i = A.istart + (int)blockIdx.x*64 + (int)threadIdx.x, j = A.jstart + (int)blockIdx.y*NSW6_NJ + (int)threadIdx.y;
    if (i >= A.iend || j >= A.jend) return;
    const int col = i + j*A.icells;
    const int s = (int)blockIdx.z;                         // wave-uniform
    if (!(A.mask & (NSW6_SEDI_R << s))) return;
    if (s == 0)      nsw6_sedi_column<FORM, 0>(A, col);
    else if (s == 1) nsw6_sedi_column<FORM, 1>(A, col);
    else             nsw6_sedi_column<FORM, 2>(A, col);
}

template<int FORM, class TF>
static int nsw6_exec_form(const mhh_grid* g, const Nsw6Args<TF>& A, hipStream_t st)
{
    if (A.mask & NSW6_CONV)
    {
        const GridDev<TF> gd = make_grid<TF>(g);
        if (A.ql) { Nsw6ConvOp<FORM, false, TF> op{A}; if (int e = launch_interior(st, gd, g->kstart, g->kend, op)) return e; }
        else      { Nsw6ConvOp<FORM, true, TF>  op{A}; if (int e = launch_interior(st, gd, g->kstart, g->kend, op)) return e; }
    }
    if (A.mask & (NSW6_SEDI_R | NSW6_SEDI_S | NSW6_SEDI_G))
    {
        hipLaunchKernelGGL((nsw6_sedi_kernel<FORM, TF>), dim3((g->imax + 63)/64, (g->jmax + NSW6_NJ-1)/NSW6_NJ, 3), dim3(64, NSW6_NJ, 1), 0, st, A);
        MHH_LAUNCH_CHECK();
    }
    return MHH_OK;
}
template<class TF>
static int nsw6_exec(const mhh_grid* g, int impl, const mhh_micro_params* P, const void* qr, const void* qs, const void* qg, const void* thl, const void* qt,
                     const void* ql, const void* qi, void* qrt, void* qst, void* qgt, void* thlt, void* qtt, void* rr_bot, void* rs_bot, void* rg_bot,
                     const void* rhoref, const void* pref, const void* exnref, void* const* scratch, int* nonconv, hipStream_t st)
{
    Nsw6Args<TF> A;
    A.q[0] = cp<TF>(qr); A.q[1] = cp<TF>(qs); A.q[2] = cp<TF>(qg); A.thl = cp<TF>(thl); A.qt = cp<TF>(qt); A.ql = cp<TF>(ql); A.qi = cp<TF>(qi);
    A.qct[0] = mp<TF>(qrt); A.qct[1] = mp<TF>(qst); A.qct[2] = mp<TF>(qgt); A.thlt = mp<TF>(thlt); A.qtt = mp<TF>(qtt);
    A.bot[0] = mp<TF>(rr_bot); A.bot[1] = mp<TF>(rs_bot); A.bot[2] = mp<TF>(rg_bot);
    A.rho = cp<TF>(rhoref); A.p = cp<TF>(pref); A.exn = cp<TF>(exnref); A.dz = cp<TF>(g->dz); A.dzi = cp<TF>(g->dzi);
    for (int s=0; s<3; ++s)
    {
        const bool on = P->processes & (NSW6_SEDI_R << s);
        A.c_qc[s] = on ? mp<TF>(scratch[2*s]) : nullptr; A.s_qc[s] = on ? mp<TF>(scratch[2*s+1]) : nullptr;
    }
    A.nonconv = nonconv;
    A.H = nsw6_tab<TF>(P->Nc0, P->dt); A.dt = P->dt; A.mask = P->processes;
    A.icells = g->icells; A.ijcells = g->ijcells; A.istart = g->istart; A.iend = g->iend; A.jstart = g->jstart; A.jend = g->jend;
    A.kstart = g->kstart; A.kend = g->kend;
    return impl == NSW6_POW ? nsw6_exec_form<NSW6_POW, TF>(g, A, st) : nsw6_exec_form<NSW6_SQRT, TF>(g, A, st);
}

// ---- the largest of the three calc_cfl_ss08 (:829-901, :1119-1177): w_qc of three levels in registers, walking up ----------------
template<int FORM, int S, class TF>
__device__ __forceinline__ TF nsw6_cfl_column(const Nsw6Tab<TF>& H, const TF* __restrict__ q, const TF* __restrict__ rho, const TF* __restrict__ dzi,
                                              double dt, int c, int k0, int k1, int kk)
{
    TF m = TF(0.);
    const TF rho_bot = rho[k0];
    TF wc = nsw6_w_sedi<FORM, S>(H, q[c], rho[k0], TF(std::sqrt(rho_bot/rho[k0]))), wm = wc;
    for (int k=k0; k<k1; ++k)
    {
        const TF wp = (k+1 < k1) ? nsw6_w_sedi<FORM, S>(H, q[c+kk], rho[k+1], TF(std::sqrt(rho_bot/rho[k+1]))) : TF(0.);
        m = tmax(TF(TF(0.25) * (wm + TF(2.)*wc + wp) * dzi[k] * dt), m);
        wm = wc; wc = wp;
        c += kk;
    }
    return m;
}
template<int FORM, class TF>
__global__ void __launch_bounds__(BX*BY) nsw6_cfl_kernel(const Nsw6Tab<TF> H, const TF* __restrict__ qr, const TF* __restrict__ qs, const TF* __restrict__ qg,
                                                         const TF* __restrict__ rho, const TF* __restrict__ dzi, double dt,
                                                         typename Bits<TF>::U* __restrict__ out, int i0, int i1, int j0, int j1, int k0, int k1, int jj, int kk)
{
    const int i = i0 + (int)blockIdx.x*BX + (int)threadIdx.x;
    const int j = j0 + (int)blockIdx.y*BY + (int)threadIdx.y;
    TF m = TF(0);
    if (i < i1 && j < j1)
    {
        const int c = i + j*jj + k0*kk;
        m = nsw6_cfl_column<FORM, 0>(H, qr, rho, dzi, dt, c, k0, k1, kk);
        m = tmax(m, nsw6_cfl_column<FORM, 1>(H, qs, rho, dzi, dt, c, k0, k1, kk));
        m = tmax(m, nsw6_cfl_column<FORM, 2>(H, qg, rho, dzi, dt, c, k0, k1, kk));
    }
    block_max_publish<TF, BY>(m, out);
}
template<class TF>
static int nsw6_cfl(const mhh_grid* g, int impl, const void* qr, const void* qs, const void* qg, const void* rhoref, double dt, void* work, double* out,
                    hipStream_t st)
{
    using U = typename Bits<TF>::U;
    MHH_HIP_TRY(hipMemsetAsync(work, 0, sizeof(unsigned long long), st));
    const Nsw6Tab<TF> H = nsw6_tab<TF>(1., dt);            // the velocity needs the gamma values only
    const dim3 grid((g->imax + BX-1)/BX, (g->jmax + BY-1)/BY, 1), block(BX, BY);
    if (impl == NSW6_POW)
        hipLaunchKernelGGL((nsw6_cfl_kernel<NSW6_POW, TF>), grid, block, 0, st, H, cp<TF>(qr), cp<TF>(qs), cp<TF>(qg), cp<TF>(rhoref), cp<TF>(g->dzi), dt,
                           static_cast<U*>(work), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells);
    else
        hipLaunchKernelGGL((nsw6_cfl_kernel<NSW6_SQRT, TF>), grid, block, 0, st, H, cp<TF>(qr), cp<TF>(qs), cp<TF>(qg), cp<TF>(rhoref), cp<TF>(g->dzi), dt,
                           static_cast<U*>(work), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells);
    MHH_LAUNCH_CHECK();
    TF h = 0;
    MHH_HIP_TRY(hipMemcpyAsync(&h, work, sizeof(TF), hipMemcpyDeviceToHost, st));
    MHH_HIP_TRY(hipStreamSynchronize(st));
    *out = std::max(static_cast<double>(h), 1.e-5);        // :1174, a double
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

MHH_API int mhh_micro_nsw6_exec_impl(const mhh_grid* g, int impl, const mhh_micro_params* params, const void* qr, const void* qs, const void* qg,
                                     const void* thl, const void* qt, const void* ql, const void* qi, void* qrt, void* qst, void* qgt, void* thlt, void* qtt,
                                     void* rr_bot, void* rs_bot, void* rg_bot, const void* rhoref, const void* pref, const void* exnref,
                                     void* const* scratch, int* nonconv, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(impl == MHH_NSW6_POW || impl == MHH_NSW6_SQRT, "impl: MHH_NSW6_POW or MHH_NSW6_SQRT");
    MHH_REQUIRE(params != nullptr, "null params");
    const int m = params->processes;
    MHH_REQUIRE((m & ~NSW6_ALL) == 0, "processes: a mask of MHH_NSW6_CONV, MHH_NSW6_SEDI_R, MHH_NSW6_SEDI_S, MHH_NSW6_SEDI_G");
    MHH_REQUIRE(qr && qs && qg && qrt && qst && qgt && rhoref, "null field");
    MHH_REQUIRE(!(m & NSW6_CONV) || (thl && qt && thlt && qtt && pref && exnref), "conversion needs thl, qt, thlt, qtt, pref, exnref");
    MHH_REQUIRE(!(m & NSW6_CONV) || ((ql == nullptr) == (qi == nullptr)), "ql and qi: both given or both null (null: sat_adjust inline)");
    MHH_REQUIRE(!(m & NSW6_CONV) || params->Nc0 > 0., "Nc0");
    MHH_REQUIRE(params->dt > 0., "dt > 0");
    for (int s=0; s<3; ++s)
        MHH_REQUIRE(!(m & (NSW6_SEDI_R << s)) || (scratch && scratch[2*s] && scratch[2*s+1] && (s == 0 ? rr_bot : s == 1 ? rs_bot : rg_bot)),
                    "sedimentation of a species needs its two scratch arrays (scratch[2s], scratch[2s+1]) and its surface rate");
    MHH_REQUIRE(g->dz && g->dzi, "the grid's metric arrays");
    MHH_REQUIRE(g->kgc >= 1, "one vertical ghost cell");
    if (m == 0) return MHH_OK;
#define CALL(TF) nsw6_exec<TF>(g, impl, params, qr, qs, qg, thl, qt, ql, qi, qrt, qst, qgt, thlt, qtt, rr_bot, rs_bot, rg_bot, rhoref, pref, exnref, scratch, \
                               nonconv, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_micro_nsw6_exec(const mhh_grid* g, const mhh_micro_params* params, const void* qr, const void* qs, const void* qg, const void* thl,
                                const void* qt, const void* ql, const void* qi, void* qrt, void* qst, void* qgt, void* thlt, void* qtt, void* rr_bot,
                                void* rs_bot, void* rg_bot, const void* rhoref, const void* pref, const void* exnref, void* const* scratch, int* nonconv,
                                void* stream)
{
    return mhh_micro_nsw6_exec_impl(g, MHH_NSW6_IMPL_DEFAULT, params, qr, qs, qg, thl, qt, ql, qi, qrt, qst, qgt, thlt, qtt, rr_bot, rs_bot, rg_bot, rhoref,
                                    pref, exnref, scratch, nonconv, stream);
}

MHH_API int mhh_micro_nsw6_cfl_impl(const mhh_grid* g, int impl, const void* qr, const void* qs, const void* qg, const void* rhoref, double dt, void* work,
                                    double* out, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(impl == MHH_NSW6_POW || impl == MHH_NSW6_SQRT, "impl: MHH_NSW6_POW or MHH_NSW6_SQRT");
    MHH_REQUIRE(qr && qs && qg && rhoref, "null field");
    MHH_REQUIRE(work && out, "null work/out");
    MHH_REQUIRE(g->dzi, "the grid's metric arrays");
#define CALL(TF) nsw6_cfl<TF>(g, impl, qr, qs, qg, rhoref, dt, work, out, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
MHH_API int mhh_micro_nsw6_cfl(const mhh_grid* g, const void* qr, const void* qs, const void* qg, const void* rhoref, double dt, void* work, double* out,
                               void* stream)
{
    return mhh_micro_nsw6_cfl_impl(g, MHH_NSW6_IMPL_DEFAULT, qr, qs, qg, rhoref, dt, work, out, stream);
}
