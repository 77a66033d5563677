// budget_2.h -- Budget_2<TF>::exec_stats (src/budget_2.cxx) for second-order cases: the kinetic energies and the terms of the u2, v2,
// w2, tke, uw, vw, b2 and bw budgets as masked profiles. One __device__ evaluation function per term group restates the loop bodies
// of the reference statement by statement; a term is never stored: the kernel evaluates it per cell and per mask (the mask-mean
// profiles umodel, vmodel, wmodel are the mask's) and adds it under the FULL-level flag, which is what calc_mask_stats does with a
// tmp field of loc {0,0,0} (src/fields.cxx:805), the half-level terms included. The reduction is that of level_reduce.h, with
// block_sums as the block's order. A level that the loops of a term do not write counts as zero (the tmp field of a first sample).
// pow(x, 2) is x*x and pow(x, 3) is x*x*x, both in double as std::pow(TF, int) returns double: bp2 and bp3 return double, so that the
// products and differences around them promote exactly as the reference's statements do; every store narrows once into TF.
// Kernels and C-ABI entry points; included from k_stencil.hip. stats.h gives stats_fill and stats_check.
#pragma once
#include "level_reduce.h"
#include "stats.h"

namespace mhh
{
constexpr int BNP = 6;                                             // the most profiles of one group
constexpr int BUDGET_NGROUPS = 11;
// profiles per group, in the order of the group bits
__host__ __device__ constexpr int budget_np(int G) { return G == 0 ? 2 : G == 1 ? 5 : G == 2 ? 6 : G == 3 ? 4 : G == 4 ? 4 : G == 5 ? 5 : G == 6 ? 6 : G == 7 ? 4 : G == 8 ? 1 : G == 9 ? 4 : 2; }
constexpr int BG_KE = 0, BG_SHEAR = 1, BG_TURB = 2, BG_COR = 3, BG_PRES = 4, BG_RDSTR = 5, BG_DIFF = 6, BG_BUOY = 7, BG_BWBUOY = 8, BG_ADVS = 9, BG_PRESS = 10;
constexpr int BG_DIFF_UW = 61, BG_DIFF_VW = 62;                    // the LES diffusion group runs as three launches: 4 + 1 + 1 profiles
constexpr int BG_MODEL = 100;                                      // calc_mask_mean_profile of u, v, w: not a group of the descriptor

struct BudgetName { const char* name; int half; };
static const BudgetName budget_names[BUDGET_NGROUPS][BNP] = {
    {{"ke", 0}, {"tke", 0}},
    {{"u2_shear", 0}, {"v2_shear", 0}, {"tke_shear", 0}, {"uw_shear", 1}, {"vw_shear", 1}},
    {{"u2_turb", 0}, {"v2_turb", 0}, {"w2_turb", 1}, {"tke_turb", 0}, {"uw_turb", 1}, {"vw_turb", 1}},
    {{"u2_cor", 0}, {"v2_cor", 0}, {"uw_cor", 1}, {"vw_cor", 1}},
    {{"w2_pres", 1}, {"tke_pres", 0}, {"uw_pres", 1}, {"vw_pres", 1}},
    {{"u2_rdstr", 0}, {"v2_rdstr", 0}, {"w2_rdstr", 1}, {"uw_rdstr", 1}, {"vw_rdstr", 1}},
    {{"u2_diff", 0}, {"v2_diff", 0}, {"w2_diff", 1}, {"tke_diff", 0}, {"uw_diff", 1}, {"vw_diff", 1}},
    {{"w2_buoy", 1}, {"tke_buoy", 0}, {"uw_buoy", 1}, {"vw_buoy", 1}},
    {{"bw_buoy", 1}},
    {{"b2_shear", 0}, {"b2_turb", 0}, {"bw_shear", 1}, {"bw_turb", 1}},
    {{"bw_pres", 1}, {"bw_rdstr", 1}}};

template<class TF> struct BudgetArgs
{
    const TF *u, *v, *w, *p, *evisc, *b, *ufluxbot, *vfluxbot;
    const TF *umodel, *vmodel, *wmodel, *bmean, *pmean;            // [nmasks][kcells] x 3, [kcells] x 2
    const TF *dzi, *dzhi;
    const unsigned int* mfield;
    TF utrans, vtrans, fc, dxi, dyi;
    LevelDomain dom;
    int nmasks, kcells, kstart, kend;
    int p0;                                                        // the group's first profile in part and sums
    int lastrank;                                                  // this rank holds the last rows of the domain (mpicoordy == npy-1)
};

// What a level takes from the profiles, per mask: index 0, 1, 2 is level k-1, k, k+1; a level outside 0 .. kcells-1 (k+1 of the level
// kend where kgc == 1, which no body of the reference reads) holds 0.
template<class TF> struct BudgetLev
{
    TF um[3], vm[3], wm[3], bm[3], pm[3], dzi[3], dzhi[3];
    TF wmp2;                                                       // wmodel[k+2]: wz at level k+1 (the LES diffusion group)
    int k, ks, ke;
};
template<class TF> __device__ __forceinline__ TF budget_at(const TF* p, int base, int k, int kcells) { return (p && k >= 0 && k < kcells) ? uniform_load(p, base + k) : TF(0); }

template<class TF> __device__ __forceinline__ double bp2(TF x) { return double(x)*double(x); }
template<class TF> __device__ __forceinline__ double bp3(TF x) { const double d = double(x); return d*d*d; }
template<class TF> __device__ __forceinline__ TF i22(TF a, TF b, TF c, TF d) { return TF(0.25)*(a + b + c + d); }
// Grid::interpolate_2nd (src/grid.cxx:455-486) of w to the location of u (wxloc = {1,0,1}: iih = -1) and of v (wyloc = {0,1,1}:
// jjh = -jj), the four quarter terms as written, their literals doubles, narrowed once
template<class TF> __device__ __forceinline__ TF budget_wx(const TF* __restrict__ w, size_t c)
{
    return 0.25*(0.5*w[c] + 0.5*w[c-1]) + 0.25*(0.5*w[c] + 0.5*w[c-1]) + 0.25*(0.5*w[c] + 0.5*w[c-1]) + 0.25*(0.5*w[c] + 0.5*w[c-1]);
}
template<class TF> __device__ __forceinline__ TF budget_wy(const TF* __restrict__ w, size_t c, int jj)
{
    return 0.25*(0.5*w[c] + 0.5*w[c]) + 0.25*(0.5*w[c-jj] + 0.5*w[c-jj]) + 0.25*(0.5*w[c] + 0.5*w[c]) + 0.25*(0.5*w[c-jj] + 0.5*w[c-jj]);
}

// calc_kinetic_energy (:51-94): ke, tke on kstart .. kend-1
template<class TF> __device__ __forceinline__ void budget_ke(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w;
    const int ii = 1, jj = A.dom.icells, kk = A.dom.ijcells;
    {
        const TF t = i2(TF(u[c]+A.utrans), TF(u[c+ii]+A.utrans)); const TF u2 = t*t;
        const TF s = i2(TF(v[c]+A.vtrans), TF(v[c+jj]+A.vtrans)); const TF v2 = s*s;
        const TF r = i2(w[c], w[c+kk]); const TF w2 = r*r;
        o[0] = TF(0.5) * (u2 + v2 + w2);
    }
    {
        const TF t = i2(TF(u[c]-L.um[1]), TF(u[c+ii]-L.um[1])); const TF u2 = t*t;
        const TF s = i2(TF(v[c]-L.vm[1]), TF(v[c+jj]-L.vm[1])); const TF v2 = s*s;
        const TF r = i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])); const TF w2 = r*r;
        o[1] = TF(0.5) * (u2 + v2 + w2);
    }
}

// calc_shear_terms (:100-135): u2_shear, v2_shear, tke_shear, uw_shear, vw_shear on kstart .. kend-1
template<class TF> __device__ __forceinline__ void budget_shear(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w;
    const int jj = A.dom.icells, kk = A.dom.ijcells;
    const TF dudz = (i2(L.um[1], L.um[2]) - i2(L.um[0], L.um[1])) * L.dzi[1];
    const TF dvdz = (i2(L.vm[1], L.vm[2]) - i2(L.vm[0], L.vm[1])) * L.dzi[1];
    const TF wx = budget_wx(w, c), wxt = budget_wx(w, c+kk), wy = budget_wy(w, c, jj), wyt = budget_wy(w, c+kk, jj);
    o[0] = TF(-2.) * (u[c]-L.um[1]) * i2(TF(wx-L.wm[1]), TF(wxt-L.wm[2])) * dudz;
    o[1] = TF(-2.) * (v[c]-L.vm[1]) * i2(TF(wy-L.wm[1]), TF(wyt-L.wm[2])) * dvdz;
    o[3] = -bp2(wx) * (L.um[1] - L.um[0]) * L.dzhi[1];
    o[4] = -bp2(wy) * (L.vm[1] - L.vm[0]) * L.dzhi[1];
    o[2] = TF(0.5)*(o[0] + o[1]);
}

// calc_turb_terms (:141-233): u2_turb, v2_turb, tke_turb on kstart .. kend-1; w2_turb, uw_turb, vw_turb with a body at kstart, one
// at kend and the inner one. As written: the inner w2_turb subtracts no mean from w[ijk-kk] (:225); uw_turb and vw_turb at kstart
// pair wx[ijk-kk] with wmean[k+1] (:189, :192).
template<class TF> __device__ __forceinline__ void budget_turb(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w;
    const int jj = A.dom.icells, kk = A.dom.ijcells, k = L.k;
    const TF wx = budget_wx(w, c), wxb = budget_wx(w, c-kk), wy = budget_wy(w, c, jj), wyb = budget_wy(w, c-kk, jj);
    if (k < L.ke)
    {
        const TF wxt = budget_wx(w, c+kk), wyt = budget_wy(w, c+kk, jj);
        o[0] = - ( bp2(i2(TF(u[c]-L.um[1]), TF(u[c+kk]-L.um[2]))) * (wxt-L.wm[2])
                 - bp2(i2(TF(u[c]-L.um[1]), TF(u[c-kk]-L.um[0]))) * (wx -L.wm[1]) ) * L.dzi[1];
        o[1] = - ( bp2(i2(TF(v[c]-L.vm[1]), TF(v[c+kk]-L.vm[2]))) * (wyt-L.wm[2])
                 - bp2(i2(TF(v[c]-L.vm[1]), TF(v[c-kk]-L.vm[0]))) * (wy -L.wm[1]) ) * L.dzi[1];
        o[3] = - TF(0.5) * ( bp3(TF(w[c+kk]-L.wm[2])) - bp3(TF(w[c]-L.wm[1])) ) * L.dzi[1]
               + TF(0.5) * (o[0] + o[1]);
        if (k == L.ks)
        {
            o[2] = - TF(2.) * bp3(i2(w[c], w[c+kk])) * L.dzhi[1];
            o[4] = - ( (u[c]   -L.um[1]) * bp2(i2(TF(wx-L.wm[1]), TF(wxt-L.wm[2])))
                     - (u[c-kk]-L.um[0]) * bp2(i2(TF(wx-L.wm[1]), TF(wxb-L.wm[2]))) ) * L.dzhi[1];
            o[5] = - ( (v[c]   -L.vm[1]) * bp2(i2(TF(wy-L.wm[1]), TF(wyt-L.wm[2])))
                     - (v[c-kk]-L.vm[0]) * bp2(i2(TF(wy-L.wm[1]), TF(wyb-L.wm[2]))) ) * L.dzhi[1];
        }
        else
        {
            o[2] = - ( bp3(i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])))
                     - bp3(i2(TF(w[c]-L.wm[1]), w[c-kk])) ) * L.dzhi[1];
            o[4] = - ( (u[c]   -L.um[1]) * bp2(i2(TF(wx-L.wm[1]), TF(wxt-L.wm[2])))
                     - (u[c-kk]-L.um[0]) * bp2(i2(TF(wx-L.wm[1]), TF(wxb-L.wm[0]))) ) * L.dzhi[1];
            o[5] = - ( (v[c]   -L.vm[1]) * bp2(i2(TF(wy-L.wm[1]), TF(wyt-L.wm[2])))
                     - (v[c-kk]-L.vm[0]) * bp2(i2(TF(wy-L.wm[1]), TF(wyb-L.wm[0]))) ) * L.dzhi[1];
        }
    }
    else
    {
        o[2] = - TF(2.) * bp3(i2(TF(w[c]-L.wm[1]), TF(w[c-kk]-L.wm[0]))) * L.dzhi[1];
        o[4] = - ( (u[c]   -L.um[1]) * bp2(i2(TF(wx-L.wm[1]), TF(wxb-L.wm[0])))
                 - (u[c-kk]-L.um[0]) * bp2(i2(TF(wx-L.wm[1]), TF(wxb-L.wm[0]))) ) * L.dzhi[1];
        o[5] = - ( (v[c]   -L.vm[1]) * bp2(i2(TF(wy-L.wm[1]), TF(wyb-L.wm[0])))
                 - (v[c-kk]-L.vm[0]) * bp2(i2(TF(wy-L.wm[1]), TF(wyb-L.wm[0]))) ) * L.dzhi[1];
    }
}

// calc_coriolis_terms (:239-279): u2_cor, v2_cor on kstart .. kend-1; uw_cor, vw_cor on kstart+1 .. kend-1
template<class TF> __device__ __forceinline__ void budget_cor(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w;
    const int ii = 1, jj = A.dom.icells, kk = A.dom.ijcells;
    const TF fc = A.fc;
    o[0] = TF( 2.) * (u[c]-L.um[1]) * (i22(v[c-ii], v[c], v[c-ii+jj], v[c+jj])-L.vm[1]) * fc;
    o[1] = TF(-2.) * (v[c]-L.vm[1]) * (i22(u[c-jj], u[c], u[c+ii-jj], u[c+ii])-L.um[1]) * fc;
    if (L.k == L.ks) return;
    o[2] = i2(TF(w[c]-L.wm[1]), TF(w[c-ii]-L.wm[1])) *
        i2(i22(TF(v[c   ]-L.vm[1]), TF(v[c-ii   ]-L.vm[1]), TF(v[c-ii-kk   ]-L.vm[0]), TF(v[c-kk   ]-L.vm[0])),
           i22(TF(v[c+jj]-L.vm[1]), TF(v[c-ii+jj]-L.vm[1]), TF(v[c-ii+jj-kk]-L.vm[0]), TF(v[c+jj-kk]-L.vm[0]))) * fc;
    o[3] = i2(TF(w[c]-L.wm[1]), TF(w[c-jj]-L.wm[1])) *
        i2(i22(TF(u[c   ]-L.um[1]), TF(u[c-jj   ]-L.um[1]), TF(u[c-jj-kk   ]-L.um[0]), TF(u[c-kk   ]-L.um[0])),
           i22(TF(u[c+ii]-L.um[1]), TF(u[c+ii-jj]-L.um[1]), TF(u[c+ii-jj-kk]-L.um[0]), TF(u[c+ii-kk]-L.um[0]))) * fc;
}

// calc_pressure_transport_terms (:285-352): tke_pres, uw_pres, vw_pres on kstart .. kend-1 (no top-boundary body); w2_pres with the
// double minus of its kstart body (:333-334) and the inner body on kstart+1 .. kend-1. Order: w2_pres, tke_pres, uw_pres, vw_pres.
template<class TF> __device__ __forceinline__ void budget_pres(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w; const TF* __restrict__ p = A.p;
    const int ii = 1, jj = A.dom.icells, kk = A.dom.ijcells;
    const TF dxi = A.dxi, dyi = A.dyi;
    o[1] = - ( i2(p[c], p[c+kk]) * (w[c+kk] -L.wm[2])-
               i2(p[c], p[c-kk]) * (w[c   ] -L.wm[1])) * L.dzi[1];
    o[2] = - ( i2(p[c   ], p[c-kk   ]) * (w[c   ]-L.wm[1])-
               i2(p[c-ii], p[c-ii-kk]) * (w[c-ii]-L.wm[1]) ) * dxi +
             ( i2(p[c   ], p[c-ii   ]) * (u[c   ]-L.um[1]) -
               i2(p[c-kk], p[c-ii-kk]) * (u[c-kk]-L.um[0]) ) * L.dzhi[1];
    o[3] = - ( i2(p[c-kk   ], p[c   ]) * (w[c   ]-L.wm[1])  -
               i2(p[c-jj-kk], p[c-jj]) * (w[c-jj]-L.wm[1]) ) * dyi +
             ( i2(p[c-jj   ], p[c   ]) * (v[c   ]-L.vm[1]) -
               i2(p[c-jj-kk], p[c-kk]) * (v[c-kk]-L.vm[0]) ) * L.dzhi[1];
    if (L.k == L.ks)
        o[0] = TF(-2.) * ( i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])) * p[c   ] -
                         - i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])) * p[c-kk] ) * L.dzhi[1];
    else
        o[0] = TF(-2.) * ( i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])) * p[c   ] -
                           i2(TF(w[c]-L.wm[1]), TF(w[c-kk]-L.wm[0])) * p[c-kk] ) * L.dzhi[1];
}

// calc_pressure_redistribution_terms (:358-419): u2_rdstr, v2_rdstr, uw_rdstr, vw_rdstr on kstart .. kend-1; w2_rdstr with a body
// at kstart and the inner one. Order: u2_rdstr, v2_rdstr, w2_rdstr, uw_rdstr, vw_rdstr.
template<class TF> __device__ __forceinline__ void budget_rdstr(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w; const TF* __restrict__ p = A.p;
    const int ii = 1, jj = A.dom.icells, kk = A.dom.ijcells;
    const TF dxi = A.dxi, dyi = A.dyi;
    o[0] = TF(2.) * i2(p[c], p[c-ii]) *
        ( i2(TF(u[c]-L.um[1]), TF(u[c+ii]-L.um[1])) -
          i2(TF(u[c]-L.um[1]), TF(u[c-ii]-L.um[1])) ) * dxi;
    o[1] = TF(2.) * i2(p[c], p[c-jj]) *
        ( i2(TF(v[c]-L.vm[1]), TF(v[c+jj]-L.vm[1])) -
          i2(TF(v[c]-L.vm[1]), TF(v[c-jj]-L.vm[1])) ) * dyi;
    o[3] = i22(p[c], p[c-kk], p[c-ii-kk], p[c-ii]) *
         ( ((u[c]-L.um[1]) - (u[c-kk]-L.um[0])) * L.dzhi[1] + (w[c] - w[c-ii]) * dxi );
    o[4] = i22(p[c], p[c-kk], p[c-jj-kk], p[c-jj]) *
         ( ((v[c]-L.vm[1]) - (v[c-kk]-L.vm[0])) * L.dzhi[1] + (w[c] - w[c-jj]) * dyi );
    if (L.k == L.ks)
        o[2] = TF(2.) * i2(p[c], p[c-kk]) * (w[c+kk]-L.wm[2] - (w[c]-L.wm[1])) * L.dzi[1];
    else
        o[2] = TF(2.) * i2(p[c], p[c-kk]) *
            ( i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])) - i2(TF(w[c]-L.wm[1]), TF(w[c-kk]-L.wm[0])) ) * L.dzhi[1];
}

// calc_diffusion_terms_les (:680-1038): u2_diff, v2_diff, w2_diff, tke_diff, uw_diff, vw_diff. The helper fields are evaluated on the
// fly, each one expression rounded once as its store does: wz (:703-723) = interp2(w[k]-wmean[k], w[k+1]-wmean[k+1]) on kstart ..
// kend-1 of ALL columns, mirrored with a minus sign onto kstart-1 and kend; evisch (:727-735) on the INTERIOR columns of kstart ..
// kend-1 only -- its cyclic fill is commented out in the reference (:737), so evisch[ijk+ii] of the last column and evisch[ijk+jj] of
// the last row read an unwritten cell: zero. The last row is the DOMAIN's (the rank with mpicoordy == npy-1): the parity target is the
// single-rank run, so a slab rank evaluates evisch[ijk+jj] of its own last row from evisc's exchanged ghost row and every
// decomposition gives the single rank's profile (the reference under MPI zeroes the last row of every rank). The += chains round into TF at every store. Three loops: all of kstart .. kend-1;
// kstart+1 .. kend-1 (the vertical parts, uw_diff, vw_diff, and the only place tke_diff gains 0.5*(u2_diff + v2_diff) off the
// surface); kstart, which OVERWRITES u2_diff, v2_diff, tke_diff with the surface-flux form.
template<class TF> struct BudgetWz { TF wm0, wm1, wm2, wm3; int k, ks, ke; };      // wmodel[k-1 .. k+2] by value: selected, never indexed
template<class TF> __device__ __forceinline__ TF budget_wz(const TF* __restrict__ w, size_t c, int kk, int dk, const BudgetWz<TF> Z)
{
    const int kl = Z.k + dk;
    const int kv = kl < Z.ks ? Z.ks : (kl > Z.ke-1 ? Z.ke-1 : kl);  // the level whose value the ghost level mirrors
    const int d = kv - Z.k;                                        // -1, 0, 1
    const TF m0 = d < 0 ? Z.wm0 : (d == 0 ? Z.wm1 : Z.wm2);
    const TF m1 = d < 0 ? Z.wm1 : (d == 0 ? Z.wm2 : Z.wm3);
    const size_t cv = c + (long long)d*kk;
    const TF v = i2(TF(w[cv]-m0), TF(w[cv+kk]-m1));
    return kv != kl ? -v : v;
}
template<class TF> __device__ __forceinline__ TF budget_evisch(const TF* __restrict__ e, size_t c, int jj, int kk, bool written)
{
    if (!written) return TF(0);
    const int ii = 1;
    return TF(0.125) * (e[c-ii-jj-kk] + e[c-ii-jj] + e[c-ii-kk] + e[c-ii] +
                        e[c   -jj-kk] + e[c   -jj] + e[c   -kk] + e[c   ]);
}
// PART 0 delivers u2_diff, v2_diff, w2_diff, tke_diff in o[0..3]; 1 uw_diff and 2 vw_diff in o[0]: what a part does not deliver is dead
// code to the compiler. Six outputs times the masks in one kernel spill; a part of its own for uw_diff and for vw_diff does not.
template<class TF, int PART> __device__ __forceinline__ void budget_diff_les(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, int i, int j, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w; const TF* __restrict__ evisc = A.evisc;
    const int ii = 1, ii2 = 2, jj = A.dom.icells, jj2 = 2*A.dom.icells, kk = A.dom.ijcells, kk2 = 2*A.dom.ijcells, k = L.k;
    const TF dxi = A.dxi, dyi = A.dyi;
    const TF umk = L.um[1], vmk = L.vm[1], wmk = L.wm[1];
    const TF dzik = L.dzi[1], dzikm = L.dzi[0], dzhik = L.dzhi[1], dzhikp = L.dzhi[2];
    const BudgetWz<TF> Z{L.wm[0], L.wm[1], L.wm[2], L.wmp2, L.k, L.ks, L.ke};
    TF u2, v2, w2, tke, uw = TF(0), vw = TF(0);
    {
        const TF evisc_utop   = i22(evisc[c], evisc[c+kk], evisc[c-ii+kk], evisc[c-ii]);
        const TF evisc_ubot   = i22(evisc[c], evisc[c-kk], evisc[c-ii-kk], evisc[c-ii]);
        const TF evisc_unorth = i22(evisc[c], evisc[c+jj], evisc[c+jj-ii], evisc[c-ii]);
        const TF evisc_usouth = i22(evisc[c], evisc[c-jj], evisc[c-jj-ii], evisc[c-ii]);

        const TF evisc_vtop   = i22(evisc[c], evisc[c+kk], evisc[c-jj+kk], evisc[c-jj]);
        const TF evisc_vbot   = i22(evisc[c], evisc[c-kk], evisc[c-jj-kk], evisc[c-jj]);
        const TF evisc_veast  = i22(evisc[c], evisc[c+ii], evisc[c+ii-jj], evisc[c-jj]);
        const TF evisc_vwest  = i22(evisc[c], evisc[c-ii], evisc[c-ii-jj], evisc[c-jj]);

        const TF evisc_weast  = i22(evisc[c], evisc[c+ii], evisc[c+ii-kk], evisc[c-kk]);
        const TF evisc_wwest  = i22(evisc[c], evisc[c-ii], evisc[c-ii-kk], evisc[c-kk]);
        const TF evisc_wnorth = i22(evisc[c], evisc[c+jj], evisc[c+jj-kk], evisc[c-kk]);
        const TF evisc_wsouth = i22(evisc[c], evisc[c-jj], evisc[c-jj-kk], evisc[c-kk]);

        const TF wz = budget_wz(w, c, kk, 0, Z);
        const TF wze = budget_wz(w, c+ii, kk, 0, Z), wzw = budget_wz(w, c-ii, kk, 0, Z);
        const TF wzn = budget_wz(w, c+jj, kk, 0, Z), wzs = budget_wz(w, c-jj, kk, 0, Z);

        u2 = TF(2.) * (u[c]-umk) * ( evisc[c   ] * (u[c+ii] - u[c   ]) * dxi -
                                     evisc[c-ii] * (u[c   ] - u[c-ii]) * dxi ) * TF(2.) * dxi;
        u2 += TF(2.) * (u[c]-umk) * ( evisc_unorth * (u[c+jj] - u[c      ]) * dyi -
                                      evisc_usouth * (u[c   ] - u[c-jj   ]) * dyi +
                                      evisc_unorth * (v[c+jj] - v[c+jj-ii]) * dxi -
                                      evisc_usouth * (v[c   ] - v[c-ii   ]) * dxi ) * dyi;
        u2 += TF(2.) * (u[c]-umk) * ( evisc_utop * (w[c+kk] - w[c-ii+kk]) * dxi -
                                      evisc_ubot * (w[c   ] - w[c-ii   ]) * dxi ) * dzik;

        v2 = TF(2.) * (v[c]-vmk) * ( evisc[c   ] * (v[c+jj] - v[c   ]) * dyi -
                                     evisc[c-jj] * (v[c   ] - v[c-jj]) * dyi ) * TF(2.) * dyi;
        v2 += TF(2.) * (v[c]-vmk) * ( evisc_veast * (v[c+ii] - v[c      ]) * dxi -
                                      evisc_vwest * (v[c   ] - v[c-ii   ]) * dxi +
                                      evisc_veast * (u[c+ii] - u[c+ii-jj]) * dyi -
                                      evisc_vwest * (u[c   ] - u[c-jj   ]) * dyi ) * dxi;
        v2 += TF(2.) * (v[c]-vmk) * ( evisc_vtop * (w[c+kk] - w[c-jj+kk]) * dyi -
                                      evisc_vbot * (w[c   ] - w[c-jj   ]) * dyi ) * dzik;

        w2 = TF(2.) * (w[c]-wmk) * ( evisc_weast * (w[c+ii] - w[c   ]) * dxi -
                                     evisc_wwest * (w[c   ] - w[c-ii]) * dxi ) * dxi;
        w2 += TF(2.) * (w[c]-wmk) * ( evisc_wnorth * (w[c+jj] - w[c   ]) * dyi -
                                      evisc_wsouth * (w[c   ] - w[c-jj]) * dyi ) * dyi;

        tke = wz * ( i2(evisc[c], evisc[c+ii]) * (wze - wz ) * dxi -
                     i2(evisc[c], evisc[c-ii]) * (wz  - wzw) * dxi ) * dxi;
        tke += (wz-wmk) * ( i2(evisc[c], evisc[c+ii]) * (i2(u[c+ii], u[c+ii+kk]) - i2(u[c+ii], u[c+ii-kk])) * dzik -
                            i2(evisc[c], evisc[c-ii]) * (i2(u[c   ], u[c   +kk]) - i2(u[c   ], u[c   -kk])) * dzik ) * dxi;
        tke += (wz-wmk) * ( i2(evisc[c], evisc[c+jj]) * (wzn - wz ) * dyi -
                            i2(evisc[c], evisc[c-jj]) * (wz  - wzs) * dyi ) * dyi;
        tke += (wz-wmk) * ( i2(evisc[c], evisc[c+jj]) * (i2(v[c+jj], v[c+jj+kk]) - i2(v[c+jj], v[c+jj-kk])) * dzik -
                            i2(evisc[c], evisc[c-jj]) * (i2(v[c   ], v[c   +kk]) - i2(v[c   ], v[c   -kk])) * dzik ) * dyi;

        if (k > L.ks)
        {
            const TF wzt = budget_wz(w, c, kk, 1, Z), wzb = budget_wz(w, c, kk, -1, Z);
            const TF evisch   = budget_evisch(evisc, c,    jj, kk, true);
            const TF evischn  = budget_evisch(evisc, c+jj, jj, kk, j + 1 < A.dom.jend || !A.lastrank);
            const TF evische  = budget_evisch(evisc, c+ii, jj, kk, i + 1 < A.dom.iend);

            u2 += TF(2.) * (u[c]-umk) * ( evisc_utop * (u[c+kk] - u[c   ]) * dzhikp -
                                          evisc_ubot * (u[c   ] - u[c-kk]) * dzhik  ) * dzik;
            v2 += TF(2.) * (v[c]-vmk) * ( evisc_vtop * (v[c+kk] - v[c   ]) * dzhikp -
                                          evisc_vbot * (v[c   ] - v[c-kk]) * dzhik  ) * dzik;
            w2 += TF(2.) * (w[c]-wmk) * ( evisc_weast * (u[c+ii] - u[c+ii-kk]) * dzhik -
                                          evisc_wwest * (u[c   ] - u[c   -kk]) * dzhik ) * dxi;
            w2 += TF(2.) * (w[c]-wmk) * ( evisc_wnorth * (v[c+jj] - v[c+jj-kk]) * dzhik -
                                          evisc_wsouth * (v[c   ] - v[c   -kk]) * dzhik ) * dyi;
            w2 += TF(2.) * (w[c]-wmk) * ( evisc[c   ] * (w[c+kk] - w[c   ]) * dzik  -
                                          evisc[c-kk] * (w[c   ] - w[c-kk]) * dzikm ) * TF(2.) * dzhik;

            tke += wz * ( i2(evisc[c], evisc[c+kk]) * (wzt - wz ) * dzhikp -
                          i2(evisc[c], evisc[c-kk]) * (wz  - wzb) * dzhik  ) * TF(2.) * dzik
                 + TF(0.5) * (u2 + v2);

            uw = ( ( i2(w[c-ii], w[c    ])
                    * ( ( ( ( TF(2.) * i2(evisc[c    -kk], evisc[c        ]) )
                        * ( i2(u[c+ii-kk], u[c+ii    ]) - i2(u[c    -kk], u[c        ]) ) )
                      * dxi ) - ( ( ( TF(2.) * i2(evisc[c-ii-kk], evisc[c-ii    ]) )
                        * ( i2(u[c    -kk], u[c        ]) - i2(u[c-ii-kk], u[c-ii    ]) ) )
                      * dxi ) ) )
                  * dxi );
            uw += ( ( i2(w[c-ii], w[c    ])
                     * ( ( evischn
                       * ( ( ( i2(u[c+jj-kk], u[c+jj    ]) - i2(u[c    -kk], u[c        ]) )
                           * dyi )
                         + ( ( i2(v[c    +jj-kk], v[c    +jj    ]) - i2(v[c-ii+jj-kk], v[c-ii+jj    ]) )
                           * dxi ) ) ) - ( evisch
                       * ( ( ( i2(u[c    -kk], u[c        ]) - i2(u[c-jj-kk], u[c-jj    ]) )
                           * dyi )
                         + ( ( i2(v[c        -kk], v[c            ]) - i2(v[c-ii    -kk], v[c-ii        ]) )
                           * dxi ) ) ) ) )
                   * dyi );
            uw += ( ( i2(w[c-ii], w[c    ])
                     * ( ( i2(evisc[c-ii    ], evisc[c        ])
                       * ( ( ( i2(u[c    ], u[c+kk]) - i2(u[c-kk], u[c    ]) )
                           * dzik )
                         + ( ( i2(w[c        ], w[c    +kk]) - i2(w[c-ii    ], w[c-ii+kk]) )
                           * dxi ) ) ) - ( i2(evisc[c-ii-kk], evisc[c    -kk])
                       * ( ( ( i2(u[c-kk], u[c    ]) - i2(u[c-kk2], u[c-kk]) )
                           * dzikm )
                         + ( ( i2(w[c    -kk], w[c        ]) - i2(w[c-ii-kk], w[c-ii    ]) )
                           * dxi ) ) ) ) )
                   * dzhik );
            uw += ( ( i2(u[c-kk], u[c    ])
                    * ( ( i2(evisc[c    -kk], evisc[c        ])
                      * ( ( ( i2(w[c    ], w[c+ii]) - i2(w[c-ii], w[c    ]) )
                          * dxi )
                        + ( ( i2(u[c        ], u[c+ii    ]) - i2(u[c    -kk], u[c+ii-kk]) )
                          * dzhik ) ) ) - ( i2(evisc[c-ii-kk], evisc[c-ii    ])
                      * ( ( ( i2(w[c-ii], w[c    ]) - i2(w[c-ii2], w[c-ii]) )
                          * dxi )
                        + ( ( i2(u[c-ii    ], u[c        ]) - i2(u[c-ii-kk], u[c    -kk]) )
                          * dzhik ) ) ) ) )
                  * dxi );
            uw += ( ( i2(u[c-kk], u[c    ])
                    * ( ( evischn
                      * ( ( ( i2(w[c-ii+jj], w[c    +jj]) - i2(w[c-ii    ], w[c        ]) )
                          * dyi )
                        + ( ( i2(v[c-ii+jj    ], v[c    +jj    ]) - i2(v[c-ii+jj-kk], v[c    +jj-kk]) )
                          * dzhik ) ) ) - ( evisch
                      * ( ( ( i2(w[c-ii    ], w[c        ]) - i2(w[c-ii-jj], w[c    -jj]) )
                          * dyi )
                        + ( ( i2(v[c-ii        ], v[c            ]) - i2(v[c-ii    -kk], v[c        -kk]) )
                          * dzhik ) ) ) ) )
                  * dyi );
            uw += ( ( i2(u[c-kk], u[c    ])
                    * ( ( ( 2 * i2(evisc[c-ii    ], evisc[c        ]) )
                      * ( ( i2(w[c-ii+kk], w[c    +kk]) - i2(w[c-ii    ], w[c        ]) )
                        * dzik ) ) - ( ( TF(2.) * i2(evisc[c-ii-kk], evisc[c    -kk]) )
                      * ( ( i2(w[c-ii    ], w[c        ]) - i2(w[c-ii-kk], w[c    -kk]) )
                        * dzikm ) ) ) )
                  * dzhik );

            vw = ( ( i2(w[c-jj], w[c    ])
                  * ( ( evische
                    * ( ( ( i2(v[c+ii-kk], v[c+ii    ]) - i2(v[c    -kk], v[c        ]) )
                        * dxi )
                      + ( ( i2(u[c+ii    -kk], u[c+ii        ]) - i2(u[c+ii-jj-kk], u[c+ii-jj    ]) )
                        * dyi ) ) ) - ( evisch
                    * ( ( ( i2(v[c    -kk], v[c        ]) - i2(v[c-ii-kk], v[c-ii    ]) )
                        * dxi )
                      + ( ( i2(u[c        -kk], u[c            ]) - i2(u[c    -jj-kk], u[c    -jj    ]) )
                        * dyi ) ) ) ) )
                * dxi );
            vw += ( ( i2(w[c-jj], w[c    ])
                  * ( ( ( TF(2.) * i2(evisc[c    -kk], evisc[c        ]) )
                    * ( i2(v[c+jj-kk], v[c+jj    ]) - i2(v[c    -kk], v[c        ]) ) ) - ( ( TF(2.) * i2(evisc[c-jj-kk], evisc[c-jj    ]) )
                    * ( i2(v[c    -kk], v[c        ]) - i2(v[c-jj-kk], v[c-jj    ]) ) ) ) )
                * dyi );
            vw += ( ( i2(w[c-jj], w[c    ])
                  * ( ( i2(evisc[c-jj    ], evisc[c        ])
                    * ( ( ( i2(v[c    ], v[c+kk]) - i2(v[c-kk], v[c    ]) )
                        * dzik )
                      + ( ( i2(w[c        ], w[c    +kk]) - i2(w[c-jj    ], w[c-jj+kk]) )
                        * dyi ) ) ) - ( i2(evisc[c-jj-kk], evisc[c    -kk])
                    * ( ( ( i2(v[c-kk], v[c    ]) - i2(v[c-kk2], v[c-kk]) )
                        * dzikm )
                      + ( ( i2(w[c    -kk], w[c        ]) - i2(w[c-jj-kk], w[c-jj    ]) )
                        * dyi ) ) ) ) )
                * dzhik );
            vw += ( ( i2(v[c-kk], v[c    ])
                  * ( ( evische
                    * ( ( ( i2(w[c+ii-jj], w[c+ii    ]) - i2(w[c    -jj], w[c        ]) )
                        * dxi )
                      + ( ( i2(u[c+ii-jj    ], u[c+ii        ]) - i2(u[c+ii-jj-kk], u[c+ii    -kk]) )
                        * dzhik ) ) ) - ( evisch
                    * ( ( ( i2(w[c    -jj], w[c        ]) - i2(w[c-ii-jj], w[c-ii    ]) )
                        * dxi )
                      + ( ( i2(u[c    -jj    ], u[c            ]) - i2(u[c    -jj-kk], u[c        -kk]) )
                        * dzhik ) ) ) ) )
                * dxi );
            vw += ( ( i2(v[c-kk], v[c    ])
                  * ( ( i2(evisc[c    -kk], evisc[c        ])
                    * ( ( ( i2(w[c    ], w[c+jj]) - i2(w[c-jj], w[c    ]) )
                        * dyi )
                      + ( ( i2(v[c        ], v[c+jj    ]) - i2(v[c    -kk], v[c+jj-kk]) )
                        * dzhik ) ) ) - ( i2(evisc[c-jj-kk], evisc[c-jj    ])
                    * ( ( ( i2(w[c-jj], w[c    ]) - i2(w[c-jj2], w[c-jj]) )
                        * dyi )
                      + ( ( i2(v[c-jj    ], v[c        ]) - i2(v[c-jj-kk], v[c    -kk]) )
                        * dzhik ) ) ) ) )
                * dyi );
            vw += ( ( i2(v[c-kk], v[c    ])
                  * ( ( ( TF(2.) * i2(evisc[c-jj    ], evisc[c        ]) )
                    * ( ( i2(w[c-jj+kk], w[c    +kk]) - i2(w[c-jj    ], w[c        ]) )
                      * dzik ) ) - ( ( TF(2.) * i2(evisc[c-jj-kk], evisc[c    -kk]) )
                    * ( ( i2(w[c-jj    ], w[c        ]) - i2(w[c-jj-kk], w[c    -kk]) )
                      * dzikm ) ) ) )
                * dzhik );
        }
        else
        {
            const size_t ij = c - (size_t)k*kk;
            const TF wzt = budget_wz(w, c, kk, 1, Z);
            u2 = TF(2.) * (u[c]-umk) * ( evisc_utop * (u[c+kk] - u[c   ]) * dzhikp + A.ufluxbot[ij]) * dzik;
            v2 = TF(2.) * (v[c]-vmk) * ( evisc_vtop * (v[c+kk] - v[c   ]) * dzhikp + A.vfluxbot[ij]) * dzik;
            tke = (wz-wmk) * ( i2(evisc[c], evisc[c+kk]) * (wzt - wz ) * dzhikp ) * TF(2.) * dzik
                + TF(0.5) * (u2 + v2);
        }
    }
    if (PART == 0) { o[0] = u2; o[1] = v2; o[2] = w2; o[3] = tke; }
    else if (PART == 1) o[0] = uw;
    else o[0] = vw;
}

// calc_buoyancy_terms (:1044-1090): tke_buoy on kstart .. kend-1; w2_buoy, uw_buoy, vw_buoy on kstart+1 .. kend-1.
// Order: w2_buoy, tke_buoy, uw_buoy, vw_buoy.
template<class TF> __device__ __forceinline__ void budget_buoy(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ u = A.u; const TF* __restrict__ v = A.v; const TF* __restrict__ w = A.w; const TF* __restrict__ b = A.b;
    const int ii = 1, jj = A.dom.icells, kk = A.dom.ijcells;
    o[1] = i2(TF(w[c]-L.wm[1]), TF(w[c+kk]-L.wm[2])) * (b[c] - L.bm[1]);
    if (L.k == L.ks) return;
    o[0] = TF(2.) * i2(TF(b[c]-L.bm[1]), TF(b[c-kk]-L.bm[0])) * (w[c]-L.wm[1]);
    o[2] = i2 (TF(u[c]-L.um[1]), TF(u[c-kk]-L.um[0])) *
           i22(TF(b[c]-L.bm[1]), TF(b[c-ii]-L.bm[1]), TF(b[c-ii-kk]-L.bm[0]), TF(b[c-kk]-L.bm[0]));
    o[3] = i2 (TF(v[c]-L.vm[1]), TF(v[c-kk]-L.vm[0])) *
           i22(TF(b[c]-L.bm[1]), TF(b[c-jj]-L.bm[1]), TF(b[c-jj-kk]-L.bm[0]), TF(b[c-kk]-L.bm[0]));
}

// calc_buoyancy_terms_scalar (:1096-1115) with s = b: bw_buoy on kstart .. kend-1
template<class TF> __device__ __forceinline__ void budget_bwbuoy(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ b = A.b;
    const int kk = A.dom.ijcells;
    o[0] = i2(TF(b[c]-L.bm[1]), TF(b[c-kk]-L.bm[0])) * i2(TF(b[c]-L.bm[1]), TF(b[c-kk]-L.bm[0]));
}

// calc_advection_terms_scalar (:1121-1156) with s = b: b2_shear, b2_turb, bw_shear, bw_turb on kstart .. kend-1; the shear terms
// use w without its mean, as written
template<class TF> __device__ __forceinline__ void budget_advs(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ w = A.w; const TF* __restrict__ s = A.b;
    const int kk = A.dom.ijcells;
    const TF dsdz  = (i2(L.bm[1], L.bm[2]) - i2(L.bm[1], L.bm[0])) * L.dzi[1];
    const TF dsdzh = (L.bm[1] - L.bm[0]) * L.dzhi[1];
    o[0] = - TF(2.) * (s[c] - L.bm[1]) * i2(w[c], w[c+kk]) * dsdz;
    o[1] = - ((bp2(i2(TF(s[c]-L.bm[1]), TF(s[c+kk]-L.bm[2]))) * w[c+kk]) -
              (bp2(i2(TF(s[c]-L.bm[1]), TF(s[c-kk]-L.bm[0]))) * w[c   ])) * L.dzi[1];
    o[2] = - bp2(w[c]) * dsdzh;
    o[3] = - ((bp2(i2(w[c], w[c+kk])) * (s[c   ]-L.bm[1]))-
              (bp2(i2(w[c], w[c-kk])) * (s[c-kk]-L.bm[0]))) * L.dzhi[1];
}

// calc_pressure_terms_scalar (:1257-1279) with s = b: bw_pres, bw_rdstr on kstart .. kend-1
template<class TF> __device__ __forceinline__ void budget_press(const BudgetArgs<TF>& A, const BudgetLev<TF>& L, size_t c, TF (&o)[BNP])
{
    if (L.k >= L.ke) return;
    const TF* __restrict__ s = A.b; const TF* __restrict__ p = A.p;
    const int kk = A.dom.ijcells;
    o[0] = - ((p[c]-L.pm[1]) * (s[c]-L.bm[1]) - (p[c-kk]-L.pm[0]) * (s[c-kk]-L.bm[0])) * L.dzhi[1];
    o[1] = i2(TF(p[c]-L.pm[1]), TF(p[c-kk]-L.pm[0])) * ((s[c]-L.bm[1])-(s[c-kk]-L.bm[0])) * L.dzhi[1];
}

// One group: blockIdx.x is a tile (a level k0 + kz and a chunk of rows). NP x NM double accumulators per thread, indexed statically.
// G == BG_MODEL: Stats::calc_mask_mean_profile (src/stats.cxx:1328-1347), calc_mean of u, v under the full-level flag and of w under
// the half-level flag over ALL levels 0 .. kcells-1.
template<class TF, int G, int NM>
__global__ void __launch_bounds__(LEVEL_THREADS) budget_partial_kernel(const BudgetArgs<TF> A, const Tiling t, double* __restrict__ part, int k0, int nk, int nchunks)
{
    constexpr int NP = (G == BG_MODEL) ? 3 : (G == BG_DIFF) ? 4 : (G == BG_DIFF_UW || G == BG_DIFF_VW) ? 1 : budget_np(G);
    LevelTile T;
    if (!level_tile(t, blockIdx.x, k0, A.dom, T)) return;
    if (T.kz >= nk) return;
    const int k = T.k, kk = A.dom.ijcells;
    const unsigned int* __restrict__ msk = A.mfield + (size_t)k*kk;
    BudgetLev<TF> L[NM];
    double acc[NP][NM];
#pragma unroll
    for (int n=0; n<NM; ++n)
    {
        const int base = (n < A.nmasks ? n : 0)*A.kcells;
        const bool live = (G != BG_MODEL) && n < A.nmasks;
        L[n].k = k; L[n].ks = A.kstart; L[n].ke = A.kend;
#pragma unroll
        for (int d=0; d<3; ++d)
        {
            const int kl = k - 1 + d;
            L[n].um[d] = live ? budget_at(A.umodel, base, kl, A.kcells) : TF(0);
            L[n].vm[d] = live ? budget_at(A.vmodel, base, kl, A.kcells) : TF(0);
            L[n].wm[d] = live ? budget_at(A.wmodel, base, kl, A.kcells) : TF(0);
            L[n].bm[d] = live ? budget_at(A.bmean, 0, kl, A.kcells) : TF(0);
            L[n].pm[d] = live ? budget_at(A.pmean, 0, kl, A.kcells) : TF(0);
            L[n].dzi[d] = live ? budget_at(A.dzi, 0, kl, A.kcells) : TF(0);
            L[n].dzhi[d] = live ? budget_at(A.dzhi, 0, kl, A.kcells) : TF(0);
        }
        L[n].wmp2 = (live && (G == BG_DIFF || G == BG_DIFF_UW || G == BG_DIFF_VW)) ? budget_at(A.wmodel, base, k + 2, A.kcells) : TF(0);
#pragma unroll
        for (int p=0; p<NP; ++p) acc[p][n] = 0.;
    }
    for_chunk_cells(A.dom, T.j0, T.j1, [&](int i, int j, int ij) __attribute__((always_inline))
    {
        const unsigned int m = msk[ij];
        const size_t c = (size_t)ij + (size_t)k*kk;
        if (G == BG_MODEL)
        {
            const double vu = double(A.u[c]), vv = double(A.v[c]), vw = double(A.w[c]);
#pragma unroll
            for (int n=0; n<NM; ++n)
            {
                acc[0][n] += double((m >> (2*n)) & 1u) * vu;
                acc[1][n] += double((m >> (2*n)) & 1u) * vv;
                acc[2 % NP][n] += double((m >> (2*n + 1)) & 1u) * vw;
            }
        }
        else if (G == BG_DIFF_UW || G == BG_DIFF_VW)
        {
            // uw_diff and vw_diff read no mask-mean profile: one evaluation per cell serves every mask
            TF o[BNP];
#pragma unroll
            for (int p=0; p<BNP; ++p) o[p] = TF(0);
            if (G == BG_DIFF_UW) budget_diff_les<TF, 1>(A, L[0], c, i, j, o);
            else                 budget_diff_les<TF, 2>(A, L[0], c, i, j, o);
            const double term = double(o[0]);
#pragma unroll
            for (int n=0; n<NM; ++n)
                if (n < A.nmasks) acc[0][n] += double((m >> (2*n)) & 1u) * term;
        }
        else
        {
#pragma unroll
            for (int n=0; n<NM; ++n)
            {
                if (n >= A.nmasks) continue;                          // block-uniform: a mask that does not exist costs no evaluation
                TF o[BNP];
#pragma unroll
                for (int p=0; p<BNP; ++p) o[p] = TF(0);
                if (G == BG_KE)          budget_ke(A, L[n], c, o);
                else if (G == BG_SHEAR)  budget_shear(A, L[n], c, o);
                else if (G == BG_TURB)   budget_turb(A, L[n], c, o);
                else if (G == BG_COR)    budget_cor(A, L[n], c, o);
                else if (G == BG_PRES)   budget_pres(A, L[n], c, o);
                else if (G == BG_RDSTR)  budget_rdstr(A, L[n], c, o);
                else if (G == BG_DIFF)   budget_diff_les<TF, 0>(A, L[n], c, i, j, o);
                else if (G == BG_BUOY)   budget_buoy(A, L[n], c, o);
                else if (G == BG_BWBUOY) budget_bwbuoy(A, L[n], c, o);
                else if (G == BG_ADVS)   budget_advs(A, L[n], c, o);
                else if (G == BG_PRESS)  budget_press(A, L[n], c, o);
                const double in = double((m >> (2*n)) & 1u);          // in_mask<double>(mask, flag) * fld (calc_mean, :281)
#pragma unroll
                for (int p=0; p<NP; ++p) acc[p][n] += in * double(o[p]);
            }
        }
    });
    const int tid = threadIdx.x + threadIdx.y*BX;
#pragma unroll
    for (int p=0; p<NP; ++p)
    {
        const double sum = block_sums<NM>(acc[p]);
        if (tid < NM && tid < A.nmasks) part[(((size_t)(A.p0 + p)*A.nmasks + tid)*A.kcells + k)*nchunks + T.by] = sum;
    }
}

// A budget profile: calc_mean under the full-level flag over kstart .. kend, then set_fillvalue_prof over all levels
// (calc_mask_stats, src/stats.cxx:1350-1390). model != 0: calc_mask_mean_profile, every level, u and v by nmask and w by nmaskh; a
// level without a cell holds 0 (the reference keeps what the vector held).
template<class TF>
__global__ void __launch_bounds__(256) budget_finish_kernel(const double* __restrict__ sums, const int* __restrict__ nmask, TF* __restrict__ out,
                                                            int nmasks, int kcells, int kstart, int kend, int model)
{
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= kcells) return;
    const int prof = blockIdx.y / nmasks, n = blockIdx.y % nmasks;
    const size_t o = (size_t)blockIdx.y*kcells + k;
    const int cnt = nmask[(n*2 + (model && prof == 2 ? 1 : 0))*kcells + k];
    TF v = TF(0);
    if (cnt != 0 && (model || (k >= kstart && k <= kend))) v = TF(sums[o] / cnt);
    if (cnt == 0 && !model) v = stats_fill<TF>();
    out[o] = v;
}

// Thermo_dry calc_buoyancy (src/thermo_dry.cxx:51-63): b = grav/thref[k] * (th - thref[k]) on all kcells levels of the interior columns
template<class TF> struct BudgetDryBuoyancyOp
{
    TF* b; const TF* th; const TF* thref; TF grav;
    __device__ void operator()(int, int, int k, int c) const { b[c] = grav/thref[k] * (th[c] - thref[k]); }
};

// ---- host side ---------------------------------------------------------------------------------------------
constexpr unsigned int BUDGET_ALL = (1u << BUDGET_NGROUPS) - 1u;
constexpr unsigned int BUDGET_NEEDS_B = (1u << BG_BUOY) | (1u << BG_BWBUOY) | (1u << BG_ADVS) | (1u << BG_PRESS);

static int budget_nprofs(unsigned int groups)
{
    int n = 0;
    for (int G=0; G<BUDGET_NGROUPS; ++G) if (groups & (1u << G)) n += budget_np(G);
    return n;
}

static int budget_check(const mhh_grid* g, int nmasks, const mhh_budget_2_desc* d)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(d != nullptr, "null descriptor");
    if (d->order != 2) { set_error("mhh_budget_2: second-order grids only (Budget_4 is not built)"); return MHH_EINVAL; }
    if (d->groups == 0 || (d->groups & ~BUDGET_ALL)) { set_error("mhh_budget_2: unknown group bit in 0x%x", d->groups); return MHH_EINVAL; }
    if (d->groups & (1u << BG_DIFF))
    {
        if (d->diff_scheme != MHH_DIFF_SMAG2) { set_error("mhh_budget_2: the diffusion group is calc_diffusion_terms_les, for diff_smag2 only (scheme %d; the DNS terms are not built)", d->diff_scheme); return MHH_EINVAL; }
        if (g->igc < 2 || g->jgc < 2) { set_error("mhh_budget_2: the LES diffusion group needs two horizontal ghost cells (set_minimum_ghost_cells(2, 2, 1))"); return MHH_EINVAL; }
        MHH_REQUIRE(d->evisc && d->u_fluxbot && d->v_fluxbot, "the LES diffusion group needs evisc, u_fluxbot and v_fluxbot");
        MHH_REQUIRE(g->kmax >= 2, "at least two levels");
    }
    if ((d->groups & BUDGET_NEEDS_B) && !d->b) { set_error("mhh_budget_2: the buoyancy, b2 and bw groups need b"); return MHH_EINVAL; }
    MHH_REQUIRE(g->igc >= 1 && g->jgc >= 1, "the terms read one horizontal ghost cell");
    return MHH_OK;
}

template<class TF>
static BudgetArgs<TF> budget_args(const mhh_grid* g, const void* mfield, int nmasks, const mhh_budget_2_desc* d)
{
    BudgetArgs<TF> A{};
    if (d)
    {
        A.u = cp<TF>(d->u); A.v = cp<TF>(d->v); A.w = cp<TF>(d->w); A.p = cp<TF>(d->p); A.evisc = cp<TF>(d->evisc); A.b = cp<TF>(d->b);
        A.ufluxbot = cp<TF>(d->u_fluxbot); A.vfluxbot = cp<TF>(d->v_fluxbot);
        A.umodel = cp<TF>(d->umodel); A.vmodel = cp<TF>(d->vmodel); A.wmodel = cp<TF>(d->wmodel); A.bmean = cp<TF>(d->bmean); A.pmean = cp<TF>(d->pmean);
        A.utrans = TF(d->utrans); A.vtrans = TF(d->vtrans); A.fc = TF(d->fc);
    }
    A.dzi = cp<TF>(g->dzi); A.dzhi = cp<TF>(g->dzhi);
    A.mfield = static_cast<const unsigned int*>(mfield);
    { const GridDev<TF> gd = make_grid<TF>(g); A.dxi = gd.dxi_d; A.dyi = gd.dyi_d; }
    A.lastrank = (g->mpicoordy == g->npy - 1);
    A.nmasks = nmasks; A.dom = level_domain(g); A.kcells = g->kcells; A.kstart = g->kstart; A.kend = g->kend;
    return A;
}

template<class TF, int G>
static int budget_group_launch(const BudgetArgs<TF>& A, const mhh_grid* g, int nmasks, double* part, int k0, int nk, hipStream_t st)
{
    const Tiling t = level_tiling(g, nk);
    const dim3 grid(tiling_blocks(t)), block(BX, BY, 1);
    with_mask_width(nmasks, [&](auto nm) { hipLaunchKernelGGL((budget_partial_kernel<TF, G, decltype(nm)::value>), grid, block, 0, st, A, t, part, k0, nk, level_chunks(g)); });
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

template<class TF>
static int budget_sums_launch(const mhh_grid* g, const void* mfield, int nmasks, const mhh_budget_2_desc* d, double* sums, double* scratch, hipStream_t st)
{
    BudgetArgs<TF> A = budget_args<TF>(g, mfield, nmasks, d);
    const int k0 = g->kstart, nk = g->kmax + 1;                    // kstart .. kend inclusive (calc_mean, :271)
    int p0 = 0;
#define MHH_BUDGET_GROUP(G) if (d->groups & (1u << G)) { A.p0 = p0; if (int e = budget_group_launch<TF, G>(A, g, nmasks, scratch, k0, nk, st)) return e; p0 += budget_np(G); }
    MHH_BUDGET_GROUP(BG_KE) MHH_BUDGET_GROUP(BG_SHEAR) MHH_BUDGET_GROUP(BG_TURB) MHH_BUDGET_GROUP(BG_COR) MHH_BUDGET_GROUP(BG_PRES) MHH_BUDGET_GROUP(BG_RDSTR)
    if (d->groups & (1u << BG_DIFF))
    {
        A.p0 = p0;     if (int e = budget_group_launch<TF, BG_DIFF>(A, g, nmasks, scratch, k0, nk, st)) return e;
        A.p0 = p0 + 4; if (int e = budget_group_launch<TF, BG_DIFF_UW>(A, g, nmasks, scratch, k0, nk, st)) return e;
        A.p0 = p0 + 5; if (int e = budget_group_launch<TF, BG_DIFF_VW>(A, g, nmasks, scratch, k0, nk, st)) return e;
        p0 += budget_np(BG_DIFF);
    }
    MHH_BUDGET_GROUP(BG_BUOY) MHH_BUDGET_GROUP(BG_BWBUOY) MHH_BUDGET_GROUP(BG_ADVS) MHH_BUDGET_GROUP(BG_PRESS)
#undef MHH_BUDGET_GROUP
    return level_sums_launch(g, scratch, sums, p0*nmasks, LevelRanges{p0*nmasks, {k0}, {nk}}, st);       // one range for every profile
}

template<class TF>
static int budget_model_sums_launch(const mhh_grid* g, const void* mfield, int nmasks, const void* u, const void* v, const void* w, double* sums, double* scratch, hipStream_t st)
{
    BudgetArgs<TF> A = budget_args<TF>(g, mfield, nmasks, nullptr);
    A.u = cp<TF>(u); A.v = cp<TF>(v); A.w = cp<TF>(w);
    if (int e = budget_group_launch<TF, BG_MODEL>(A, g, nmasks, scratch, 0, g->kcells, st)) return e;
    return level_sums_launch(g, scratch, sums, 3*nmasks, LevelRanges{3*nmasks, {0}, {g->kcells}}, st);
}
} // namespace mhh

MHH_API int mhh_budget_2_nprofs(unsigned int groups) { return (groups & ~BUDGET_ALL) ? -1 : budget_nprofs(groups); }
// the n-th profile of a group set: its name (Budget_2::create, :1315-1412) and 0 for "z", 1 for "zh"; NULL past the end
MHH_API const char* mhh_budget_2_prof_name(unsigned int groups, int n, int* half)
{
    if (n < 0 || (groups & ~BUDGET_ALL)) return nullptr;
    for (int G=0; G<BUDGET_NGROUPS; ++G)
    {
        if (!(groups & (1u << G))) continue;
        if (n < budget_np(G)) { if (half) *half = budget_names[G][n].half; return budget_names[G][n].name; }
        n -= budget_np(G);
    }
    return nullptr;
}
MHH_API unsigned long long mhh_budget_2_scratch_elems(const mhh_grid* g, int nmasks)
{
    if (!g || nmasks < 1) return 0;
    return (unsigned long long)budget_nprofs(BUDGET_ALL) * nmasks * g->kcells * level_chunks(g);
}

// Stats::calc_mask_mean_profile (src/stats.cxx:1328-1347) of u, v, w as double sums[3][nmasks][kcells] over ALL levels; a slab rank
// adds them over the ranks before mhh_budget_2_model_finish
MHH_API int mhh_budget_2_model_sums(const mhh_grid* g, const void* mfield, int nmasks, const void* u, const void* v, const void* w, void* sums, void* scratch, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(mfield && u && v && w && sums && scratch, "null pointer");
#define CALL(TF) budget_model_sums_launch<TF>(g, mfield, nmasks, u, v, w, static_cast<double*>(sums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// out[3][nmasks][kcells] of the grid's dtype = umodel, vmodel, wmodel: u and v divided by nmask[k], w by nmaskh[k]
MHH_API int mhh_budget_2_model_finish(const mhh_grid* g, int nmasks, const void* sums, const void* nmask, void* out, void* stream)
{
    if (int e = stats_check(g, nmasks)) return e;
    MHH_REQUIRE(sums && nmask && out, "null pointer");
    const dim3 grid((g->kcells + 255)/256, 3*nmasks);
#define CALL(TF) [&]{ hipLaunchKernelGGL(budget_finish_kernel<TF>, grid, dim3(256), 0, as_stream(stream), static_cast<const double*>(sums), static_cast<const int*>(nmask), \
                                         mp<TF>(out), nmasks, g->kcells, g->kstart, g->kend, 1); return MHH_OK; }()
    if (int e = MHH_DISPATCH(g, CALL)) return e;
#undef CALL
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// The calc_* loops of Budget_2::exec_stats (src/budget_2.cxx:1414-1818) and the calc_mean of calc_mask_stats over each, as double
// sums[nprofs][nmasks][kcells]
MHH_API int mhh_budget_2_sums(const mhh_grid* g, const void* mfield, int nmasks, const mhh_budget_2_desc* desc, void* sums, void* scratch, void* stream)
{
    if (int e = budget_check(g, nmasks, desc)) return e;
    MHH_REQUIRE(mfield && sums && scratch, "null pointer");
    MHH_REQUIRE(desc->u && desc->v && desc->w && desc->umodel && desc->vmodel && desc->wmodel, "u, v, w and their model profiles");
    MHH_REQUIRE(!(desc->groups & ((1u << BG_PRES) | (1u << BG_RDSTR) | (1u << BG_PRESS))) || desc->p, "the pressure groups need p");
    MHH_REQUIRE(!(desc->groups & BUDGET_NEEDS_B) || desc->bmean, "the buoyancy groups need bmean");
    MHH_REQUIRE(!(desc->groups & (1u << BG_PRESS)) || desc->pmean, "bw_pres and bw_rdstr need pmean");
    MHH_REQUIRE(g->dzi && g->dzhi, "dzi, dzhi");
#define CALL(TF) budget_sums_launch<TF>(g, mfield, nmasks, desc, static_cast<double*>(sums), static_cast<double*>(scratch), as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// out[nprofs][nmasks][kcells] of the grid's dtype: sum / nmask[k] (the full-level count, for "zh" profiles too) on kstart .. kend, the
// fill value where nmask[k] == 0 (calc_mask_stats, src/stats.cxx:1350-1390)
MHH_API int mhh_budget_2_finish(const mhh_grid* g, int nmasks, const mhh_budget_2_desc* desc, const void* sums, const void* nmask, void* out, void* stream)
{
    if (int e = budget_check(g, nmasks, desc)) return e;
    MHH_REQUIRE(sums && nmask && out, "null pointer");
    const dim3 grid((g->kcells + 255)/256, budget_nprofs(desc->groups)*nmasks);
#define CALL(TF) [&]{ hipLaunchKernelGGL(budget_finish_kernel<TF>, grid, dim3(256), 0, as_stream(stream), static_cast<const double*>(sums), static_cast<const int*>(nmask), \
                                         mp<TF>(out), nmasks, g->kcells, g->kstart, g->kend, 0); return MHH_OK; }()
    if (int e = MHH_DISPATCH(g, CALL)) return e;
#undef CALL
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// Thermo_dry::get_thermo_field("b") (calc_buoyancy, src/thermo_dry.cxx:51-63)
MHH_API int mhh_thermo_dry_buoyancy(const mhh_grid* g, void* b, const void* th, const void* thref, double grav, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(b && th && thref, "null pointer");
#define CALL(TF) [&]{ const BudgetDryBuoyancyOp<TF> op{mp<TF>(b), cp<TF>(th), cp<TF>(thref), TF(grav)}; \
                      return launch_cells(as_stream(stream), op, g->istart, g->iend, g->jstart, g->jend, 0, g->kcells, g->icells, g->ijcells); }()
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
