// pres4_bands.h -- what the single-GPU pressure plan (k_pres.hip) and the slab plan (k_slab.hip) build alike: the modified wave
// numbers of Pres_2 / Pres_4 and the seven bands of Pres_4 on the host (Pres_2::set_values src/pres_2.cxx:125-153;
// Pres_4::set_values src/pres_4.cxx:179-252), and the LU factorisation of one column's 7-band system on the device
// (src/pres_4.cxx:358-470, hdma :574-730). One copy, so that both plans solve with the same factor bits. Internal to the library.
#pragma once
#include <cmath>
#include <vector>
#include "k_common.h"

namespace mhh
{
template<class TF>
static void host_bmat(int order, const mhh_grid* g, std::vector<TF>& bi, std::vector<TF>& bj)
{
    const int itot = g->itot, jtot = g->jtot;
    const TF dx = TF(g->dx), dy = TF(g->dy);
    const TF dxidxi = 1./(dx*dx), dyidyi = 1./(dy*dy);
    const TF pi = std::acos(-1.);
    bi.resize(itot); bj.resize(jtot);
    if (order == 2)
    {
        for (int j=0; j<jtot/2+1; ++j) bj[j] = 2. * (std::cos(2.*pi*(TF)j/(TF)jtot)-1.) * dyidyi;
        for (int i=0; i<itot/2+1; ++i) bi[i] = 2. * (std::cos(2.*pi*(TF)i/(TF)itot)-1.) * dxidxi;
    }
    else
    {
        for (int j=0; j<jtot/2+1; j++)
            bj[j] = ( 2.* (1./576.) * std::cos(6.*pi*(double)j/(double)jtot) - 2.* (54./576.) * std::cos(4.*pi*(double)j/(double)jtot)
                    + 2.* (783./576.) * std::cos(2.*pi*(double)j/(double)jtot) - (1460./576.) ) * dyidyi;
        for (int i=0; i<itot/2+1; i++)
            bi[i] = ( 2.* (1./576.) * std::cos(6.*pi*(double)i/(double)itot) - 2.* (54./576.) * std::cos(4.*pi*(double)i/(double)itot)
                    + 2.* (783./576.) * std::cos(2.*pi*(double)i/(double)itot) - (1460./576.) ) * dxidxi;
    }
    for (int j=jtot/2+1; j<jtot; ++j) bj[j] = bj[jtot-j];
    for (int i=itot/2+1; i<itot; ++i) bi[i] = bi[itot-i];
}

// the bands m1..m7 of the interior rows, kmax values each, from the host metrics dzi4 / dzhi4 (kcells values each)
template<class TF>
static void host_pres4_bands(const mhh_grid* g, const TF* dzi4, const TF* h, std::vector<TF> (&m)[7])
{
    const int kmax = g->kmax, kstart = g->kstart;
    for (int n=0; n<7; ++n) m[n].assign(kmax, TF(0));
    std::vector<TF>& m1 = m[0]; std::vector<TF>& m2 = m[1]; std::vector<TF>& m3 = m[2]; std::vector<TF>& m4 = m[3];
    std::vector<TF>& m5 = m[4]; std::vector<TF>& m6 = m[5]; std::vector<TF>& m7 = m[6];
    int k = 0, kc = kstart;
    m1[k] = 0.;
    m2[k] = (1./576.) * (               -  27.*h[kc]                            ) * dzi4[kc];
    m3[k] = (1./576.) * ( -1.*h[kc+1] + 729.*h[kc] +  27.*h[kc+1]               ) * dzi4[kc];
    m4[k] = (1./576.) * ( 27.*h[kc+1] - 729.*h[kc] - 729.*h[kc+1] -  1.*h[kc+2] ) * dzi4[kc];
    m5[k] = (1./576.) * (-27.*h[kc+1] +  27.*h[kc] + 729.*h[kc+1] + 27.*h[kc+2] ) * dzi4[kc];
    m6[k] = (1./576.) * (  1.*h[kc+1]              -  27.*h[kc+1] - 27.*h[kc+2] ) * dzi4[kc];
    m7[k] = (1./576.) * (                                         +  1.*h[kc+2] ) * dzi4[kc];
    for (k=1; k<kmax-1; k++)
    {
        kc = kstart+k;
        m1[k] = (1./576.) * (   1.*h[kc-1]                                           ) * dzi4[kc];
        m2[k] = (1./576.) * ( -27.*h[kc-1] -  27.*h[kc]                              ) * dzi4[kc];
        m3[k] = (1./576.) * (  27.*h[kc-1] + 729.*h[kc] +  27.*h[kc+1]               ) * dzi4[kc];
        m4[k] = (1./576.) * (  -1.*h[kc-1] - 729.*h[kc] - 729.*h[kc+1] -  1.*h[kc+2] ) * dzi4[kc];
        m5[k] = (1./576.) * (              +  27.*h[kc] + 729.*h[kc+1] + 27.*h[kc+2] ) * dzi4[kc];
        m6[k] = (1./576.) * (                           -  27.*h[kc+1] - 27.*h[kc+2] ) * dzi4[kc];
        m7[k] = (1./576.) * (                                          +  1.*h[kc+2] ) * dzi4[kc];
    }
    k = kmax-1; kc = kstart+k;
    m1[k] = (1./576.) * (   1.*h[kc-1]                                         ) * dzi4[kc];
    m2[k] = (1./576.) * ( -27.*h[kc-1] -  27.*h[kc]                +  1.*h[kc] ) * dzi4[kc];
    m3[k] = (1./576.) * (  27.*h[kc-1] + 729.*h[kc] +  27.*h[kc+1] - 27.*h[kc] ) * dzi4[kc];
    m4[k] = (1./576.) * (  -1.*h[kc-1] - 729.*h[kc] - 729.*h[kc+1] + 27.*h[kc] ) * dzi4[kc];
    m5[k] = (1./576.) * (              +  27.*h[kc] + 729.*h[kc+1] -  1.*h[kc] ) * dzi4[kc];
    m6[k] = (1./576.) * (                           -  27.*h[kc+1]             ) * dzi4[kc];
    m7[k] = 0.;
}

// =======================================================================================================
// pres_4: 7-band LU without pivoting on kmax+4 unknowns per column (src/pres_4.cxx:358-470, hdma :574-730)
// The band matrix depends on the grid and (kx,ky) only, so its LU factors are computed once at plan creation
// (the reference's elimination order) and kept: band n (0..6), row r of a column at Wc[n*bstride + r*ncol].
// =======================================================================================================
// one column: Wc = the column's element of band 0, row 0; row r of band n at Wc[n*bstride + r*ncol]
template<class TF>
__device__ __forceinline__ void hdma_factor_column(TF* __restrict__ Wc, size_t ncol, size_t bstride, TF bi, TF bj, bool mean,
                                                   const TF* __restrict__ M1, const TF* __restrict__ M2, const TF* __restrict__ M3, const TF* __restrict__ M4,
                                                   const TF* __restrict__ M5, const TF* __restrict__ M6, const TF* __restrict__ M7, int kmax)
{
    TF* __restrict__ m1 = Wc;             TF* __restrict__ m2 = Wc + bstride;   TF* __restrict__ m3 = Wc + 2*bstride; TF* __restrict__ m4 = Wc + 3*bstride;
    TF* __restrict__ m5 = Wc + 4*bstride; TF* __restrict__ m6 = Wc + 5*bstride; TF* __restrict__ m7 = Wc + 6*bstride;
#define A(arr, k) arr[(size_t)(k)*ncol]
    // fill (rows 0,1: bottom bc; 2..kmax+1: interior; kmax+2, kmax+3: top bc)
    A(m1,0)=0; A(m2,0)=0; A(m3,0)=0; A(m4,0)=1; A(m5,0)=0;  A(m6,0)=0; A(m7,0)=-1;
    A(m1,1)=0; A(m2,1)=0; A(m3,1)=0; A(m4,1)=1; A(m5,1)=-1; A(m6,1)=0; A(m7,1)=0;
    for (int k=0; k<kmax; ++k)
    {
        A(m1,k+2)=M1[k]; A(m2,k+2)=M2[k]; A(m3,k+2)=M3[k]; A(m4,k+2)=M4[k] + bi + bj;
        A(m5,k+2)=M5[k]; A(m6,k+2)=M6[k]; A(m7,k+2)=M7[k];
    }
    const int t = kmax+2;
    if (mean) { A(m1,t)=TF(0.);    A(m2,t)=TF(-1/3.); A(m3,t)=TF(2.);  A(m4,t)=TF(1.);
                A(m1,t+1)=TF(-2.); A(m2,t+1)=TF(9.);  A(m3,t+1)=TF(0.); A(m4,t+1)=TF(1.); }
    else      { A(m1,t)=TF(0.);    A(m2,t)=TF(0.);    A(m3,t)=TF(-1.); A(m4,t)=TF(1.);
                A(m1,t+1)=TF(-1.); A(m2,t+1)=TF(0.);  A(m3,t+1)=TF(0.); A(m4,t+1)=TF(1.); }
    A(m5,t)=0; A(m6,t)=0; A(m7,t)=0;
    A(m5,t+1)=0; A(m6,t+1)=0; A(m7,t+1)=0;
    // LU
    int k = 0;
    A(m1,k)=1; A(m2,k)=1; A(m3,k)=TF(1.)/A(m4,k); A(m4,k)=1; A(m5,k)=A(m5,k)*A(m3,k); A(m6,k)=A(m6,k)*A(m3,k); A(m7,k)=A(m7,k)*A(m3,k);
    k = 1;
    A(m1,k)=1; A(m2,k)=1; A(m3,k)=A(m3,k)/A(m4,k-1);
    A(m4,k)=A(m4,k)-A(m3,k)*A(m5,k-1); A(m5,k)=A(m5,k)-A(m3,k)*A(m6,k-1); A(m6,k)=A(m6,k)-A(m3,k)*A(m7,k-1);
    k = 2;
    A(m1,k)=1; A(m2,k)=A(m2,k)/A(m4,k-2);
    A(m3,k)=( A(m3,k) - A(m2,k)*A(m5,k-2) ) / A(m4,k-1);
    A(m4,k)=A(m4,k) - A(m3,k)*A(m5,k-1) - A(m2,k)*A(m6,k-2);
    A(m5,k)=A(m5,k) - A(m3,k)*A(m6,k-1) - A(m2,k)*A(m7,k-2);
    A(m6,k)=A(m6,k) - A(m3,k)*A(m7,k-1);
    for (k=3; k<kmax+4; ++k)
    {
        if (k == kmax+2) A(m7,kmax+1) = TF(1.);
        A(m1,k)=( A(m1,k) ) / A(m4,k-3);
        A(m2,k)=( A(m2,k) - A(m1,k)*A(m5,k-3) ) / A(m4,k-2);
        A(m3,k)=( A(m3,k) - A(m2,k)*A(m5,k-2) - A(m1,k)*A(m6,k-3) ) / A(m4,k-1);
        A(m4,k)=  A(m4,k) - A(m3,k)*A(m5,k-1) - A(m2,k)*A(m6,k-2) - A(m1,k)*A(m7,k-3);
        if (k < kmax+3) A(m5,k)= A(m5,k) - A(m3,k)*A(m6,k-1) - A(m2,k)*A(m7,k-2);
        if (k < kmax+2) A(m6,k)= A(m6,k) - A(m3,k)*A(m7,k-1);
        if (k == kmax+2) { A(m6,k)=TF(1.); A(m7,k)=TF(1.); }
        if (k == kmax+3) { A(m5,k)=TF(1.); A(m6,k)=TF(1.); A(m7,k)=TF(1.); }
    }
#undef A
}
} // namespace mhh
