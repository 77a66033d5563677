// cell_ops.h -- per-cell arithmetic of the RHS operators (advec_2 / advec_2i5 / advec_4, diff_2 / diff_4 /
// diff_smag2, pres in/out) as __host__ __device__ inline functions.
//
// Every function returns the increment(s) the reference adds to ONE tendency cell, with the reference's
// expression association (file:line cited per function, paths relative to the reference root), so that
// with -ffp-contract=off the HIP kernels are bit-identical to the reference CPU path in fp64 and fp32.
// The functions take a pointer + flat index + strides, so the same body serves one-cell-per-thread
// kernels and the fused multi-tendency kernels. Compiling this header with a host compiler
// (MHH_HD empty) is how tests/emul checks the arithmetic on the CPU before any GPU time is spent.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#  define MHH_HD __host__ __device__ __forceinline__
#else
#  define MHH_HD inline
#endif

namespace mhh
{
// Kernel-side grid descriptor (subset of Grid_data, include/grid.h:49-135, narrowed to TF on the host).
template<class TF>
struct GridDev
{
    int itot, jtot, ktot, imax, jmax, kmax, igc, jgc, kgc;
    int icells, jcells, ijcells, kcells;
    int istart, iend, jstart, jend, kstart, kend;
    int dim3;                 // jtot != 1 (Advec_4::exec, src/advec_4.cxx:596)
    TF dx, dy, zsize;
    TF dxi_t, dyi_t;          // TF(1.)/dx : spelling of advec_*, pres_2  (TF quotient)
    TF dxi_d, dyi_d;          // TF(1./dx) : spelling of diff_smag2, pres_4, calc_cfl of advec_2/2i5 (double quotient, narrowed)
    TF dxidxi_d, dyidyi_d;    // TF(1./(dx*dx)): diff_smag2 diff_c / dnmul, diff_4 diff_c
    TF dxidxi_t, dyidyi_t;    // TF(1/(dx*dx)) : diff_4 diff_w
    double dxidxi_2, dyidyi_2;// double(TF(1)/(dx*dx)): diff_2 (src/diff_2.cxx:44-45, a double even in SP builds)
    const TF* z; const TF* dz; const TF* dzi; const TF* dzhi; const TF* dzi4; const TF* dzhi4;
};

MHH_HD double tabs(double a) { return __builtin_fabs(a); }
MHH_HD float  tabs(float a)  { return __builtin_fabsf(a); }

// ---- F2: TWO single-precision cells per lane (cells i, i+1 of a row). Every operation is the element-wise fp32 operation, so
// a kernel body written once against its "lane value" type computes, with F2, the same bits per cell as with float -- on
// gfx950 as packed instructions (v_pk_add_f32, v_pk_mul_f32: two cells per issue slot, no contraction involved). Used by the
// k-marching kernel for the fp32 configuration (k_march.hip); scalars (metrics, coefficients) stay plain float and broadcast.
#if defined(__clang__)
typedef float mhh_f2v __attribute__((ext_vector_type(2)));
struct F2
{
    mhh_f2v v;
    MHH_HD F2() {}
    MHH_HD F2(float s) : v{s, s} {}
    MHH_HD explicit F2(double s) : v{(float)s, (float)s} {}
    MHH_HD explicit F2(int s) : v{(float)s, (float)s} {}
    MHH_HD F2(mhh_f2v x) : v(x) {}
    MHH_HD F2(float a, float b) : v{a, b} {}
    MHH_HD float lo() const { return v.x; }
    MHH_HD float hi() const { return v.y; }
};
MHH_HD F2 operator+(F2 a, F2 b) { return F2(a.v + b.v); }
MHH_HD F2 operator-(F2 a, F2 b) { return F2(a.v - b.v); }
MHH_HD F2 operator*(F2 a, F2 b) { return F2(a.v * b.v); }
MHH_HD F2 operator/(F2 a, F2 b) { return F2(a.v / b.v); }
MHH_HD F2 operator-(F2 a) { return F2(-a.v); }
MHH_HD F2 tabs(F2 a) { return F2(__builtin_elementwise_abs(a.v)); }
MHH_HD F2 tfma(F2 a, F2 b, F2 c) { return F2(__builtin_fmaf(a.v.x, b.v.x, c.v.x), __builtin_fmaf(a.v.y, b.v.y, c.v.y)); }
#else   // host compilers (tests/emul): the same type, element by element
struct F2
{
    float v[2];
    F2() {}
    F2(float s) : v{s, s} {}
    explicit F2(double s) : v{(float)s, (float)s} {}
    explicit F2(int s) : v{(float)s, (float)s} {}
    F2(float a, float b) : v{a, b} {}
    float lo() const { return v[0]; }
    float hi() const { return v[1]; }
};
inline F2 operator+(F2 a, F2 b) { return F2(a.v[0] + b.v[0], a.v[1] + b.v[1]); }
inline F2 operator-(F2 a, F2 b) { return F2(a.v[0] - b.v[0], a.v[1] - b.v[1]); }
inline F2 operator*(F2 a, F2 b) { return F2(a.v[0] * b.v[0], a.v[1] * b.v[1]); }
inline F2 operator/(F2 a, F2 b) { return F2(a.v[0] / b.v[0], a.v[1] / b.v[1]); }
inline F2 operator-(F2 a) { return F2(-a.v[0], -a.v[1]); }
inline F2 tabs(F2 a) { return F2(__builtin_fabsf(a.v[0]), __builtin_fabsf(a.v[1])); }
inline F2 tfma(F2 a, F2 b, F2 c) { return F2(__builtin_fmaf(a.v[0], b.v[0], c.v[0]), __builtin_fmaf(a.v[1], b.v[1], c.v[1])); }
#endif
MHH_HD F2 operator+(F2 a) { return a; }
MHH_HD F2 operator+(F2 a, float b) { return a + F2(b); }
MHH_HD F2 operator+(float a, F2 b) { return F2(a) + b; }
MHH_HD F2 operator-(F2 a, float b) { return a - F2(b); }
MHH_HD F2 operator-(float a, F2 b) { return F2(a) - b; }
MHH_HD F2 operator*(F2 a, float b) { return a * F2(b); }
MHH_HD F2 operator*(float a, F2 b) { return F2(a) * b; }
MHH_HD F2 operator/(F2 a, float b) { return a / F2(b); }
MHH_HD F2& operator+=(F2& a, F2 b) { a = a + b; return a; }
MHH_HD F2& operator-=(F2& a, F2 b) { a = a - b; return a; }
// lane-value traits: the scalar type of the arithmetic and the cells a lane carries
template<class VT> struct lane_of { typedef VT scalar; static constexpr int cells = 1; };
template<> struct lane_of<F2> { typedef float scalar; static constexpr int cells = 2; };
template<class TF> MHH_HD TF tmin(TF a, TF b) { return (b < a) ? b : a; }   // std::min semantics
template<class TF> MHH_HD TF tmax(TF a, TF b) { return (a < b) ? b : a; }   // std::max semantics
template<class TF> MHH_HD TF sq(TF a) { return a*a; }

// ---- interpolation weights (include/finite_difference.h:36-155) -------------------------------------
template<class TF> MHH_HD TF i2(TF a, TF b) { return TF(0.5)*(a+b); }
template<class TF> MHH_HD TF i6(TF a, TF b, TF c, TF d, TF e, TF f)
{ return TF(37./60.)*(c+d) - TF(8./60.)*(b+e) + TF(1./60.)*(a+f); }
template<class TF> MHH_HD TF i5(TF a, TF b, TF c, TF d, TF e, TF f)
{ return TF(10./60.)*(d-c) - TF(5./60.)*(e-b) + TF(1./60.)*(f-a); }
template<class TF> MHH_HD TF i4ws(TF a, TF b, TF c, TF d) { return TF(7./12.)*(b+c) - TF(1./12.)*(a+d); }
template<class TF> MHH_HD TF i3ws(TF a, TF b, TF c, TF d) { return TF(3./12.)*(c-b) - TF(1./12.)*(d-a); }

// Four-point weights, summed left to right as the reference writes them. A product by a power of two is exact (no rounding
// unless it underflows: |x| < 2^-1018 in fp64), so RN(w*x + t) with such a w is ONE fma with the bits of the multiplication
// followed by the addition -- an instruction less per such weight (the -1/16 at both ends of the 4th-order interpolation: two of
// its seven operations, 108 of the ~900 vector instructions per cell of advec_4 + diff_4). The other weights keep their two
// roundings. F2 (two fp32 cells per lane) keeps the product-sum: its operations are packed instructions.
constexpr bool w_is_pow2(double w) { double a = w < 0 ? -w : w; if (a == 0) return false; while (a < 1) a *= 2; while (a > 1) a /= 2; return a == 1; }
template<class TF> MHH_HD TF pw2_fma(double w, TF x, TF t) { return TF(w)*x + t; }
MHH_HD double pw2_fma(double w, double x, double t) { return __builtin_fma(w, x, t); }
MHH_HD float  pw2_fma(double w, float x, float t)   { return __builtin_fmaf((float)w, x, t); }
#ifndef MHH_W4_POW2_FMA
#define MHH_W4_POW2_FMA 1
#endif
#define MHH_W4(name, w0, w1, w2, w3) \
    template<class TF> MHH_HD TF name(TF a, TF b, TF c, TF d) { \
        TF t; \
        if constexpr (MHH_W4_POW2_FMA && w_is_pow2(w0))      t = pw2_fma(w0, a, TF(w1)*b); \
        else if constexpr (MHH_W4_POW2_FMA && w_is_pow2(w1)) t = pw2_fma(w1, b, TF(w0)*a); \
        else                                                 t = TF(w0)*a + TF(w1)*b; \
        if constexpr (MHH_W4_POW2_FMA && w_is_pow2(w2)) t = pw2_fma(w2, c, t); else t = t + TF(w2)*c; \
        if constexpr (MHH_W4_POW2_FMA && w_is_pow2(w3)) t = pw2_fma(w3, d, t); else t = t + TF(w3)*d; \
        return t; }
MHH_W4(ci4, -1./16.,  9./16.,  9./16., -1./16.)
MHH_W4(bi4,  5./16., 15./16., -5./16.,  1./16.)
MHH_W4(ti4,  1./16., -5./16., 15./16.,  5./16.)
MHH_W4(cg4,  1./24., -27./24., 27./24., -1./24.)
MHH_W4(bg4, -23./24., 21./24.,  3./24., -1./24.)
MHH_W4(tg4,  1./24., -3./24., -21./24., 23./24.)
#undef MHH_W4
template<class TF> MHH_HD TF i4c(TF a, TF b, TF c, TF d) { return MHH_W4_POW2_FMA ? pw2_fma(-1./16., a+d, TF(9./16.)*(b+c)) : TF(-1./16.)*(a+d) + TF(9./16.)*(b+c); }

// =======================================================================================================
// advec_2 (src/advec_2.cxx:81-202). COMP: 0=u 1=v 2=w (momentum, staggering offset o = -1/-jj/-kk), 3=scalar.
// rt/rb/rc/dz are the face/cell density weights and the metric of the row k (chosen by the caller):
//   u,v,s: rt=rhorefh[k+1] rb=rhorefh[k] rc=rhoref[k] dz=dzi[k];  w: rt=rhoref[k] rb=rhoref[k-1] rc=rhorefh[k] dz=dzhi[k]
// =======================================================================================================
template<class TF>
MHH_HD TF advec2_mom(const TF* __restrict__ f, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                     int c, int o, int jj, int kk, TF dxi, TF dyi, TF rt, TF rb, TF rc, TF dz)
{
    return
        - ( i2(u[c+1+o], u[c+1]) * i2(f[c], f[c+1])
          - i2(u[c  +o], u[c  ]) * i2(f[c-1], f[c]) ) * dxi
        - ( i2(v[c+jj+o], v[c+jj]) * i2(f[c], f[c+jj])
          - i2(v[c   +o], v[c   ]) * i2(f[c-jj], f[c]) ) * dyi
        - ( rt * i2(w[c+kk+o], w[c+kk]) * i2(f[c], f[c+kk])
          - rb * i2(w[c   +o], w[c   ]) * i2(f[c-kk], f[c]) ) / rc * dz;
}
template<class TF>
MHH_HD TF advec2_s(const TF* __restrict__ s, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                   int c, int jj, int kk, TF dxi, TF dyi, TF rt, TF rb, TF rc, TF dz)
{
    return
        - ( u[c+1]  * i2(s[c], s[c+1])  - u[c] * i2(s[c-1],  s[c]) ) * dxi
        - ( v[c+jj] * i2(s[c], s[c+jj]) - v[c] * i2(s[c-jj], s[c]) ) * dyi
        - ( rt * w[c+kk] * i2(s[c], s[c+kk]) - rb * w[c] * i2(s[c-kk], s[c]) ) / rc * dz;
}

// =======================================================================================================
// advec_2i5 (src/advec_2i5.cxx:151-728)
// Vertical order table: order of the interpolation on a face. 0 = wall (no flux), 2 = 2nd (no upwind term),
// 4 = 4th centred + 3rd upwind, 6 = 6th centred + 5th upwind. For u,v,scalars `kf` is the bottom face of cell
// kf; for w it is the cell centre (the w equation's "faces").
// =======================================================================================================
MHH_HD int order_face_c(int kf, int kstart, int kend)
{
    if (kf <= kstart || kf >= kend) return 0;
    if (kf == kstart+1 || kf == kend-1) return 2;
    if (kf == kstart+2 || kf == kend-2) return 4;
    return 6;
}
MHH_HD int order_face_w(int kc, int kstart, int kend)
{
    if (kc == kstart || kc == kend-1) return 2;
    if (kc == kstart+1 || kc == kend-2) return 4;
    return 6;
}
// interpolants on the face between f[c-s] and f[c]
template<class TF> MHH_HD TF face_cen(const TF* __restrict__ f, int c, int s, int order)
{
    if (order == 2) return i2(f[c-s], f[c]);
    if (order == 4) return i4ws(f[c-2*s], f[c-s], f[c], f[c+s]);
    return i6(f[c-3*s], f[c-2*s], f[c-s], f[c], f[c+s], f[c+2*s]);
}
template<class TF> MHH_HD TF face_upw(const TF* __restrict__ f, int c, int s, int order)
{
    if (order == 4) return i3ws(f[c-2*s], f[c-s], f[c], f[c+s]);
    return i5(f[c-3*s], f[c-2*s], f[c-s], f[c], f[c+s], f[c+2*s]);
}

// horizontal increment (:181-201, :333-352, :483-503, :612-632); ue/uw/vn/vs = advecting face velocities
template<class TF>
MHH_HD TF advec25_hor(const TF* __restrict__ f, int c, int jj, TF ue, TF uw, TF vn, TF vs, TF dxi, TF dyi)
{
    const TF fm3 = f[c-3], fm2 = f[c-2], fm1 = f[c-1], f0 = f[c], fp1 = f[c+1], fp2 = f[c+2], fp3 = f[c+3];
    const TF gm3 = f[c-3*jj], gm2 = f[c-2*jj], gm1 = f[c-jj], gp1 = f[c+jj], gp2 = f[c+2*jj], gp3 = f[c+3*jj];
    return
        - ( ue * i6(fm2, fm1, f0, fp1, fp2, fp3) - uw * i6(fm3, fm2, fm1, f0, fp1, fp2) ) * dxi
        + ( tabs(ue) * i5(fm2, fm1, f0, fp1, fp2, fp3) - tabs(uw) * i5(fm3, fm2, fm1, f0, fp1, fp2) ) * dxi
        - ( vn * i6(gm2, gm1, f0, gp1, gp2, gp3) - vs * i6(gm3, gm2, gm1, f0, gp1, gp2) ) * dyi
        + ( tabs(vn) * i5(gm2, gm1, f0, gp1, gp2, gp3) - tabs(vs) * i5(gm3, gm2, gm1, f0, gp1, gp2) ) * dyi;
}
// the same with the cell's own value handed over (the marching kernel holds it in a register; f points at the cell in an
// LDS plane of row pitch jj). ue/uw/vn/vs may be SUMS a+b of the two velocities a face averages, with dxi/dyi halved by the
// caller: scaling by 2 commutes with every rounding of the expression (no overflow; exact unless a velocity sum is subnormal),
// so 0.5*(a+b) * I * dxi and (a+b) * I * (0.5*dxi) are the same bits -- one multiplication per face less.
// P = something indexable at the cell (a pointer, or the marching kernel's plane view), TF = the lane value, MT = the metrics' type
template<class P, class TF, class MT>
MHH_HD TF advec25_hor_f0(const P& f, TF f0, int jj, TF ue, TF uw, TF vn, TF vs, MT dxi, MT dyi)
{
    const TF fm3 = f[-3], fm2 = f[-2], fm1 = f[-1], fp1 = f[1], fp2 = f[2], fp3 = f[3];
    const TF gm3 = f[-3*jj], gm2 = f[-2*jj], gm1 = f[-jj], gp1 = f[jj], gp2 = f[2*jj], gp3 = f[3*jj];
    return
        - ( ue * i6(fm2, fm1, f0, fp1, fp2, fp3) - uw * i6(fm3, fm2, fm1, f0, fp1, fp2) ) * dxi
        + ( tabs(ue) * i5(fm2, fm1, f0, fp1, fp2, fp3) - tabs(uw) * i5(fm3, fm2, fm1, f0, fp1, fp2) ) * dxi
        - ( vn * i6(gm2, gm1, f0, gp1, gp2, gp3) - vs * i6(gm3, gm2, gm1, f0, gp1, gp2) ) * dyi
        + ( tabs(vn) * i5(gm2, gm1, f0, gp1, gp2, gp3) - tabs(vs) * i5(gm3, gm2, gm1, f0, gp1, gp2) ) * dyi;
}

// x / d for a divisor known in advance, with r = RN(1/d) from an IEEE division on the host: the correctly rounded quotient in
// five multiply-adds instead of the ~14 issue slots of a full fp64 division (v_rcp_f64, v_div_scale/fmas/fixup).
// q0 = RN(x r) is within 1.5 ulp of x/d; one residual correction makes it a faithful rounding (the residual is exact or
// rounded by < 2^-53 of itself, the correction term carries the 2^-53 relative error of r: together < 2^-51 ulp); from a
// faithful quotient a second correction with the exact residual RN(x - d q) gives RN(x/d) (Markstein's theorem; it needs
// r = RN(1/d) and a significand of d that is not all ones -- the host checks that, known_divisor_ok). Exact for x = 0 and for
// every x whose residual does not underflow (|x| > 2^-960 in fp64, |x| >= 2^-100 in fp32: the last bit of the residual of a
// faithful quotient is 2^-47 |x| at the least and has to stay at or above 2^-149; tests/cpp/tiling_probe.cpp, mode divknown, finds
// the first fp32 mismatches in the binade 2^-112 for d = 0.4 and 0.8, 2^-113 for d = 1/3, 2/3): eddy viscosities are never that small.
MHH_HD double tfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
MHH_HD float  tfma(float a, float b, float c)    { return __builtin_fmaf(a, b, c); }
template<class VT, class TF>
MHH_HD VT div_known(VT x, TF d, TF r)
{
    const VT md = VT(-d), rr = VT(r);
    VT q = x * rr;
    VT e = tfma(md, q, x);
    q = tfma(e, rr, q);
    e = tfma(md, q, x);
    return tfma(e, rr, q);
}

// vertical increment (:204-299 etc.) for face orders ot (top) / ob (bottom)
template<class TF>
MHH_HD TF advec25_ver(const TF* __restrict__ f, int c, int kk, int ot, int ob, TF wt, TF wb, TF rt, TF rb, TF rc, TF dz)
{
    const TF It = ot ? face_cen(f, c+kk, kk, ot) : TF(0);
    const TF Ib = ob ? face_cen(f, c, kk, ob) : TF(0);
    TF cen;
    if (ob == 0)      cen = - ( rt * wt * It ) / rc * dz;
    else if (ot == 0) cen = - ( -rb * wb * Ib ) / rc * dz;
    else              cen = - ( rt * wt * It - rb * wb * Ib ) / rc * dz;
    const bool ut = (ot >= 4), ub = (ob >= 4);
    if (ut && ub) return cen + ( rt * tabs(wt) * face_upw(f, c+kk, kk, ot) - rb * tabs(wb) * face_upw(f, c, kk, ob) ) / rc * dz;
    if (ut)       return cen + ( rt * tabs(wt) * face_upw(f, c+kk, kk, ot) ) / rc * dz;
    if (ub)       return cen - ( rb * tabs(wb) * face_upw(f, c, kk, ob) ) / rc * dz;
    return cen;
}

// advec_2i4 (src/advec_2i4.cxx:101-640): 2nd-order advecting velocities, 4th-order (-1,9,9,-1)/16 interpolation of the
// advected field, 2nd order on the vertical faces next to a wall; ONE increment per cell (x, y and z terms in one sum).
// ot / ob = order of the top / bottom vertical face: the 2i5 table capped at 4 (0 = wall, 2, 4).
template<class TF>
MHH_HD TF advec24(const TF* __restrict__ f, int c, int jj, int kk, TF ue, TF uw, TF vn, TF vs, TF wt, TF wb,
                  int ot, int ob, TF dxi, TF dyi, TF rt, TF rb, TF rc, TF dz)
{
    const TF It = (ot == 0) ? TF(0) : (ot == 2) ? i2(f[c], f[c+kk]) : i4c(f[c-kk], f[c], f[c+kk], f[c+2*kk]);
    const TF Ib = (ob == 0) ? TF(0) : (ob == 2) ? i2(f[c-kk], f[c]) : i4c(f[c-2*kk], f[c-kk], f[c], f[c+kk]);
    const TF X = ue * i4c(f[c-1 ], f[c], f[c+1 ], f[c+2   ]) - uw * i4c(f[c-2   ], f[c-1 ], f[c], f[c+1 ]);
    const TF Y = vn * i4c(f[c-jj], f[c], f[c+jj], f[c+2*jj]) - vs * i4c(f[c-2*jj], f[c-jj], f[c], f[c+jj]);
    if (ob == 0) return - ( X ) * dxi - ( Y ) * dyi - ( rt * wt * It ) / rc * dz;
    if (ot == 0) return - ( X ) * dxi - ( Y ) * dyi - ( -rb * wb * Ib ) / rc * dz;
    return - ( X ) * dxi - ( Y ) * dyi - ( rt * wt * It - rb * wb * Ib ) / rc * dz;
}

// advec_2i62 (src/advec_2i62.cxx:105-310): 6th-order interpolation of the advected field horizontally, two-point
// interpolation vertically on every level; one increment per cell.
template<class TF>
MHH_HD TF advec262(const TF* __restrict__ f, int c, int jj, int kk, TF ue, TF uw, TF vn, TF vs, TF wt, TF wb,
                   TF dxi, TF dyi, TF rt, TF rb, TF rc, TF dz)
{
    return - ( ue * i6(f[c-2   ], f[c-1 ], f[c], f[c+1 ], f[c+2   ], f[c+3   ]) - uw * i6(f[c-3   ], f[c-2   ], f[c-1 ], f[c], f[c+1 ], f[c+2   ]) ) * dxi
           - ( vn * i6(f[c-2*jj], f[c-jj], f[c], f[c+jj], f[c+2*jj], f[c+3*jj]) - vs * i6(f[c-3*jj], f[c-2*jj], f[c-jj], f[c], f[c+jj], f[c+2*jj]) ) * dyi
           - ( rt * wt * i2(f[c], f[c+kk]) - rb * wb * i2(f[c-kk], f[c]) ) / rc * dz;
}

// Thermo_dry buoyancy tendency of w (src/thermo_dry.cxx:165-197): grav/threfh[k] * (th at the w level - threfh[k])
template<class TF>
MHH_HD TF buoyancy_tend(const TF* __restrict__ th, int c, int kk, int order, TF grav, TF threfh_k)
{
    const TF thh = (order == 4) ? i4c(th[c-2*kk], th[c-kk], th[c], th[c+kk]) : i2(th[c-kk], th[c]);
    return grav/threfh_k * (thh - threfh_k);
}

// Thermo_buoy (src/thermo_buoy.cxx), in the reference's expression order. Only the w terms depend on k near the walls: the
// caller runs them for k in (kstart, kend), so b[k-2] at k = kstart+1 is b[kstart-1], the first ghost level. What needs kgc >= 2 at
// 4th order is the bt term of the slope form, w[k+2] = w[kend+1] at k = kend-1; the entry points ask it of every 4th-order call,
// as the dry buoyancy does.
// b at the w level: calc_buoyancy_tend_2nd / _4th (:94-109, :167-184)
template<class TF> MHH_HD TF buoy_w(const TF* __restrict__ b, int c, int kk, int order)
{ return (order == 4) ? i4c(b[c-2*kk], b[c-kk], b[c], b[c+kk]) : i2(b[c-kk], b[c]); }
// the same at 4th order from a register window b[k-2 .. k+1] (k_march4.hip)
template<class TF> MHH_HD TF buoy_w4(const TF (&bw)[4]) { return i4c(bw[0], bw[1], bw[2], bw[3]); }
// b at the u location (calc_buoyancy_tend_u_2nd / _4th, :111-126, :186-201): b[i-2] at istart needs igc >= 2 at 4th order
template<class TF> MHH_HD TF buoy_u(const TF* __restrict__ b, int c, int order)
{ return (order == 4) ? i4c(b[c-2], b[c-1], b[c], b[c+1]) : i2(b[c-1], b[c]); }
// the stratification term of bt (calc_buoyancy_tend_b_2nd / _4th, :145-165, :220-250): bt -= n2 * buoy_bt(...)
template<class TF> MHH_HD TF buoy_bt(const TF* __restrict__ u, const TF* __restrict__ w, int c, int kk, int order, TF sa, TF ca, TF utrans)
{
    if (order == 4) return sa * (i4c(u[c-1], u[c], u[c+1], u[c+2]) + utrans) + ca * i4c(w[c-kk], w[c], w[c+kk], w[c+2*kk]);
    return sa * (i2(u[c], u[c+1]) + utrans) + ca * i2(w[c], w[c+kk]);
}
// calc_N2 (:49-61)
template<class TF> MHH_HD TF buoy_N2(TF bm, TF bp, TF dzi, TF bg_n2) { return TF(0.5)*(bp - bm)*dzi + bg_n2; }

// =======================================================================================================
// Koren (1993) flux-limited scalar advection (include/advec_monotonic.h:10-180, selected per scalar by
// advec.fluxlimit_list, src/advec_2i5.cxx:921,1030). face = 0: interior face, 1: first face above the bottom wall
// (upwind value for upward flow), 2: last face below the top wall (upwind value for downward flow).
// =======================================================================================================
MHH_HD double tcopysign1(double d) { return __builtin_copysign(1., d); }
MHH_HD float  tcopysign1(float d)  { return __builtin_copysignf(1.f, d); }
template<class TF> MHH_HD TF teps();
template<> MHH_HD double teps<double>() { return 2.220446049250313e-16; }
template<> MHH_HD float  teps<float>()  { return 1.1920928955078125e-07f; }
template<class TF>
MHH_HD TF koren_upwind(TF vel, TF far, TF near_, TF across)          // vel * (near + phi/2 * (near - far)), r from across-near
{
    const TF d = near_ - far;
    const TF denom = tcopysign1(d) * tmax(tabs(d), teps<TF>());
    const TF two_r = TF(2.) * (across - near_) / denom;
    const TF phi = tmax(TF(0.), tmin(two_r, tmin(TF(1./3.)*(TF(1.)+two_r), TF(2.))));
    return vel*(near_ + TF(0.5)*phi*(near_ - far));
}
template<class TF>
MHH_HD TF koren_flux(int face, TF vel, TF sm2, TF sm1, TF sp1, TF sp2)
{
    if (vel >= TF(0.)) return (face == 1) ? vel*sm1 : koren_upwind(vel, sm2, sm1, sp1);
    return (face == 2) ? vel*sp1 : koren_upwind(vel, sp2, sp1, sm1);
}
// increment of st at cell c; lev: 0 interior, 1 kstart, 2 kstart+1, 3 kend-2, 4 kend-1
template<class TF>
MHH_HD TF advec_s_lim_cell(const TF* __restrict__ s, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                           int c, int jj, int kk, int lev, TF dxi, TF dyi, TF rt, TF rb, TF rc, TF dz)
{
    const TF xm2 = s[c-2], xm1 = s[c-1], s0 = s[c], xp1 = s[c+1], xp2 = s[c+2];
    const TF ym2 = s[c-2*jj], ym1 = s[c-jj], yp1 = s[c+jj], yp2 = s[c+2*jj];
    const TF hor = - ( koren_flux(0, u[c+1],  xm1, s0, xp1, xp2) - koren_flux(0, u[c], xm2, xm1, s0, xp1) ) * dxi
                   - ( koren_flux(0, v[c+jj], ym1, s0, yp1, yp2) - koren_flux(0, v[c], ym2, ym1, s0, yp1) ) * dyi;
    const TF zm1 = s[c-kk], zp1 = s[c+kk];
    if (lev == 1) return hor - ( rt * koren_flux(1, w[c+kk], zm1, s0, zp1, s[c+2*kk]) ) / rc * dz;
    if (lev == 4) return hor - ( - rb * koren_flux(2, w[c], s[c-2*kk], zm1, s0, zp1) ) / rc * dz;
    const TF zm2 = s[c-2*kk], zp2 = s[c+2*kk];
    return hor - ( rt * koren_flux(lev == 3 ? 2 : 0, w[c+kk], zm1, s0, zp1, zp2)
                 - rb * koren_flux(lev == 2 ? 1 : 0, w[c],    zm2, zm1, s0, zp1) ) / rc * dz;
}

// =======================================================================================================
// advec_4 (src/advec_4.cxx:88-486): three separate decrements (x, y if dim3, z); returns them through d[3].
// sd = staggering stride of the advected momentum component (1, jj, kk); is_w selects the w equation, whose
// vertical advecting velocity is the advected field itself incl. the biased wall forms.
// =======================================================================================================
// The arithmetic is written once against a "view" of each field -- view.at<DI,DJ,DK>() = the value DI, DJ, DK cells away
// from the cell being updated -- so that the one-thread-per-cell kernels (GlobalView: flat array) and the k-marching
// kernel (k_march4.hip: LDS planes for horizontal offsets, a register window for the own column) execute the very same
// expressions.
template<class TF> struct GlobalView
{
    const TF* __restrict__ p; int c, jj, kk;
    template<int DI, int DJ, int DK> MHH_HD TF at() const { return p[c + DI + DJ*jj + DK*kk]; }
};
// 4th-order interpolation of `a` to the location of momentum component COMP (along its staggering direction), evaluated
// at the cell (SI, SJ, SK) away: a[-2e], a[-e], a[0], a[+e] with e the unit vector of COMP
template<int COMP, int SI, int SJ, int SK, class TF, class V>
MHH_HD TF stag_ci4(const V& a)
{
    constexpr int EI = (COMP == 0), EJ = (COMP == 1), EK = (COMP == 2);
    return ci4<TF>(a.template at<SI-2*EI, SJ-2*EJ, SK-2*EK>(), a.template at<SI-EI, SJ-EJ, SK-EK>(),
                   a.template at<SI, SJ, SK>(), a.template at<SI+EI, SJ+EJ, SK+EK>());
}
template<int COMP, int M, class TF, class FV, class UV>
MHH_HD TF advec4_px(const FV& f, const UV& u)
{ return stag_ci4<COMP, M-1, 0, 0, TF>(u) * ci4<TF>(f.template at<M-3,0,0>(), f.template at<M-2,0,0>(), f.template at<M-1,0,0>(), f.template at<M,0,0>()); }
template<int COMP, int M, class TF, class FV, class VV>
MHH_HD TF advec4_py(const FV& f, const VV& v)
{ return stag_ci4<COMP, 0, M-1, 0, TF>(v) * ci4<TF>(f.template at<0,M-3,0>(), f.template at<0,M-2,0>(), f.template at<0,M-1,0>(), f.template at<0,M,0>()); }
template<int COMP, int M, class TF, class FV, class WV>
MHH_HD TF advec4_pz(const FV& f, const WV& w, bool bot, bool top)
{
    TF fi;
    if (M == 0 && bot)      fi = bi4<TF>(f.template at<0,0,-2>(), f.template at<0,0,-1>(), f.template at<0,0,0>(), f.template at<0,0,1>());
    else if (M == 3 && top) fi = ti4<TF>(f.template at<0,0,-1>(), f.template at<0,0,0>(), f.template at<0,0,1>(), f.template at<0,0,2>());
    else                    fi = ci4<TF>(f.template at<0,0,M-3>(), f.template at<0,0,M-2>(), f.template at<0,0,M-1>(), f.template at<0,0,M>());
    TF ve;
    if constexpr (COMP == 2) ve = fi;                        // the w equation advects itself vertically
    else                     ve = stag_ci4<COMP, 0, 0, M-1, TF>(w);
    return ve * fi;
}
// COMP = 0, 1, 2: the u, v, w equation; f is the advected component itself (u, v or w)
template<int COMP, class TF, class FV, class UV, class VV, class WV>
MHH_HD void advec4_mom_v(TF d[3], const FV& f, const UV& u, const VV& v, const WV& w, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3)
{
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    d[0] = ( cg0*advec4_px<COMP,0,TF>(f, u) + cg1*advec4_px<COMP,1,TF>(f, u) + cg2*advec4_px<COMP,2,TF>(f, u) + cg3*advec4_px<COMP,3,TF>(f, u) ) * dxi;
    d[1] = TF(0);
    if (dim3)
        d[1] = ( cg0*advec4_py<COMP,0,TF>(f, v) + cg1*advec4_py<COMP,1,TF>(f, v) + cg2*advec4_py<COMP,2,TF>(f, v) + cg3*advec4_py<COMP,3,TF>(f, v) ) * dyi;
    d[2] = ( cg0*advec4_pz<COMP,0,TF>(f, w, bot, top) + cg1*advec4_pz<COMP,1,TF>(f, w, bot, top)
           + cg2*advec4_pz<COMP,2,TF>(f, w, bot, top) + cg3*advec4_pz<COMP,3,TF>(f, w, bot, top) ) * dz;
}
// The same with the VERTICAL face products carried from level to level by a k-marching kernel (k_march4.hip): product M of level
// k+1 is product M+1 of level k -- same operands, same order -- so a level forms only its topmost product (M = 3) and takes the
// other three from the level below (c[0..2]); `fresh` (the first level a thread works, and the levels whose lowest product is the
// biased wall form) forms all four. Fifteen operations and four LDS reads per reused product of the u and v equations, eight
// for w. The sum and its order are advec4_mom_v's: the same bits.
template<int COMP, class TF, class FV, class UV, class VV, class WV>
MHH_HD void advec4_mom_vc(TF d[3], const FV& f, const UV& u, const VV& v, const WV& w, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3, TF (&c)[3], bool fresh)
{
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    d[0] = ( cg0*advec4_px<COMP,0,TF>(f, u) + cg1*advec4_px<COMP,1,TF>(f, u) + cg2*advec4_px<COMP,2,TF>(f, u) + cg3*advec4_px<COMP,3,TF>(f, u) ) * dxi;
    d[1] = TF(0);
    if (dim3)
        d[1] = ( cg0*advec4_py<COMP,0,TF>(f, v) + cg1*advec4_py<COMP,1,TF>(f, v) + cg2*advec4_py<COMP,2,TF>(f, v) + cg3*advec4_py<COMP,3,TF>(f, v) ) * dyi;
    TF p0, p1, p2;
    if (fresh) { p0 = advec4_pz<COMP,0,TF>(f, w, bot, top); p1 = advec4_pz<COMP,1,TF>(f, w, bot, top); p2 = advec4_pz<COMP,2,TF>(f, w, bot, top); }
    else       { p0 = c[0]; p1 = c[1]; p2 = c[2]; }
    const TF p3 = advec4_pz<COMP,3,TF>(f, w, bot, top);
    d[2] = ( cg0*p0 + cg1*p1 + cg2*p2 + cg3*p3 ) * dz;
    c[0] = p1; c[1] = p2; c[2] = p3;
}
// advec_4m (src/advec_4m.cxx:90-478): every term is grad4 over four face products, each the 4th-order interpolated
// advecting velocity times a TWO-point mean of the advected quantity over a widening stencil ((-3,0), (-1,0), (0,1), (0,3)
// cells along the direction); at the walls the outermost vertical product is the mirrored one. One increment per cell.
// COMP 0..2 = u, v, w equation, 3 = scalar (velocities taken at their faces, no interpolation).
template<class TF> MHH_HD TF grad4m(TF a, TF b, TF c, TF d) { return - TF(1./24.)*(d-a) - TF(-27./24.)*(c-b); }
template<int COMP, int DI, int DJ, int DK, class TF, class V>
MHH_HD TF vel4m(const V& a)
{
    if constexpr (COMP == 3) return a.template at<DI, DJ, DK>();
    else
    {   // interp4c, the paired form -1/16 (a+d) + 9/16 (b+c) (advec_4 proper uses the four-term sum)
        constexpr int EI = (COMP == 0), EJ = (COMP == 1), EK = (COMP == 2);
        return i4c<TF>(a.template at<DI-2*EI, DJ-2*EJ, DK-2*EK>(), a.template at<DI-EI, DJ-EJ, DK-EK>(),
                       a.template at<DI, DJ, DK>(), a.template at<DI+EI, DJ+EJ, DK+EK>());
    }
}
template<int COMP, class TF, class FV, class UV, class VV, class WV>
MHH_HD TF advec4m_v(const FV& f, const UV& u, const VV& v, const WV& w, bool bot, bool top, TF dxi, TF dyi, TF dz)
{
    const TF gx = grad4m<TF>(vel4m<COMP,-1,0,0,TF>(u) * i2(f.template at<-3,0,0>(), f.template at<0,0,0>()),
                             vel4m<COMP, 0,0,0,TF>(u) * i2(f.template at<-1,0,0>(), f.template at<0,0,0>()),
                             vel4m<COMP, 1,0,0,TF>(u) * i2(f.template at< 0,0,0>(), f.template at<1,0,0>()),
                             vel4m<COMP, 2,0,0,TF>(u) * i2(f.template at< 0,0,0>(), f.template at<3,0,0>()));
    const TF gy = grad4m<TF>(vel4m<COMP,0,-1,0,TF>(v) * i2(f.template at<0,-3,0>(), f.template at<0,0,0>()),
                             vel4m<COMP,0, 0,0,TF>(v) * i2(f.template at<0,-1,0>(), f.template at<0,0,0>()),
                             vel4m<COMP,0, 1,0,TF>(v) * i2(f.template at<0, 0,0>(), f.template at<0,1,0>()),
                             vel4m<COMP,0, 2,0,TF>(v) * i2(f.template at<0, 0,0>(), f.template at<0,3,0>()));
    const TF p0 = bot ? -vel4m<COMP,0,0, 1,TF>(w) * i2(f.template at<0,0,-1>(), f.template at<0,0,2>())
                      :  vel4m<COMP,0,0,-1,TF>(w) * i2(f.template at<0,0,-3>(), f.template at<0,0,0>());
    const TF p3 = top ? -vel4m<COMP,0,0, 0,TF>(w) * i2(f.template at<0,0,-2>(), f.template at<0,0,1>())
                      :  vel4m<COMP,0,0, 2,TF>(w) * i2(f.template at<0,0, 0>(), f.template at<0,0,3>());
    const TF gz = grad4m<TF>(p0,
                             vel4m<COMP,0,0,0,TF>(w) * i2(f.template at<0,0,-1>(), f.template at<0,0,0>()),
                             vel4m<COMP,0,0,1,TF>(w) * i2(f.template at<0,0, 0>(), f.template at<0,0,1>()),
                             p3);
    return - gx * dxi - gy * dyi - gz * dz;
}
template<class TF>
MHH_HD TF advec4m(int comp, const TF* __restrict__ f, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                  int c, int jj, int kk, bool bot, bool top, TF dxi, TF dyi, TF dz)
{
    const GlobalView<TF> fv{f, c, jj, kk}, uv{u, c, jj, kk}, vv{v, c, jj, kk}, wv{w, c, jj, kk};
    if (comp == 0) return advec4m_v<0, TF>(fv, uv, vv, wv, bot, top, dxi, dyi, dz);
    if (comp == 1) return advec4m_v<1, TF>(fv, uv, vv, wv, bot, top, dxi, dyi, dz);
    if (comp == 2) return advec4m_v<2, TF>(fv, uv, vv, wv, false, false, dxi, dyi, dz);
    return advec4m_v<3, TF>(fv, uv, vv, wv, bot, top, dxi, dyi, dz);
}
template<class TF>
MHH_HD void advec4_mom(TF d[3], const TF* __restrict__ f, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                       int c, int sd, bool is_w, int jj, int kk, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3)
{
    const GlobalView<TF> fv{f, c, jj, kk}, uv{u, c, jj, kk}, vv{v, c, jj, kk}, wv{w, c, jj, kk};
    if (is_w)          advec4_mom_v<2>(d, fv, uv, vv, wv, bot, top, dxi, dyi, dz, dim3);
    else if (sd == 1)  advec4_mom_v<0>(d, fv, uv, vv, wv, bot, top, dxi, dyi, dz, dim3);
    else               advec4_mom_v<1>(d, fv, uv, vv, wv, bot, top, dxi, dyi, dz, dim3);
}
// Scalar advection (src/advec_4.cxx:360-486): the velocities are taken at their faces, no interpolation. Written against views as
// advec4_mom_v: u is read at<-1..2,0,0>, v at<0,-1..2,0>, w at<0,0,-1..2>, s at +-3 along each axis.
template<int M, class TF, class SV, class UV>
MHH_HD TF advec4_s_px(const SV& s, const UV& u)
{ return u.template at<M-1,0,0>() * ci4<TF>(s.template at<M-3,0,0>(), s.template at<M-2,0,0>(), s.template at<M-1,0,0>(), s.template at<M,0,0>()); }
template<int M, class TF, class SV, class VV>
MHH_HD TF advec4_s_py(const SV& s, const VV& v)
{ return v.template at<0,M-1,0>() * ci4<TF>(s.template at<0,M-3,0>(), s.template at<0,M-2,0>(), s.template at<0,M-1,0>(), s.template at<0,M,0>()); }
template<int M, class TF, class SV, class WV>
MHH_HD TF advec4_s_pz(const SV& s, const WV& w, bool bot, bool top)
{
    TF fi;
    if (M == 0 && bot)      fi = bi4<TF>(s.template at<0,0,-2>(), s.template at<0,0,-1>(), s.template at<0,0,0>(), s.template at<0,0,1>());
    else if (M == 3 && top) fi = ti4<TF>(s.template at<0,0,-1>(), s.template at<0,0,0>(), s.template at<0,0,1>(), s.template at<0,0,2>());
    else                    fi = ci4<TF>(s.template at<0,0,M-3>(), s.template at<0,0,M-2>(), s.template at<0,0,M-1>(), s.template at<0,0,M>());
    return w.template at<0,0,M-1>() * fi;
}
// The vertical face products w * ci4(s ...) are carried from level to level (see advec4_mom_vc): product M of level k+1 is
// product M+1 of level k, same operands in the same order; `fresh` forms all four. This is the one statement of the arithmetic:
// advec4_s_v is the form that carries nothing
template<class TF, class SV, class UV, class VV, class WV>
MHH_HD void advec4_s_vc(TF d[3], const SV& s, const UV& u, const VV& v, const WV& w, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3, TF (&c)[3], bool fresh)
{
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    d[0] = ( cg0*advec4_s_px<0,TF>(s, u) + cg1*advec4_s_px<1,TF>(s, u) + cg2*advec4_s_px<2,TF>(s, u) + cg3*advec4_s_px<3,TF>(s, u) ) * dxi;
    d[1] = TF(0);
    if (dim3)
        d[1] = ( cg0*advec4_s_py<0,TF>(s, v) + cg1*advec4_s_py<1,TF>(s, v) + cg2*advec4_s_py<2,TF>(s, v) + cg3*advec4_s_py<3,TF>(s, v) ) * dyi;
    TF p0, p1, p2;
    if (fresh) { p0 = advec4_s_pz<0,TF>(s, w, bot, top); p1 = advec4_s_pz<1,TF>(s, w, bot, top); p2 = advec4_s_pz<2,TF>(s, w, bot, top); }
    else       { p0 = c[0]; p1 = c[1]; p2 = c[2]; }
    const TF p3 = advec4_s_pz<3,TF>(s, w, bot, top);
    d[2] = ( cg0*p0 + cg1*p1 + cg2*p2 + cg3*p3 ) * dz;
    c[0] = p1; c[1] = p2; c[2] = p3;
}
template<class TF, class SV, class UV, class VV, class WV>
MHH_HD void advec4_s_v(TF d[3], const SV& s, const UV& u, const VV& v, const WV& w, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3)
{
    TF carried[3];
    advec4_s_vc(d, s, u, v, w, bot, top, dxi, dyi, dz, dim3, carried, true);
}
template<class TF>
MHH_HD void advec4_s(TF d[3], const TF* __restrict__ s, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                     int c, int jj, int kk, bool bot, bool top, TF dxi, TF dyi, TF dz, bool dim3)
{
    const GlobalView<TF> sv{s, c, jj, kk}, uv{u, c, jj, kk}, vv{v, c, jj, kk}, wv{w, c, jj, kk};
    advec4_s_v(d, sv, uv, vv, wv, bot, top, dxi, dyi, dz, dim3);
}

// calc_cfl integrand (advec_2.cxx:51-78, advec_2i5.cxx:60-148, advec_4.cxx:51-86)
template<class TF>
MHH_HD TF cfl_cell(int scheme, const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                   int c, int jj, int kk, int k, int kstart, int kend, TF dxi, TF dyi, TF dzi_k)
{
    if (scheme == 2)
        return tabs(i2(u[c], u[c+1]))*dxi + tabs(i2(v[c], v[c+jj]))*dyi + tabs(i2(w[c], w[c+kk]))*dzi_k;
    if (scheme == 41)       // src/advec_4m.cxx:51-88: the weighted sum spelled out, metrics dxi = 1./dx and dzi
        return tabs(ci4(u[c-1], u[c], u[c+1], u[c+2]))*dxi + tabs(ci4(v[c-jj], v[c], v[c+jj], v[c+2*jj]))*dyi
             + tabs(ci4(w[c-kk], w[c], w[c+kk], w[c+2*kk]))*dzi_k;
    if (scheme == 262)      // src/advec_2i62.cxx:58-105
        return tabs(i6(u[c-2], u[c-1], u[c], u[c+1], u[c+2], u[c+3]))*dxi + tabs(i6(v[c-2*jj], v[c-jj], v[c], v[c+jj], v[c+2*jj], v[c+3*jj]))*dyi
             + tabs(i2(w[c], w[c+kk]))*dzi_k;
    if (scheme == 24)       // src/advec_2i4.cxx:51-99
        return tabs(i4c(u[c-1], u[c], u[c+1], u[c+2]))*dxi + tabs(i4c(v[c-jj], v[c], v[c+jj], v[c+2*jj]))*dyi
             + tabs((k == kstart || k == kend-1) ? i2(w[c], w[c+kk]) : i4c(w[c-kk], w[c], w[c+kk], w[c+2*kk]))*dzi_k;
    if (scheme == 4)
        return tabs(i4c(u[c-1], u[c], u[c+1], u[c+2]))*dxi + tabs(i4c(v[c-jj], v[c], v[c+jj], v[c+2*jj]))*dyi
             + tabs(i4c(w[c-kk], w[c], w[c+kk], w[c+2*kk]))*dzi_k;
    TF wi;
    if (k == kstart || k == kend-1)        wi = i2(w[c], w[c+kk]);
    else if (k == kstart+1 || k == kend-2 || scheme == 253) wi = i4ws(w[c-kk], w[c], w[c+kk], w[c+2*kk]);   // 2i53: 4th order on every inner level
    else                                   wi = i6(w[c-2*kk], w[c-kk], w[c], w[c+kk], w[c+2*kk], w[c+3*kk]);
    return tabs(i6(u[c-2], u[c-1], u[c], u[c+1], u[c+2], u[c+3]))*dxi
         + tabs(i6(v[c-2*jj], v[c-jj], v[c], v[c+jj], v[c+2*jj], v[c+3*jj]))*dyi
         + tabs(wi)*dzi_k;
}

// =======================================================================================================
// diff_2 (src/diff_2.cxx:39-86): at += visc * ( ... ) with DOUBLE dxidxi/dyidyi. Returns the new tendency value
// (the += is evaluated in the promoted type, so the caller must not re-round).
//   centred fields: gt=dzhi[k+1] gb=dzhi[k] gc=dzi[k];  w: gt=dzi[k] gb=dzi[k-1] gc=dzhi[k]
// =======================================================================================================
template<class TF>
MHH_HD TF diff2_apply(TF t, const TF* __restrict__ a, int c, int jj, int kk, TF visc, double dxidxi, double dyidyi, TF gt, TF gb, TF gc)
{
    t += visc * (
            + ( (a[c+1 ] - a[c]) - (a[c] - a[c-1 ]) ) * dxidxi
            + ( (a[c+jj] - a[c]) - (a[c] - a[c-jj]) ) * dyidyi
            + ( (a[c+kk] - a[c]) * gt - (a[c] - a[c-kk]) * gb ) * gc );
    return t;
}

// =======================================================================================================
// diff_4 (src/diff_4.cxx:41-173): three increments. g4[0..3] = inner metric at the four faces, go = outer metric.
// =======================================================================================================
template<class TF, class AV>
MHH_HD void diff4_v(TF d[3], const AV& a, bool bot, bool top, TF visc, TF dxidxi, TF dyidyi, const TF g4[4], TF go, bool dim3)
{
    const TF cdg0 = TF(-1460./576.), cdg1 = TF(783./576.), cdg2 = TF(-54./576.), cdg3 = TF(1./576.);
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    d[0] = visc * (cdg3*a.template at<-3,0,0>() + cdg2*a.template at<-2,0,0>() + cdg1*a.template at<-1,0,0>() + cdg0*a.template at<0,0,0>()
                 + cdg1*a.template at<1,0,0>() + cdg2*a.template at<2,0,0>() + cdg3*a.template at<3,0,0>())*dxidxi;
    d[1] = TF(0);
    if (dim3)
        d[1] = visc * (cdg3*a.template at<0,-3,0>() + cdg2*a.template at<0,-2,0>() + cdg1*a.template at<0,-1,0>() + cdg0*a.template at<0,0,0>()
                     + cdg1*a.template at<0,1,0>() + cdg2*a.template at<0,2,0>() + cdg3*a.template at<0,3,0>())*dyidyi;
    const TF g0 = bot ? bg4<TF>(a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>())
                      : cg4<TF>(a.template at<0,0,-3>(), a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>());
    const TF g3 = top ? tg4<TF>(a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>())
                      : cg4<TF>(a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>(), a.template at<0,0,3>());
    d[2] = visc * ( cg0*g0 * g4[0]
                  + cg1*cg4<TF>(a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>()) * g4[1]
                  + cg2*cg4<TF>(a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>()) * g4[2]
                  + cg3*g3 * g4[3] ) * go;
}
// diff4_v with the inner vertical gradients carried from level to level (see advec4_mom_vc): gradient M of level k+1 is gradient
// M+1 of level k; seven operations per reused gradient
template<class TF, class AV>
MHH_HD void diff4_vc(TF d[3], const AV& a, bool bot, bool top, TF visc, TF dxidxi, TF dyidyi, const TF g4[4], TF go, bool dim3, TF (&c)[3], bool fresh)
{
    const TF cdg0 = TF(-1460./576.), cdg1 = TF(783./576.), cdg2 = TF(-54./576.), cdg3 = TF(1./576.);
    const TF cg0 = TF(1./24.), cg1 = TF(-27./24.), cg2 = TF(27./24.), cg3 = TF(-1./24.);
    d[0] = visc * (cdg3*a.template at<-3,0,0>() + cdg2*a.template at<-2,0,0>() + cdg1*a.template at<-1,0,0>() + cdg0*a.template at<0,0,0>()
                 + cdg1*a.template at<1,0,0>() + cdg2*a.template at<2,0,0>() + cdg3*a.template at<3,0,0>())*dxidxi;
    d[1] = TF(0);
    if (dim3)
        d[1] = visc * (cdg3*a.template at<0,-3,0>() + cdg2*a.template at<0,-2,0>() + cdg1*a.template at<0,-1,0>() + cdg0*a.template at<0,0,0>()
                     + cdg1*a.template at<0,1,0>() + cdg2*a.template at<0,2,0>() + cdg3*a.template at<0,3,0>())*dyidyi;
    TF g0, g1, g2;
    if (fresh)
    {
        g0 = bot ? bg4<TF>(a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>())
                 : cg4<TF>(a.template at<0,0,-3>(), a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>());
        g1 = cg4<TF>(a.template at<0,0,-2>(), a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>());
        g2 = cg4<TF>(a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>());
    }
    else { g0 = c[0]; g1 = c[1]; g2 = c[2]; }
    const TF g3 = top ? tg4<TF>(a.template at<0,0,-1>(), a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>())
                      : cg4<TF>(a.template at<0,0,0>(), a.template at<0,0,1>(), a.template at<0,0,2>(), a.template at<0,0,3>());
    d[2] = visc * ( cg0*g0 * g4[0] + cg1*g1 * g4[1] + cg2*g2 * g4[2] + cg3*g3 * g4[3] ) * go;
    c[0] = g1; c[1] = g2; c[2] = g3;
}
template<class TF>
MHH_HD void diff4_cell(TF d[3], const TF* __restrict__ a, int c, int jj, int kk, bool bot, bool top, TF visc,
                       TF dxidxi, TF dyidyi, const TF g4[4], TF go, bool dim3)
{
    const GlobalView<TF> av{a, c, jj, kk};
    diff4_v(d, av, bot, top, visc, dxidxi, dyidyi, g4, go, dim3);
}

// =======================================================================================================
// diff_smag2 (src/diff_smag2.cxx)
// =======================================================================================================
// calc_strain2 (:47-155); mo = surface model active on this (lowest) level
template<class TF>
MHH_HD TF smag_strain2(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, int c, int jj, int kk,
                       bool mo, TF ugradbot, TF vgradbot, TF dxi, TF dyi, TF dzi_k, TF dzhi_k, TF dzhi_kp)
{
    TF acc = sq((u[c+1]-u[c])*dxi);
    acc = acc + sq((v[c+jj]-v[c])*dyi);
    acc = acc + sq((w[c+kk]-w[c])*dzi_k);
    acc = acc + TF(0.125)*sq((u[c      ]-u[c  -jj])*dyi + (v[c      ]-v[c-1   ])*dxi);
    acc = acc + TF(0.125)*sq((u[c+1    ]-u[c+1-jj])*dyi + (v[c+1    ]-v[c     ])*dxi);
    acc = acc + TF(0.125)*sq((u[c  +jj ]-u[c      ])*dyi + (v[c  +jj]-v[c-1+jj])*dxi);
    acc = acc + TF(0.125)*sq((u[c+1+jj ]-u[c+1    ])*dyi + (v[c+1+jj]-v[c  +jj])*dxi);
    if (mo)
    {
        acc = acc + TF(0.5)*sq(ugradbot);
        acc = acc + TF(0.125)*sq((w[c      ]-w[c-1   ])*dxi);
        acc = acc + TF(0.125)*sq((w[c+1    ]-w[c     ])*dxi);
        acc = acc + TF(0.125)*sq((w[c  +kk ]-w[c-1+kk])*dxi);
        acc = acc + TF(0.125)*sq((w[c+1+kk ]-w[c  +kk])*dxi);
        acc = acc + TF(0.5)*sq(vgradbot);
        acc = acc + TF(0.125)*sq((w[c      ]-w[c-jj   ])*dyi);
        acc = acc + TF(0.125)*sq((w[c+jj   ]-w[c      ])*dyi);
        acc = acc + TF(0.125)*sq((w[c   +kk]-w[c-jj+kk])*dyi);
        acc = acc + TF(0.125)*sq((w[c+jj+kk]-w[c   +kk])*dyi);
    }
    else
    {
        acc = acc + TF(0.125)*sq((u[c      ]-u[c  -kk])*dzhi_k  + (w[c      ]-w[c-1   ])*dxi);
        acc = acc + TF(0.125)*sq((u[c+1    ]-u[c+1-kk])*dzhi_k  + (w[c+1    ]-w[c     ])*dxi);
        acc = acc + TF(0.125)*sq((u[c  +kk ]-u[c     ])*dzhi_kp + (w[c  +kk ]-w[c-1+kk])*dxi);
        acc = acc + TF(0.125)*sq((u[c+1+kk ]-u[c+1   ])*dzhi_kp + (w[c+1+kk ]-w[c  +kk])*dxi);
        acc = acc + TF(0.125)*sq((v[c      ]-v[c   -kk])*dzhi_k  + (w[c      ]-w[c-jj   ])*dyi);
        acc = acc + TF(0.125)*sq((v[c+jj   ]-v[c+jj-kk])*dzhi_k  + (w[c+jj   ]-w[c      ])*dyi);
        acc = acc + TF(0.125)*sq((v[c   +kk]-v[c      ])*dzhi_kp + (w[c   +kk]-w[c-jj+kk])*dyi);
        acc = acc + TF(0.125)*sq((v[c+jj+kk]-v[c+jj   ])*dzhi_kp + (w[c+jj+kk]-w[c   +kk])*dyi);
    }
    TF s2 = TF(2.)*acc;
    s2 += 1.e-9;          // Constants::dsmall is a double: promoted add, narrowed on store
    return s2;
}

// evisc from strain^2 (calc_evisc / calc_evisc_neutral, src/diff_smag2.cxx:157-367, the surface-model branches and the
// plain Smagorinsky length for resolved walls): pow(x, 2) and pow(y, 1/2) are evaluated as x*x and sqrt(y).
MHH_HD double dsqrt2(double x) { return __builtin_sqrt(x); }
MHH_HD float  dsqrt2(float x)  { return __builtin_sqrtf(x); }
// the squared mixing length: depends on the level and the column's roughness length only (three divisions and a square root
// per cell in fp64) -- for a horizontally uniform z0m it is a per-level table (mhh_smag2_mlen2_host, mhh_diff_params::mlen2)
template<class TF>
MHH_HD TF evisc_mlen2(int sm, int neutral, TF mlen0_k, TF z_k, TF z0m_ij)
{
    if (!sm) return sq(mlen0_k);
    if (neutral) return sq(TF(1.)/(TF(1.)/mlen0_k + TF(1.)/(TF(0.4)*(z_k+z0m_ij))));
    return sq(dsqrt2(TF(1.)/(TF(1.)/sq(mlen0_k) + TF(1.)/sq(TF(0.4)*(z_k+z0m_ij)))));
}
template<class TF>
MHH_HD TF evisc_from_mlen2(TF fac, TF s2, TF n2, int neutral, TF tPr)
{
    if (neutral) return fac * dsqrt2(s2);
    TF rit = n2 / s2 / tPr;
    rit = tmin(rit, TF(1.-1.e-9));
    return fac * dsqrt2(s2) * dsqrt2(TF(1.)-rit);
}
template<class TF>
MHH_HD TF evisc_value(TF s2, TF n2, int sm, int neutral, TF mlen0_k, TF z_k, TF z0m_ij, TF tPr)
{
    return evisc_from_mlen2(evisc_mlen2(sm, neutral, mlen0_k, z_k, z0m_ij), s2, n2, neutral, tPr);
}

// diff_u / diff_v (:369-571). fb/ft: this level takes the surface flux at the bottom / top instead of the resolved gradient.
template<class TF>
MHH_HD TF smag_diff_u(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, const TF* __restrict__ ev,
                      int c, int jj, int kk, bool fb, bool ft, TF fluxbot, TF fluxtop, TF visc, TF dxi, TF dyi,
                      TF rhk, TF rhkp, TF rk, TF dzi_k, TF dzhi_k, TF dzhi_kp)
{
    const TF ee = ev[c] + visc;
    const TF ew = ev[c-1] + visc;
    const TF en = TF(0.25)*(ev[c-1   ] + ev[c   ] + ev[c-1+jj] + ev[c+jj]) + visc;
    const TF es = TF(0.25)*(ev[c-1-jj] + ev[c-jj] + ev[c-1   ] + ev[c   ]) + visc;
    const TF hor = + ( ee*(u[c+1]-u[c  ])*dxi - ew*(u[c  ]-u[c-1])*dxi ) * TF(2.)*dxi
                   + ( en*((u[c+jj]-u[c   ])*dyi + (v[c+jj]-v[c-1+jj])*dxi)
                     - es*((u[c   ]-u[c-jj])*dyi + (v[c   ]-v[c-1   ])*dxi) ) * dyi;
    TF ver;
    if (fb)
    {
        const TF et = TF(0.25)*(ev[c-1] + ev[c] + ev[c-1+kk] + ev[c+kk]) + visc;
        ver = ( rhkp * et*((u[c+kk]-u[c])*dzhi_kp + (w[c+kk]-w[c-1+kk])*dxi) + rhk * fluxbot ) / rk * dzi_k;
    }
    else if (ft)
    {
        const TF eb = TF(0.25)*(ev[c-1-kk] + ev[c-kk] + ev[c-1] + ev[c]) + visc;
        ver = ( - rhkp * fluxtop - rhk * eb*((u[c]-u[c-kk])*dzhi_k + (w[c]-w[c-1])*dxi) ) / rk * dzi_k;
    }
    else
    {
        const TF et = TF(0.25)*(ev[c-1   ] + ev[c   ] + ev[c-1+kk] + ev[c+kk]) + visc;
        const TF eb = TF(0.25)*(ev[c-1-kk] + ev[c-kk] + ev[c-1   ] + ev[c   ]) + visc;
        ver = ( rhkp * et*((u[c+kk]-u[c   ])*dzhi_kp + (w[c+kk]-w[c-1+kk])*dxi)
              - rhk  * eb*((u[c   ]-u[c-kk])*dzhi_k  + (w[c   ]-w[c-1   ])*dxi) ) / rk * dzi_k;
    }
    return hor + ver;
}
template<class TF>
MHH_HD TF smag_diff_v(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, const TF* __restrict__ ev,
                      int c, int jj, int kk, bool fb, bool ft, TF fluxbot, TF fluxtop, TF visc, TF dxi, TF dyi,
                      TF rhk, TF rhkp, TF rk, TF dzi_k, TF dzhi_k, TF dzhi_kp)
{
    const TF ee = TF(0.25)*(ev[c  -jj] + ev[c  ] + ev[c+1-jj] + ev[c+1]) + visc;
    const TF ew = TF(0.25)*(ev[c-1-jj] + ev[c-1] + ev[c  -jj] + ev[c  ]) + visc;
    const TF en = ev[c] + visc;
    const TF es = ev[c-jj] + visc;
    const TF hor = + ( ee*((v[c+1]-v[c  ])*dxi + (u[c+1]-u[c+1-jj])*dyi)
                     - ew*((v[c  ]-v[c-1])*dxi + (u[c  ]-u[c  -jj])*dyi) ) * dxi
                   + ( en*(v[c+jj]-v[c   ])*dyi - es*(v[c   ]-v[c-jj])*dyi ) * TF(2.)*dyi;
    TF ver;
    if (fb)
    {
        const TF et = TF(0.25)*(ev[c-jj] + ev[c] + ev[c+kk-jj] + ev[c+kk]) + visc;
        ver = ( rhkp * et*((v[c+kk]-v[c])*dzhi_kp + (w[c+kk]-w[c-jj+kk])*dyi) + rhk * fluxbot ) / rk * dzi_k;
    }
    else if (ft)
    {
        const TF eb = TF(0.25)*(ev[c-kk-jj] + ev[c-kk] + ev[c-jj] + ev[c]) + visc;
        ver = ( - rhkp * fluxtop - rhk * eb*((v[c]-v[c-kk])*dzhi_k + (w[c]-w[c-jj])*dyi) ) / rk * dzi_k;
    }
    else
    {
        const TF et = TF(0.25)*(ev[c   -jj] + ev[c   ] + ev[c+kk-jj] + ev[c+kk]) + visc;
        const TF eb = TF(0.25)*(ev[c-kk-jj] + ev[c-kk] + ev[c   -jj] + ev[c   ]) + visc;
        ver = ( rhkp * et*((v[c+kk]-v[c   ])*dzhi_kp + (w[c+kk]-w[c-jj+kk])*dyi)
              - rhk  * eb*((v[c   ]-v[c-kk])*dzhi_k  + (w[c   ]-w[c-jj   ])*dyi) ) / rk * dzi_k;
    }
    return hor + ver;
}
// diff_w (:573-617): rk=rhoref[k] rkm=rhoref[k-1] rhk=rhorefh[k]
template<class TF>
MHH_HD TF smag_diff_w(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, const TF* __restrict__ ev,
                      int c, int jj, int kk, TF visc, TF dxi, TF dyi, TF rk, TF rkm, TF rhk, TF dzi_k, TF dzi_km, TF dzhi_k)
{
    const TF ee = TF(0.25)*(ev[c   -kk] + ev[c   ] + ev[c+1 -kk] + ev[c+1 ]) + visc;
    const TF ew = TF(0.25)*(ev[c-1 -kk] + ev[c-1 ] + ev[c   -kk] + ev[c   ]) + visc;
    const TF en = TF(0.25)*(ev[c   -kk] + ev[c   ] + ev[c+jj-kk] + ev[c+jj]) + visc;
    const TF es = TF(0.25)*(ev[c-jj-kk] + ev[c-jj] + ev[c   -kk] + ev[c   ]) + visc;
    const TF et = ev[c] + visc;
    const TF eb = ev[c-kk] + visc;
    return
        + ( ee*((w[c+1]-w[c  ])*dxi + (u[c+1]-u[c+1-kk])*dzhi_k)
          - ew*((w[c  ]-w[c-1])*dxi + (u[c  ]-u[c  -kk])*dzhi_k) ) * dxi
        + ( en*((w[c+jj]-w[c   ])*dyi + (v[c+jj]-v[c+jj-kk])*dzhi_k)
          - es*((w[c   ]-w[c-jj])*dyi + (v[c   ]-v[c   -kk])*dzhi_k) ) * dyi
        + ( rk  * et*(w[c+kk]-w[c   ])*dzi_k
          - rkm * eb*(w[c   ]-w[c-kk])*dzi_km ) / rhk * TF(2.)*dzhi_k;
}
// diff_c (:619-709)
template<class TF>
MHH_HD TF smag_diff_c(const TF* __restrict__ a, const TF* __restrict__ ev, int c, int jj, int kk, bool fb, bool ft,
                      TF fluxbot, TF fluxtop, TF tPr, TF visc, TF dxidxi, TF dyidyi,
                      TF rhk, TF rhkp, TF rk, TF dzi_k, TF dzhi_k, TF dzhi_kp)
{
    const TF ee = TF(0.5)*(ev[c   ]+ev[c+1 ])/tPr + visc;
    const TF ew = TF(0.5)*(ev[c-1 ]+ev[c   ])/tPr + visc;
    const TF en = TF(0.5)*(ev[c   ]+ev[c+jj])/tPr + visc;
    const TF es = TF(0.5)*(ev[c-jj]+ev[c   ])/tPr + visc;
    const TF hor = + ( ee*(a[c+1 ]-a[c]) - ew*(a[c]-a[c-1 ]) ) * dxidxi
                   + ( en*(a[c+jj]-a[c]) - es*(a[c]-a[c-jj]) ) * dyidyi;
    TF ver;
    if (fb)
    {
        const TF et = TF(0.5)*(ev[c]+ev[c+kk])/tPr + visc;
        ver = ( rhkp * et*(a[c+kk]-a[c])*dzhi_kp + rhk * fluxbot ) / rk * dzi_k;
    }
    else if (ft)
    {
        const TF eb = TF(0.5)*(ev[c-kk]+ev[c])/tPr + visc;
        ver = ( -rhkp * fluxtop - rhk * eb*(a[c]-a[c-kk])*dzhi_k ) / rk * dzi_k;
    }
    else
    {
        const TF et = TF(0.5)*(ev[c   ]+ev[c+kk])/tPr + visc;
        const TF eb = TF(0.5)*(ev[c-kk]+ev[c   ])/tPr + visc;
        ver = ( rhkp * et*(a[c+kk]-a[c   ])*dzhi_kp
              - rhk  * eb*(a[c   ]-a[c-kk])*dzhi_k ) / rk * dzi_k;
    }
    return hor + ver;
}

// =======================================================================================================
// pres_2 / pres_4 pointwise pieces
// =======================================================================================================
// Pres_2::input integrand (src/pres_2.cxx:185-195)
template<class TF>
MHH_HD TF pres2_in(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                   const TF* __restrict__ ut, const TF* __restrict__ vt, const TF* __restrict__ wt,
                   int c, int jj, int kk, TF dxi, TF dyi, TF dti, TF rk, TF rhk, TF rhkp, TF dzi_k)
{
    return rk * ( (ut[c+1 ] + u[c+1 ] * dti) - (ut[c] + u[c] * dti) ) * dxi
         + rk * ( (vt[c+jj] + v[c+jj] * dti) - (vt[c] + v[c] * dti) ) * dyi
         + ( rhkp * (wt[c+kk] + w[c+kk] * dti)
           - rhk  * (wt[c   ] + w[c   ] * dti) ) * dzi_k;
}
// Pres_4::input integrand (src/pres_4.cxx:305-316); wtm/wtp2 etc. read through the pointers (ghosts set by caller)
template<class TF>
MHH_HD TF pres4_in(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w,
                   const TF* __restrict__ ut, const TF* __restrict__ vt, const TF* __restrict__ wt,
                   int c, int jj, int kk, TF dxi, TF dyi, TF dti, TF dzi4_k, bool dim3)
{
    TF p = cg4(ut[c-1] + u[c-1]*dti, ut[c] + u[c]*dti, ut[c+1] + u[c+1]*dti, ut[c+2] + u[c+2]*dti) * dxi;
    if (dim3)
        p += cg4(vt[c-jj] + v[c-jj]*dti, vt[c] + v[c]*dti, vt[c+jj] + v[c+jj]*dti, vt[c+2*jj] + v[c+2*jj]*dti) * dyi;
    p += cg4(wt[c-kk] + w[c-kk]*dti, wt[c] + w[c]*dti, wt[c+kk] + w[c+kk]*dti, wt[c+2*kk] + w[c+2*kk]*dti) * dzi4_k;
    return p;
}
// divergence integrands (src/pres_2.cxx:411-415, src/pres_4.cxx:755-759)
template<class TF>
MHH_HD TF div2_cell(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, int c, int jj, int kk,
                    TF dxi, TF dyi, TF rk, TF rhk, TF rhkp, TF dzi_k)
{
    return rk*((u[c+1]-u[c])*dxi + (v[c+jj]-v[c])*dyi) + (rhkp*w[c+kk]-rhk*w[c])*dzi_k;
}
template<class TF>
MHH_HD TF div4_cell(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ w, int c, int jj, int kk,
                    TF dxi, TF dyi, TF dzi4_k)
{
    return cg4(u[c-1], u[c], u[c+1], u[c+2]) * dxi + cg4(v[c-jj], v[c], v[c+jj], v[c+2*jj]) * dyi
         + cg4(w[c-kk], w[c], w[c+kk], w[c+2*kk]) * dzi4_k;
}

// =======================================================================================================
// Buffer (src/buffer.cxx:37-58) and Force (src/force.cxx:46-305): one function per reference kernel body. Each returns what
// the reference adds to (or, where named _sub, subtracts from) ONE tendency cell; per-level values arrive as arguments.
// =======================================================================================================
// calc_buffer (src/buffer.cxx:55): at -= sigmaz*(a - abuf[k])
template<class TF> MHH_HD TF buffer_sub(TF sigmaz, TF a, TF abuf_k) { return sigmaz*(a - abuf_k); }
// enforce_fixed_flux (src/force.cxx:71): the body force from the two volume means, all operands TF
template<class TF> MHH_HD TF force_fixed_flux_body(TF u_flux, TF u_mean, TF ut_mean, TF u_grid, TF dt) { return (u_flux - u_mean - u_grid) / dt - ut_mean; }
// Field3d_operators::calc_mean (src/field3d_operators.cxx:152): the double sum over the TF denominator itot*jtot*zsize
template<class TF> MHH_HD TF mean_of_sum(double sum, TF den) { return TF(sum / den); }
// calc_coriolis_2nd (src/force.cxx:96,105): ut += coriolis2_u, vt -= coriolis2_v
template<class TF> MHH_HD TF coriolis2_u(const TF* __restrict__ v, int c, int jj, TF fc, TF vgrid, TF vg_k)
{ return fc * (TF(0.25)*(v[c-1] + v[c] + v[c-1+jj] + v[c+jj]) + vgrid - vg_k); }
template<class TF> MHH_HD TF coriolis2_v(const TF* __restrict__ u, int c, int jj, TF fc, TF ugrid, TF ug_k)
{ return fc * (TF(0.25)*(u[c-jj] + u[c] + u[c+1-jj] + u[c+1]) + ugrid - ug_k); }
// calc_coriolis_4th (src/force.cxx:132-136,145-149): ci0*(ci0*a + ci1*b + ci2*c + ci3*d) + ci1*(...) + ..., 16 points
template<class TF> MHH_HD TF coriolis4_u(const TF* __restrict__ v, int c, int jj, TF fc, TF vgrid, TF vg_k)
{
    return fc * ( ci4( ci4(v[c-2-jj  ], v[c-1-jj  ], v[c-jj  ], v[c+1-jj  ]),
                       ci4(v[c-2     ], v[c-1     ], v[c     ], v[c+1     ]),
                       ci4(v[c-2+jj  ], v[c-1+jj  ], v[c+jj  ], v[c+1+jj  ]),
                       ci4(v[c-2+2*jj], v[c-1+2*jj], v[c+2*jj], v[c+1+2*jj]) )
                + vgrid - vg_k );
}
template<class TF> MHH_HD TF coriolis4_v(const TF* __restrict__ u, int c, int jj, TF fc, TF ugrid, TF ug_k)
{
    return fc * ( ci4( ci4(u[c-1-2*jj], u[c-2*jj], u[c+1-2*jj], u[c+2-2*jj]),
                       ci4(u[c-1-jj  ], u[c-jj  ], u[c+1-jj  ], u[c+2-jj  ]),
                       ci4(u[c-1     ], u[c     ], u[c+1     ], u[c+2     ]),
                       ci4(u[c-1+jj  ], u[c+jj  ], u[c+1+jj  ], u[c+2+jj  ]) )
                + ugrid - ug_k );
}
// advec_wls_2nd_mean (src/force.cxx:216-232): st -= wls[k]*(s[k]-s[k-1])*dzhi[k] (wls[k] > 0) or wls[k]*(s[k+1]-s[k])*dzhi[k+1];
// s is the mean PROFILE
template<class TF> MHH_HD TF wls_mean_sub(TF sm_km, TF sm_k, TF sm_kp, TF wls_k, TF dzhi_k, TF dzhi_kp)
{ return (wls_k > 0.) ? wls_k * (sm_k-sm_km)*dzhi_k : wls_k * (sm_kp-sm_k)*dzhi_kp; }
// advec_wls_2nd_local (src/force.cxx:250-266): the same on the field
template<class TF> MHH_HD TF wls_local_sub(const TF* __restrict__ s, int c, int kk, TF wls_k, TF dzhi_k, TF dzhi_kp)
{ return (wls_k > 0.) ? wls_k * (s[c]-s[c-kk])*dzhi_k : wls_k * (s[c+kk]-s[c])*dzhi_kp; }
// advec_wls_2nd_local_w (src/force.cxx:284-302), k in (kstart, kend): wl = interp2(wls[k-1], wls[k]), dzi[k-1] or dzi[k]
template<class TF> MHH_HD TF wls_local_w_sub(const TF* __restrict__ w, int c, int kk, TF wls_km, TF wls_k, TF dzi_km, TF dzi_k)
{ return (i2(wls_km, wls_k) > 0.) ? i2(wls_km, wls_k) * (w[c]-w[c-kk])*dzi_km : i2(wls_km, wls_k) * (w[c+kk]-w[c])*dzi_k; }
// calc_nudging_tendency (src/force.cxx:183): formed once per level, then added
template<class TF> MHH_HD TF nudge_tend(TF factor_k, TF mean_k, TF ref_k) { return -factor_k * (mean_k - ref_k); }

// =======================================================================================================
// Boundary_surface: the Monin-Obukhov surface layer (include/monin_obukhov.h:42-150, include/boundary_surface_kernels.h:136-284,
// src/boundary_surface.cxx:54-339). pow, log and exp are CALLS of the math library (the reference's std::pow(x, TF(0.5)) is
// not a square root), every product and quotient keeps the reference's association.
// =======================================================================================================
constexpr int SURF_NZL = 10000;                                     // nzL_lut (include/boundary.h:55)
template<class TF> MHH_HD TF most_kappa() { return TF(0.4); }       // Constants::kappa<TF>
// gradient functions: Wilson (2001) on the unstable side, the IFS forms on the stable side (monin_obukhov.h:42-86)
template<class TF> MHH_HD TF most_phim_unstable(TF zeta) { return std::pow(TF(1.) + TF(3.6)*std::pow(tabs(zeta), TF(2./3.)), TF(-1./2.)); }
template<class TF> MHH_HD TF most_phih_unstable(TF zeta) { return std::pow(TF(1.) + TF(7.9)*std::pow(tabs(zeta), TF(2./3.)), TF(-1./2.)); }
template<class TF> MHH_HD TF most_phim(TF zeta) { return (zeta <= TF(0.)) ? most_phim_unstable(zeta) : TF(1) + TF(5)*zeta; }
template<class TF> MHH_HD TF most_phih(TF zeta) { return (zeta <= TF(0.)) ? most_phih_unstable(zeta) : sq(TF(1) + TF(4)*zeta); }
// integrated functions (monin_obukhov.h:91-134); a = 1, b = 2/3 (a TF quotient), c = 5, d = 0.35
template<class TF> MHH_HD TF most_psim_unstable(TF zeta) { return TF(3.)*std::log( ( TF(1.) + TF(1.)/most_phim_unstable(zeta) ) / TF(2.)); }
template<class TF> MHH_HD TF most_psih_unstable(TF zeta) { return TF(3.) * std::log( ( TF(1.) + TF(1.) / most_phih_unstable(zeta) ) / TF(2.)); }
template<class TF> MHH_HD TF most_psim_stable(TF zeta)
{
    const TF a = TF(1), b = TF(2)/TF(3), c = TF(5), d = TF(0.35);
    return -b * (zeta - (c/d)) * std::exp(-d * zeta) - a*zeta - (b*c)/d;
}
template<class TF> MHH_HD TF most_psih_stable(TF zeta)
{
    const TF a = TF(1), b = TF(2)/TF(3), c = TF(5), d = TF(0.35);
    return -b * (zeta - (c/d)) * std::exp(-d * zeta) - std::pow(TF(1)+ b*a*zeta, TF(1.5)) -(b*c)/d + TF(1);
}
// fm, fh (monin_obukhov.h:136-150)
template<class TF> MHH_HD TF most_fm(TF zsl, TF z0m, TF L)
{
    return (L <= TF(0.))
        ? most_kappa<TF>() / (std::log(zsl/z0m) - most_psim_unstable(zsl/L) + most_psim_unstable(z0m/L))
        : most_kappa<TF>() / (std::log(zsl/z0m) - most_psim_stable  (zsl/L) + most_psim_stable  (z0m/L));
}
template<class TF> MHH_HD TF most_fh(TF zsl, TF z0h, TF L)
{
    return (L <= TF(0.))
        ? most_kappa<TF>() / (std::log(zsl/z0h) - most_psih_unstable(zsl/L) + most_psih_unstable(z0h/L))
        : most_kappa<TF>() / (std::log(zsl/z0h) - most_psih_stable  (zsl/L) + most_psih_stable  (z0h/L));
}

// calc_dutot (boundary_surface_kernels.h:164-179): the filtered wind at the scalar point against the surface values,
// floored at 0.1; c = the cell at kstart, ij its column. Reads u[i-1..i+2], v[j-1..j+2]: igc >= 2 and jgc >= 2.
template<class TF> MHH_HD TF surf_dutot(const TF* __restrict__ u, const TF* __restrict__ v, const TF* __restrict__ ubot, const TF* __restrict__ vbot,
                                        int c, int ij, int jj)
{
    const int ii = 1, ii2 = 2, jj2 = 2*jj;
    const TF minval = 1.e-1;
    const TF u_filtered = TF(1./9) *
        ( TF(0.5)*u[c-ii-jj] + u[c-jj] + u[c+ii-jj] + TF(0.5)*u[c+ii2-jj]
        + TF(0.5)*u[c-ii   ] + u[c   ] + u[c+ii   ] + TF(0.5)*u[c+ii2   ]
        + TF(0.5)*u[c-ii+jj] + u[c+jj] + u[c+ii+jj] + TF(0.5)*u[c+ii2+jj] );
    const TF v_filtered = TF(1./9) *
        ( TF(0.5)*v[c-ii-jj] + v[c-ii] + v[c-ii+jj] + TF(0.5)*v[c-ii+jj2]
        + TF(0.5)*v[c   -jj] + v[c   ] + v[c   +jj] + TF(0.5)*v[c   +jj2]
        + TF(0.5)*v[c+ii-jj] + v[c+ii] + v[c+ii+jj] + TF(0.5)*v[c+ii+jj2] );
    const TF du2 = sq(u_filtered - TF(0.5)*(ubot[ij] + ubot[ij+ii]))
                 + sq(v_filtered - TF(0.5)*(vbot[ij] + vbot[ij+jj]));
    return tmax(std::pow(du2, TF(0.5)), minval);
}

// find_zL (boundary_surface_kernels.h:246-260): walk the table from the cell's stored index n, every test in float. The
// downward loop tests n > 0 BEFORE it reads f[n-1] (the reference reads f[-1] at n == 0 and then stops on `n > 0`: the same
// n wherever its result is defined). The interpolation runs in float and is widened to TF on return.
template<class TF> MHH_HD TF surf_find_zL(const float* __restrict__ zL, const float* __restrict__ f, int& n, const float Ri)
{
    if ( (f[n]-Ri) > 0.f )
        while ( n > 0 && (f[n-1]-Ri) > 0.f ) { --n; }
    else
        while ( (f[n]-Ri) < 0.f && n < (SURF_NZL-1) ) { ++n; }
    const TF zL0 = (n == 0 || n == SURF_NZL-1) ? zL[n] : zL[n-1] + (Ri-f[n-1]) / (f[n]-f[n-1]) * (zL[n]-zL[n-1]);
    return zL0;
}
// calc_obuk_noslip_flux_lookup / _dirichlet_lookup (:262-284): Ri formed in TF, narrowed to float
template<class TF> MHH_HD TF surf_obuk_flux(const float* __restrict__ zL, const float* __restrict__ f, int& n, TF du, TF bfluxbot, TF zsl)
{
    const float Ri = -most_kappa<TF>() * bfluxbot * zsl / (du*du*du);
    return zsl/surf_find_zL<TF>(zL, f, n, Ri);
}
template<class TF> MHH_HD TF surf_obuk_dirichlet(const float* __restrict__ zL, const float* __restrict__ f, int& n, TF du, TF db, TF zsl)
{
    const float Ri = most_kappa<TF>() * db * zsl / sq(du);
    const TF zL0 = surf_find_zL<TF>(zL, f, n, Ri);
    return zsl/zL0;
}
// Thermo_dry's hooks at the surface (src/thermo_dry.cxx:133-162,629-633)
template<class TF> MHH_HD TF dry_bfluxbot(TF grav, TF threfh_ks, TF thfluxbot) { return grav/threfh_ks*thfluxbot; }
template<class TF> MHH_HD TF dry_db(TF grav, TF thref_ks, TF threfh_ks, TF th, TF thbot)
{
    const TF bbot = grav/threfh_ks * (thbot - threfh_ks);
    const TF b    = grav/thref_ks  * (th    - thref_ks );
    const TF db_ref = grav/thref_ks*(thref_ks - threfh_ks);
    return b - bbot + db_ref;
}
// stability case 1 (src/boundary_surface.cxx:90): fixed ustar and fixed buoyancy flux
template<class TF> MHH_HD TF surf_obuk_ustar_flux(TF ustar, TF bfluxbot) { return -(ustar*ustar*ustar) / (most_kappa<TF>()*bfluxbot); }
// surfm, Dirichlet branch (:211-214): the flux from the stability function averaged over the two neighbouring columns;
// ijm = ij-1 for u, ij-jj for v
template<class TF> MHH_HD TF surf_mom_flux(TF a, TF abot, const TF* __restrict__ ustar, const TF* __restrict__ obuk, const TF* __restrict__ z0m,
                                           int ij, int ijm, TF zsl)
{
    return -(a-abot)*TF(0.5)*
        (ustar[ijm]*most_fm(zsl, z0m[ijm], obuk[ijm]) + ustar[ij]*most_fm(zsl, z0m[ij], obuk[ij]));
}
// surfm, Ustar branch (:234-248): ustar redistributed over the two flux components
template<class TF> MHH_HD void surf_mom_flux_ustar(TF& ufluxbot, TF& vfluxbot, const TF* __restrict__ u, const TF* __restrict__ v,
                                                   const TF* __restrict__ ubot, const TF* __restrict__ vbot, const TF* __restrict__ ustar,
                                                   int c, int ij, int jj)
{
    const int ii = 1;
    const TF minval = 1.e-2;
    const TF vonu2 = tmax(minval, TF(0.25)*(
                sq(v[c-ii]-vbot[ij-ii]) + sq(v[c-ii+jj]-vbot[ij-ii+jj])
              + sq(v[c   ]-vbot[ij   ]) + sq(v[c   +jj]-vbot[ij   +jj])) );
    const TF uonv2 = tmax(minval, TF(0.25)*(
                sq(u[c-jj]-ubot[ij-jj]) + sq(u[c+ii-jj]-ubot[ij+ii-jj])
              + sq(u[c   ]-ubot[ij   ]) + sq(u[c+ii   ]-ubot[ij+ii   ])) );
    const TF u2 = tmax(minval, sq(u[c]-ubot[ij]) );
    const TF v2 = tmax(minval, sq(v[c]-vbot[ij]) );
    const TF um = ustar[ij-ii], vm = ustar[ij-jj], us = ustar[ij];
    const TF ustaronu4 = TF(0.5)*(um*um*um*um + us*us*us*us);
    const TF ustaronv4 = TF(0.5)*(vm*vm*vm*vm + us*us*us*us);
    ufluxbot = -std::copysign(TF(1), u[c]-ubot[ij]) * std::pow(ustaronu4 / (TF(1) + vonu2 / u2), TF(0.5));
    vfluxbot = -std::copysign(TF(1), v[c]-vbot[ij]) * std::pow(ustaronv4 / (TF(1) + uonv2 / v2), TF(0.5));
}
// surfs (:316-336): the linearly interpolated gradient goes to the ghost cells, not the Monin-Obukhov one
template<class TF> MHH_HD TF surf_scalar_flux(TF var, TF varbot, TF ustar, TF obuk, TF z0h, TF zsl) { return -(var-varbot)*ustar*most_fh(zsl, z0h, obuk); }
template<class TF> MHH_HD TF surf_scalar_bot(TF var, TF varfluxbot, TF ustar, TF obuk, TF z0h, TF zsl) { return varfluxbot / (ustar*most_fh(zsl, z0h, obuk)) + var; }
template<class TF> MHH_HD TF surf_lin_grad(TF var, TF varbot, TF zsl) { return (var-varbot)/zsl; }
// calc_duvdz_mo (boundary_surface_kernels.h:214-221): d = du_c or dv_c, the velocity difference at the scalar point
template<class TF> MHH_HD TF surf_duvdz_mo(TF d, TF ustar, TF obuk, TF z0m, TF zsl)
{
    const TF fluxbot = -d * ustar * most_fm(zsl, z0m, obuk);
    return -fluxbot / (most_kappa<TF>() * zsl * ustar) * most_phim(zsl/obuk);
}
// calc_dbdz_mo (:241)
template<class TF> MHH_HD TF surf_dbdz_mo(TF bfluxbot, TF ustar, TF obuk, TF zsl) { return -bfluxbot / (most_kappa<TF>() * zsl * ustar) * most_phih(zsl/obuk); }

// ---- Thermo_moist (include/thermo_moist_functions.h), in the reference's expression order ---------------------------------------
// The constants of include/constants.h:32-42,73-83, each held in TF as the reference's variable templates hold them (Ls and ep
// are the TF sum and the TF quotient).
template<class TF> struct MoistC
{
    static constexpr TF grav = TF(9.81), Rd = TF(287.04), Rv = TF(461.5), cp = TF(1005), Lv = TF(2.501e6), Lf = TF(3.337e5);
    static constexpr TF Ls = Lv + Lf, T0 = TF(273.15), p0 = TF(1.e5), ep = Rd/Rv;
    static constexpr TF c00 = TF(+6.1121000000E+02), c10 = TF(+4.4393067270E+01), c20 = TF(+1.4279398448E+00), c30 = TF(+2.6415206946E-02),
                        c40 = TF(+3.0291749160E-04), c50 = TF(+2.1159987257E-06), c60 = TF(+7.5015702516E-09), c70 = TF(-1.5604873363E-12),
                        c80 = TF(-9.9726710231E-14), c90 = TF(-4.8165754883E-17), c100 = TF(+1.3839187032E-18);
};
// :47-75
template<class TF> MHH_HD TF moist_virtual_temperature(TF exn, TF thl, TF qt, TF ql, TF qi)
{
    typedef MoistC<TF> K;
    const TF th = thl + K::Lv*ql/(K::cp*exn) + K::Ls*qi/(K::cp*exn);
    return th * (TF(1.) - (TF(1.) - K::Rv/K::Rd)*qt - K::Rv/K::Rd*(ql+qi));
}
template<class TF> MHH_HD TF moist_buoyancy(TF exn, TF thl, TF qt, TF ql, TF qi, TF thvref)
{
    return MoistC<TF>::grav * (moist_virtual_temperature(exn, thl, qt, ql, qi) - thvref) / thvref;
}
template<class TF> MHH_HD TF moist_virtual_temperature_no_ql(TF thl, TF qt)
{
    typedef MoistC<TF> K;
    return thl * (TF(1.) - (TF(1.) - K::Rv/K::Rd)*qt);
}
template<class TF> MHH_HD TF moist_buoyancy_no_ql(TF thl, TF qt, TF thvref)
{
    typedef MoistC<TF> K;
    return K::grav * (thl * (TF(1.) - (TF(1.) - K::Rv/K::Rd)*qt) - thvref) / thvref;
}
template<class TF> MHH_HD TF moist_buoyancy_flux_no_ql(TF thl, TF thlflux, TF qt, TF qtflux, TF thvref)
{
    typedef MoistC<TF> K;
    return K::grav/thvref * (thlflux * (TF(1.) - (TF(1.)-K::Rv/K::Rd)*qt) - (TF(1.)-K::Rv/K::Rd)*thl*qtflux);
}
// :86-122: the 10th-degree Horner form of Buck's curve over water; Buck's curve over ice through exp
template<class TF> MHH_HD TF moist_esat_liq(TF T)
{
    typedef MoistC<TF> K;
    const TF x = tmax(TF(-75.), T-K::T0);
    return K::c00+x*(K::c10+x*(K::c20+x*(K::c30+x*(K::c40+x*(K::c50+x*(K::c60+x*(K::c70+x*(K::c80+x*(K::c90+x*K::c100)))))))));
}
template<class TF> MHH_HD TF moist_qsat_liq(TF p, TF T)
{
    typedef MoistC<TF> K;
    return K::ep*moist_esat_liq(T)/(p-(TF(1.)-K::ep)*moist_esat_liq(T));
}
template<class TF> MHH_HD TF moist_esat_ice(TF T)
{
    const TF x = tmax(TF(-100.), T-MoistC<TF>::T0);
    return TF(611.15)*std::exp(TF(22.452)*x / (TF(272.55)+x));
}
template<class TF> MHH_HD TF moist_qsat_ice(TF p, TF T)
{
    typedef MoistC<TF> K;
    return K::ep*moist_esat_ice(T)/(p-(TF(1.)-K::ep)*moist_esat_ice(T));
}
// :126-141 (Tomita 2008)
template<class TF> MHH_HD TF moist_water_fraction(TF T)
{
    return tmax(TF(0.), tmin((T - TF(233.15)) / (MoistC<TF>::T0 - TF(233.15)), TF(1.)));
}
template<class TF> MHH_HD TF moist_qsat(TF p, TF T)
{
    const TF alpha = moist_water_fraction(T);
    return alpha*moist_qsat_liq(p, T) + (TF(1.)-alpha)*moist_qsat_ice(p, T);
}
// :151-162
template<class TF> MHH_HD TF moist_dqsatdT_liq(TF p, TF T)
{
    typedef MoistC<TF> K;
    const TF den = p - moist_esat_liq(T)*(TF(1.) - K::ep);
    return (K::ep/den - (TF(1.) + K::ep)*K::ep*moist_esat_liq(T)/sq(den)) * K::Lv*moist_esat_liq(T) / (K::Rv*sq(T));
}
template<class TF> MHH_HD TF moist_dqsatdT_ice(TF p, TF T)
{
    typedef MoistC<TF> K;
    const TF den = p - moist_esat_ice(T)*(TF(1.) - K::ep);
    return (K::ep/den + (TF(1.) - K::ep)*K::ep*moist_esat_ice(T)/sq(den)) * K::Ls*moist_esat_ice(T) / (K::Rv*sq(T));
}
// :172-175. The reference writes an unqualified pow: with <cmath> alone that is the C library's pow(double, double) in both
// builds, narrowed to TF on return.
template<class TF> MHH_HD TF moist_exner(TF p)
{
    typedef MoistC<TF> K;
    return TF(pow(double(p/K::p0), double(K::Rd/K::cp)));
}
// sat_adjust (:186-291). niter is returned beside the answer: where the reference throws (niter == nitermax) the caller counts the
// cell and goes on with the tenth iterate. The warm branch and everything in front of the branch hold + - * /, max and fabs only.
template<class TF> struct MoistSat { TF ql, qi, t, qs; int niter; };
constexpr int moist_nitermax = 10;
template<class TF> MHH_HD MoistSat<TF> moist_sat_adjust(TF thl, TF qt, TF p, TF exn)
{
    typedef MoistC<TF> K;
    int niter = 0;
    TF tnr_old = TF(1.e9);
    const TF tl = thl * exn;
    TF qs = moist_qsat_liq(p, tl);
    MoistSat<TF> ans = {TF(0.), TF(0.), tl, qs, 0};
    if (qt-ans.qs <= TF(0.))
        return ans;
    TF tnr = tl;
    if (tl >= K::T0)
    {
        while (tabs(tnr-tnr_old)/tnr_old > TF(1.e-5) && niter < moist_nitermax)
        {
            ++niter;
            tnr_old = tnr;
            qs = moist_qsat_liq(p, tnr);
            const TF f = tnr - tl - K::Lv/K::cp*(qt - qs);
            const TF f_prime = TF(1.) + K::Lv/K::cp*moist_dqsatdT_liq(p, tnr);
            tnr -= f / f_prime;
        }
        qs = moist_qsat_liq(p, tnr);
        ans.ql = tmax(TF(0.), qt - qs);
        ans.t  = tnr;
        ans.qs = qs;
    }
    else
    {
        while (tabs(tnr-tnr_old)/tnr_old > TF(1.e-5) && niter < moist_nitermax)
        {
            ++niter;
            tnr_old = tnr;
            qs = moist_qsat(p, tnr);
            const TF alpha_w = moist_water_fraction(tnr);
            const TF alpha_i = TF(1.) - alpha_w;
            const TF dalphadT = (alpha_w > TF(0.) && alpha_w < TF(1.)) ? TF(0.025) : TF(0.);
            const TF dqsatdT_w = moist_dqsatdT_liq(p, tnr);
            const TF dqsatdT_i = moist_dqsatdT_ice(p, tnr);
            const TF f =
                tnr - tl - alpha_w*K::Lv/K::cp*qt - alpha_i*K::Ls/K::cp*qt
                         + alpha_w*K::Lv/K::cp*qs + alpha_i*K::Ls/K::cp*qs;
            const TF f_prime = TF(1.)
                - dalphadT*K::Lv/K::cp*qt + dalphadT*K::Ls/K::cp*qt
                + dalphadT*K::Lv/K::cp*qs - dalphadT*K::Ls/K::cp*qs
                + alpha_w*K::Lv/K::cp*dqsatdT_w
                + alpha_i*K::Ls/K::cp*dqsatdT_i;
            tnr -= f / f_prime;
        }
        const TF alpha_w = moist_water_fraction(tnr);
        const TF alpha_i = TF(1.) - alpha_w;
        qs = moist_qsat(p, tnr);
        const TF ql_qi = tmax(TF(0.), qt - qs);
        ans.ql = alpha_w*ql_qi;
        ans.qi = alpha_i*ql_qi;
        ans.t  = tnr;
        ans.qs = qs;
    }
    ans.niter = niter;
    return ans;
}

// ---- Microphys_2mom_warm (src/microphys_2mom_warm.cxx, include/microphys_2mom_warm.h; Seifert & Beheng 2006, Stevens & Seifert
// 2008), in the reference's expression order. pow, exp and sqrt are the unqualified calls the reference writes.
// Micro_2mom_warm_constants (include/microphys_2mom_warm.h:52-68): each a double literal narrowed to TF, pirhow the TF quotient.
template<class TF> struct MicroC
{
    static constexpr TF pi = TF(3.14159265359), K_t = TF(2.5e-2), D_v = TF(3.e-5), rho_w = TF(1.e3), rho_0 = TF(1.225);
    static constexpr TF pirhow = pi*rho_w/TF(6.), mr_min = TF(2.6e-10), mr_max = TF(3e-6), ql_min = TF(1.e-6), qr_min = TF(1.e-15);
    static constexpr double dsmall = 1.e-9;                   // include/constants.h:97: a double in both builds
};
// the process mask of mhh_micro_params (include/mhh_hip.h)
constexpr int MICRO_AUTO = 1, MICRO_ACCR = 2, MICRO_EVAP = 4, MICRO_SCBR = 8, MICRO_SEDI = 16, MICRO_CLIP = 32;
constexpr int MICRO_LOCAL = MICRO_AUTO | MICRO_ACCR | MICRO_EVAP | MICRO_SCBR;
// :76-117
template<class TF> MHH_HD TF micro_tanh2(TF x) { return x * (TF(27) + x * x) / (TF(27) + TF(9) * x * x); }
template<class TF> MHH_HD TF micro_rain_mass(TF qr, TF nr, TF rho)
{
    const TF mr = rho * qr / tmax(nr, TF(1.));
    return tmin(tmax(mr, MicroC<TF>::mr_min), MicroC<TF>::mr_max);
}
template<class TF> MHH_HD TF micro_rain_diameter(TF mr) { return pow(mr/MicroC<TF>::pirhow, TF(1.)/TF(3.)); }
template<class TF> MHH_HD TF micro_mu_r(TF dr) { return TF(10) * (TF(1) + micro_tanh2(TF(1200) * (dr - TF(0.0015)))); }
template<class TF> MHH_HD TF micro_lambda_r(TF mur, TF dr) { return pow((mur+3)*(mur+2)*(mur+1), TF(1.)/TF(3.)) / dr; }
// :120-127: copysign(1, a) is exact, so the precision it is multiplied in does not show
template<class TF> MHH_HD TF micro_minmod(TF a, TF b)
{
    const TF s = TF(__builtin_copysign(1., double(a)));
    return s * tmax(TF(0.), tmin(tabs(a), s*b));
}
// prepare_microphysics_slice (src/microphys_2mom_warm.cxx:243-275): zeros where qr <= qr_min
template<class TF> struct MicroRain { TF mr, dr, mur, lambdar; };
template<class TF> MHH_HD MicroRain<TF> micro_rain(TF qr, TF nr, TF rho)
{
    MicroRain<TF> r = {TF(0), TF(0), TF(0), TF(0)};
    if (qr > MicroC<TF>::qr_min)
    {
        r.mr = micro_rain_mass(qr, nr, rho);
        r.dr = micro_rain_diameter(r.mr);
        r.mur = micro_mu_r(r.dr);
        r.lambdar = micro_lambda_r(r.mur, r.dr);
    }
    return r;
}
// The tendencies of one cell; the kernels add the processes of the mask in the order autoconversion, accretion, evaporation,
// selfcollection, breakup, as Microphys_2mom_warm::exec's calls do per cell (:694-730).
template<class TF> struct MicroTend { TF qrt, nrt, thlt, qtt; };
// autoconversion (:94-128)
template<class TF> MHH_HD void micro_autoconversion(MicroTend<TF>& t, TF qr, TF ql, TF rho, TF exner, TF nc)
{
    typedef MicroC<TF> K;
    const TF x_star = 2.6e-10;
    const TF k_cc   = 9.44e9;
    const TF nu_c   = 1;
    const TF kccxs  = k_cc / (TF(20.) * x_star) * (nu_c+2)*(nu_c+4) / sq(nu_c+1);
    if (ql > K::ql_min)
    {
        const TF xc      = rho * ql / nc;
        const TF tau     = TF(TF(1.) - ql / (ql + qr + K::dsmall));
        const auto p68   = TF(1.) - pow(tau, TF(0.68));     // fm::pow3 deduces its type from the argument
        const TF phi_au  = TF(600.) * pow(tau, TF(0.68)) * (p68*p68*p68);
        const TF au_tend = K::rho_0 * kccxs * sq(ql) * sq(xc) *
                               (TF(1.) + phi_au / sq(TF(1.)-tau));
        t.qrt  += au_tend;
        t.nrt  += au_tend * rho / x_star;
        t.qtt  -= au_tend;
        t.thlt += MoistC<TF>::Lv / (MoistC<TF>::cp * exner) * au_tend;
    }
}
// accretion (:131-158)
template<class TF> MHH_HD void micro_accretion(MicroTend<TF>& t, TF qr, TF ql, TF rho, TF exner)
{
    typedef MicroC<TF> K;
    const TF k_cr = 5.25;
    if (ql > K::ql_min && qr > K::qr_min)
    {
        const TF tau     = TF(1.) - ql / (ql + qr);
        const TF t5      = tau / (tau + TF(5e-5));
        const TF phi_ac  = t5*t5*t5*t5;
        const TF ac_tend = k_cr * ql *  qr * phi_ac * sqrt(K::rho_0 / rho);
        t.qrt  += ac_tend;
        t.qtt  -= ac_tend;
        t.thlt += MoistC<TF>::Lv / (MoistC<TF>::cp * exner) * ac_tend;
    }
}
// evaporation (:278-318)
template<class TF> MHH_HD void micro_evaporation(MicroTend<TF>& t, TF qr, TF nr, TF ql, TF qt, TF thl, TF rho, TF exner, TF p, const MicroRain<TF>& r)
{
    typedef MicroC<TF> K; typedef MoistC<TF> M;
    const TF lambda_evap = 1.;
    if (qr > K::qr_min)
    {
        const TF mr  = r.mr;
        const TF dr  = r.dr;
        const TF T   = thl * exner + (M::Lv * ql) / (M::cp * exner);
        const TF Glv = TF(1.) / (M::Rv * T / (moist_esat_liq(T) * K::D_v) +
                           (M::Lv / (K::K_t * T)) * (M::Lv / (M::Rv * T) - TF(1.)));
        const TF S   = (qt - ql) / moist_qsat_liq(p, T) - TF(1.);
        const TF F   = 1.;
        const TF ev_tend = TF(2.) * K::pi * dr * Glv * S * F * nr / rho;
        t.qrt  += ev_tend;
        t.nrt  += lambda_evap * ev_tend * rho / mr;
        t.qtt  -= ev_tend;
        t.thlt += M::Lv / (M::cp * exner) * ev_tend;
    }
}
// selfcollection_breakup (:321-370)
template<class TF> MHH_HD void micro_selfcollection_breakup(MicroTend<TF>& t, TF qr, TF nr, TF rho, const MicroRain<TF>& r)
{
    typedef MicroC<TF> K;
    const TF k_rr     = 7.12;
    const TF kappa_rr = 60.7;
    const TF D_eq     = 0.9e-3;
    const TF k_br1    = 1.0e3;
    const TF k_br2    = 2.3e3;
    if (qr > K::qr_min)
    {
        const TF dr      = r.dr;
        const TF lambdar = r.lambdar;
        const auto a9 = TF(1.) + kappa_rr / lambdar * pow(K::pirhow, TF(1.)/TF(3.));     // fm::pow9 deduces its type from the argument
        const TF sc_tend = -k_rr * nr * qr*rho / (a9*a9*a9*a9*a9*a9*a9*a9*a9) * sqrt(K::rho_0 / rho);
        t.nrt += sc_tend;
        const TF dDr = dr - D_eq;
        if (dr > TF(0.35e-3))
        {
            TF phi_br;
            if (dr <= D_eq)
                phi_br = k_br1 * dDr;
            else
                phi_br = TF(2.) * exp(k_br2 * dDr) - TF(1.);
            const TF br_tend = -(phi_br + TF(1.)) * sc_tend;
            t.nrt += br_tend;
        }
    }
}
// The sedimentation velocities of qr (4) and nr (1): step 1 of sedimentation_ss08 (:398-419) with rho_n = sqrt(1.2/rho[k]), and
// calc_max_sedimentation_cfl's (:185-198) with rho_n = 1 left out of the expression (its a_R stands alone).
template<class TF> MHH_HD TF micro_b_R() { const TF a_R = 9.65; const TF c_R = 600; const TF Dv = 25.0e-6; return a_R * exp(c_R*Dv); }
template<class TF> MHH_HD TF micro_w_sedi(TF qr, const MicroRain<TF>& r, TF rho_n, TF b_R, TF moment)
{
    const TF w_max = 9.65; const TF a_R = 9.65; const TF c_R = 600;
    if (qr > MicroC<TF>::qr_min)
        return tmin(w_max, tmax(TF(0.1), rho_n * a_R - b_R * TF(pow(TF(1.) + c_R/r.lambdar, TF(-1.)*(r.mur+moment)))));
    return TF(0.);
}
template<class TF> MHH_HD TF micro_w_cfl(TF qr, TF nr, TF rho, TF b_R)
{
    const TF w_max = 9.65; const TF a_R = 9.65; const TF c_R = 600;
    if (qr > MicroC<TF>::qr_min)
    {
        const TF mr      = micro_rain_mass(qr, nr, rho);
        const TF dr      = micro_rain_diameter(mr);
        const TF mur     = micro_mu_r(dr);
        const TF lambdar = micro_lambda_r(mur, dr);
        return tmin(w_max, tmax(TF(0.1), a_R - b_R * TF(pow(TF(1.) + c_R/lambdar, TF(-1.)*(mur+TF(4.))))));
    }
    return TF(0.);
}
// Limiter::tendency_limiter (src/limiter.cxx:54-75): eps is the double epsilon narrowed to TF
template<class TF> MHH_HD TF limiter_increment(TF a, TF at, TF dt, TF dti)
{
    constexpr TF eps = TF(2.220446049250313e-16);
    const TF a_new = a + dt*at;
    return (a_new < TF(0.)) ? (-a_new + eps) * dti : TF(0.);
}

// ---- Radiation_gcss (src/radiation_gcss.cxx: the GCSS long- and short-wave parameterisation of DYCOMS), the CPU path, in the
// reference's expression order. std::exp, std::sqrt and std::pow are the calls the reference writes: the overload of TF in the
// device and in the emulation build. What looks like a slip there is kept and named with its line.
constexpr int RAD_LW = 1, RAD_SW = 2;
template<class TF> MHH_HD TF rad_gcss_mu_min() { return TF(0.035); }                       // include/radiation_gcss.h: mu_min
// :186, :226: the layer depth z[k] - z[km1] with km1 = max(1, k-1), a literal 1 and not kstart: depth 0 at the bottom level with
// one ghost level, the ghost z with more
template<class TF> MHH_HD TF rad_gcss_depth(const TF* __restrict__ z, int k) { const int km1 = (1 < k-1) ? k-1 : 1; return z[k] - z[km1]; }
// :227: the liquid water path accumulates max(0, .) upward
template<class TF> MHH_HD TF rad_gcss_lwp(TF lwp, TF ql, TF rho, TF depth) { return lwp + tmax(TF(0.0), ql * rho * depth); }
// :228
template<class TF> MHH_HD TF rad_gcss_flx_up(TF fr1, TF xka, TF lwp) { return fr1 * std::exp(TF(-1.0) * xka * lwp); }
// :229: the inversion index ki is the LAST level that passes this (kend where none does)
template<class TF> MHH_HD bool rad_gcss_in_pbl(TF ql, TF qt) { return (ql > TF(0.01E-3)) && (qt >= TF(0.008)); }
// :233: rho_ki = rhoref[ki], the ghost entry rhoref[kend] in a column without such a level
template<class TF> MHH_HD TF rad_gcss_fact(TF div, TF rho_ki) { return div * MoistC<TF>::cp * rho_ki; }
// :235 and :243: fr0*exp(-xka*lwp) with the column TOTAL lwp (the subtraction that would make it a path from above is commented
// out, :241-242): one value per column. At kstart it is formed with TF(-1.0), in TF; from kstart+1 up with the double literal -1.0,
// so that in fp32 the product, the exp, the product with fr0 and the sum with flx are double and narrowed at the store.
template<class TF> MHH_HD TF     rad_gcss_down_kstart(TF fr0, TF xka, TF lwp) { return fr0 * std::exp(TF(-1.0) * xka * lwp); }
template<class TF> MHH_HD double rad_gcss_down_above(TF fr0, TF xka, TF lwp)  { return fr0 * std::exp(-1.0 * xka * lwp); }
// the long-wave flux of level k from flx_up of :228; :245-248: above the inversion, with `ki > 1` a literal again and the
// exponents 1.333 and 0.33333 as written
template<class TF> MHH_HD TF rad_gcss_flx(TF flx_up, int k, int kstart, TF down_kstart, double down_above, int ki, TF fact, const TF* __restrict__ z)
{
    if (k == kstart)
        return flx_up + down_kstart;
    TF flx = TF(flx_up + down_above);
    if ((k > ki) && (ki > 1) && (fact > 0.))
        flx = flx + fact * ( TF(0.25) * std::pow(z[k]-z[ki], TF(1.333)) + z[ki] * std::pow(z[k]-z[ki], TF(0.33333)) );
    return flx;
}
// :282, :304: k in [kstart+1, kend) against km = max(kstart+1, k-1), so that kstart is untouched and kstart+1 sees a zero
// difference; dzi is the parameter's name, exec passes gd.dzhi (:369); the long-wave term goes first (tt - .), then the short-wave
// one (tt + .)
template<class TF> MHH_HD TF rad_gcss_tend(TF f, TF fm, TF dzhi, TF rho) { return (f - fm) * dzhi / (rho * MoistC<TF>::cp); }
// :188-192: ql > 1.E-5 is a DOUBLE comparison (a float ql is widened); tau is zero elsewhere, tauc their sum upward
template<class TF> MHH_HD TF rad_gcss_tau(TF ql, TF rho, TF depth)
{
    const TF rho_l = 1000.;
    const TF reff = 1.E-5;
    if (ql > 1.E-5)
        return tmax(TF(0.0), TF(1.5) * ql * rho * depth / reff / rho_l);
    return TF(0.0);
}
// sunray (:101-159), line by line: what does not depend on the level. de = 1 - omega*ff is the factor of taude[k] (:125).
template<class TF> struct RadSun { TF de, rk, rp, beta, c1, c2; };
template<class TF> MHH_HD RadSun<TF> rad_gcss_sunray(TF mu, TF tauc)
{
    TF o_c1 = TF(0.9);
    TF o_c2 = TF(2.75);
    TF o_c3 = TF(0.09);
    TF gc  = TF(0.85);
    TF sfc_albedo = TF(0.05);
    TF omega  = TF(1.) - TF(1.e-3) * (o_c1 + o_c2 * (mu+TF(1.)) * std::exp(-o_c3 * tauc));
    TF ff     = gc * gc;
    TF gcde   = gc / (TF(1.) + gc);
    TF taucde = ( TF(1.0) - omega*ff) * tauc;
    TF omegade = (TF(1.)-ff) * omega/(TF(1.) - omega*ff);
    TF x1  = TF(1.) - omegade * gcde;
    TF x2  = TF(1.) - omegade;
    TF rk  = std::sqrt(TF(3.) * x2 * x1);
    TF mu2 = mu * mu;
    TF x3  = TF(4.) * (TF(1.) - rk*rk*mu2);
    TF rp  = std::sqrt(TF(3.) * x2/x1);
    TF alpha = TF(3.) * omegade * mu2 * (TF(1.) + gcde*x2) / x3;
    TF beta  = TF(3.) * omegade * mu * (TF(1.) + TF(3.)*gcde*mu2*x2) / x3;

    TF rtt = TF(2.0/3.0);
    TF exmu0 = std::exp(-taucde / mu);
    TF expk  = std::exp(rk * taucde);
    TF exmk  = TF(1.) / expk;
    TF xp23p = TF(1.) + rtt*rp;
    TF xm23p = TF(1.) - rtt*rp;
    TF ap23b = alpha + rtt*beta;

    TF t1 = TF(1.) - sfc_albedo - rtt * (TF(1.) + sfc_albedo) * rp;
    TF t2 = TF(1.) - sfc_albedo + rtt * (TF(1.) + sfc_albedo) * rp;
    TF t3 = (TF(1.) - sfc_albedo) * alpha - rtt * (TF(1.) + sfc_albedo) * beta + sfc_albedo*mu;
    TF c2 = (xp23p*t3*exmu0 - t1*ap23b*exmk) / (xp23p*t2*expk - xm23p*t1*exmk);
    TF c1 = (ap23b - c2*xm23p)/xp23p;
    RadSun<TF> s = {TF(1.) - omega*ff, rk, rp, beta, c1, c2};
    return s;
}
// :125, :154: taude[k] is formed first and then added to taupath, going DOWN from kend-1
template<class TF> MHH_HD TF rad_gcss_taupath(const RadSun<TF>& s, TF taupath, TF tau) { const TF taude = s.de * tau; return taupath + taude; }
// :155-157
template<class TF> MHH_HD TF rad_gcss_swn(const RadSun<TF>& s, TF mu, TF taupath)
{
    TF sw0 = TF(1100.);
    return sw0 * TF(4./3.) * (s.rp * (s.c1*std::exp(-s.rk*taupath)
        - s.c2 * std::exp(s.rk*taupath)) - s.beta * std::exp(-taupath/mu))
        + mu * sw0 * std::exp(-taupath / mu);
}
// calc_zenith (:39-76), a host function evaluated with the host's C library in TF: day_of_year + 1 + lon/360. is double arithmetic
// narrowed into TF, and std::round(time2sec) in d (whole days) is kept as written.
template<class TF> inline TF rad_gcss_zenith(const TF lat, const TF lon, const double day_of_year)
{
    const TF pi    = TF(M_PI);
    const TF twopi = TF(2.*M_PI);
    const TF year2days = TF(365.);
    const TF pi_angle  = TF(180.);
    const TF z1 = TF(279.934);
    const TF z2 = TF(1.914827);
    const TF z3 = TF(0.7952);
    const TF z4 = TF(0.019938);
    const TF z5 = TF(0.00162);
    const TF z6 = TF(23.4439);
    const TF time2sec = day_of_year + 1 + lon/360.;
    const TF day = std::floor(time2sec);
    const TF lambda = lat * pi / pi_angle;
    const TF d = twopi * std::round(time2sec) / year2days;
    const TF sig = d + pi/pi_angle * (z1 + z2*std::sin(d)
                                         - z3*std::cos(d)
                                         + z4*std::sin(TF(2.)*d)
                                         - z5*std::cos(TF(2.)*d));
    const TF del = std::asin(std::sin(z6*pi / pi_angle)*std::sin(sig));
    const TF h = twopi * ((time2sec - day) - TF(0.5));
    const TF mu = std::sin(lambda) * std::sin(del) + std::cos(lambda) * std::cos(del) * std::cos(h);
    return mu;
}

// ---- Microphys_nsw6 (src/microphys_nsw6.cxx: the single-moment six-class scheme of Tomita 2008), in the reference's expression
// order. The constants of :45-113, each a double literal narrowed to TF; a_r, a_s, a_g and the two pi are double expressions
// narrowed once. Lv, Ls, Lf, cp, Rv, T0 are MoistC's.
template<class TF> struct Nsw6C
{
    static constexpr TF qv_min = TF(1.e-7), ql_min = TF(1.e-7), qi_min = TF(1.e-7), qr_min = TF(1.e-12), qs_min = TF(1.e-12), qg_min = TF(1.e-12);
    static constexpr TF q_tiny = TF(1.e-15);
    static constexpr TF pi = TF(M_PI), pi_2 = TF(M_PI*M_PI);
    static constexpr TF rho_w = TF(1.e3), rho_s = TF(1.e2), rho_g = TF(4.e2);
    static constexpr TF N_0r = TF(8.e6), N_0s = TF(3.e6), N_0g = TF(4.e6);
    static constexpr TF a_r = TF(M_PI*rho_w/6.), a_s = TF(M_PI*rho_s/6.), a_g = TF(M_PI*rho_g/6.);
    static constexpr TF b_r = TF(3.), b_s = TF(3.), b_g = TF(3.);
    static constexpr TF c_r = TF(130.), c_s = TF(4.84), c_g = TF(82.5);
    static constexpr TF d_r = TF(0.5), d_s = TF(0.25), d_g = TF(0.5);
    static constexpr TF C_l = TF(4218.);
    static constexpr TF f_1r = TF(0.78), f_1s = TF(0.65), f_1g = TF(0.78), f_2r = TF(0.27), f_2s = TF(0.39), f_2g = TF(0.27);
    static constexpr TF E_ri = TF(1.), E_rw = TF(1.), E_sw = TF(1.), E_gw = TF(1.), E_gi = TF(0.1), E_sr = TF(1.), E_gr = TF(0.1);
    static constexpr TF K_a = TF(2.43e-2), K_d = TF(2.26e-5), M_i = TF(4.19e-13);
    static constexpr TF beta_saut = TF(6.e-3), beta_gaut = TF(0.e-3);
    static constexpr TF gamma_sacr = TF(25.e-3), gamma_saut = TF(60.e-3), gamma_gacs = TF(90.e-3), gamma_gaut = TF(90.e-3);
    static constexpr TF nu = TF(1.5e-5);
    static constexpr TF V_Tmin = TF(0.1), V_Tmax = TF(10.);
};
// the process mask and the two forms of the powers (include/mhh_hip.h)
constexpr int NSW6_CONV = 1, NSW6_SEDI_R = 2, NSW6_SEDI_S = 4, NSW6_SEDI_G = 8, NSW6_ALL = 15;
constexpr int NSW6_POW = 0, NSW6_SQRT = 1;

// What the scheme holds that depends on no cell: every std::tgamma of the file (its arguments are constants of the scheme), D_d
// (:139) and the constant factors in front of a level's or a cell's values, evaluated on the HOST in TF, in the reference's order
// of operations. The kernels get it in their argument block.
template<class TF> struct Nsw6Tab
{
    TF nc_c;       // TF(3.66e-2) * TF(1.e-6)*Nc0 (:333)
    TF D_d;        // :139
    TF lam[3];     // a_x * N_0x * tgamma(b_x + 1) of r, s, g (:213-226, :717-719)
    TF g_b1;       // tgamma(b_x + 1), the same for r, s, g
    TF g_bd1[3];   // tgamma(b_x + d_x + 1)
    TF fac[7];     // fac_iacr, raci, racw, sacw, saci, gacw, gaci (:146-185) up to their `* rho0_rho_sqrt`
    TF acc[3];     // tgamma(b+1)*tgamma(3), 2*tgamma(b+2)*tgamma(2), tgamma(b+3)*tgamma(1) (:289-319; b_r == b_s)
    TF f1g2[3];    // f_1x * tgamma(2) (:381, :389, :397)
    TF g_vent[3];  // tgamma(0.5*(5 + d_x))
    TF dt;         // TF(dt) (:1005)
    // sedimentation_ss08 and calc_cfl_ss08 take a_c ... N_0c as function PARAMETERS (:695, :835), so their std::tgamma(b_c + d_c + 1)
    // is a call of the C library at run time, where conversion's arguments are constant expressions that a compiler folds (correctly
    // rounded). The two differ in the last bit for some arguments (4.5 in fp64), so the velocity keeps a value of its own, evaluated
    // through nsw6_runtime. tgamma(b_c + 1) is 3! in all three calls: exact, and folded in the reference too (b_c is the same
    // constant at every call site).
    TF sed_g_bd1[3]; // tgamma(b_c + d_c + 1) (:724)
};
template<class TF> inline TF nsw6_runtime(TF x) { volatile TF v = x; return v; }
template<class TF> inline Nsw6Tab<TF> nsw6_tab(double Nc0_in, double dt)
{
    typedef Nsw6C<TF> K;
    const TF Nc0 = TF(Nc0_in);
    Nsw6Tab<TF> H;
    H.nc_c = TF(3.66e-2) * TF(1.e-6)*Nc0;
    H.D_d = TF(0.146) - TF(5.964e-2)*std::log((Nc0*TF(1.e-6)) / TF(2.e3));
    H.lam[0] = K::a_r * K::N_0r * std::tgamma(K::b_r + TF(1.));
    H.lam[1] = K::a_s * K::N_0s * std::tgamma(K::b_s + TF(1.));
    H.lam[2] = K::a_g * K::N_0g * std::tgamma(K::b_g + TF(1.));
    H.g_b1 = std::tgamma(K::b_r + TF(1.));
    H.g_bd1[0] = std::tgamma(K::b_r + K::d_r + TF(1.));
    H.g_bd1[1] = std::tgamma(K::b_s + K::d_s + TF(1.));
    H.g_bd1[2] = std::tgamma(K::b_g + K::d_g + TF(1.));
    H.fac[0] = K::pi_2 * K::E_ri * K::N_0r * K::c_r * K::rho_w * std::tgamma(TF(6.) + K::d_r) / (TF(24.) * K::M_i);
    H.fac[1] = K::pi * K::E_ri * K::N_0r * K::c_r * std::tgamma(TF(3.) + K::d_r) / TF(4.);
    H.fac[2] = K::pi * K::E_rw * K::N_0r * K::c_r * std::tgamma(TF(3.) + K::d_r) / TF(4.);
    H.fac[3] = K::pi * K::E_sw * K::N_0s * K::c_s * std::tgamma(TF(3.) + K::d_s) / TF(4.);
    H.fac[4] = K::pi * K::N_0s * K::c_s * std::tgamma(TF(3.) + K::d_s) / TF(4.);
    H.fac[5] = K::pi * K::E_gw * K::N_0g * K::c_g * std::tgamma(TF(3.) + K::d_g) / TF(4.);
    H.fac[6] = K::pi * K::E_gi * K::N_0g * K::c_g * std::tgamma(TF(3.) + K::d_g) / TF(4.);
    H.acc[0] = std::tgamma(K::b_r + TF(1.)) * std::tgamma(TF(3.));
    H.acc[1] = TF(2.) * std::tgamma(K::b_r + TF(2.)) * std::tgamma(TF(2.));
    H.acc[2] = std::tgamma(K::b_r + TF(3.)) * std::tgamma(TF(1.));
    H.f1g2[0] = K::f_1r * std::tgamma(TF(2.));
    H.f1g2[1] = K::f_1s * std::tgamma(TF(2.));
    H.f1g2[2] = K::f_1g * std::tgamma(TF(2.));
    H.g_vent[0] = std::tgamma( TF(0.5) * (TF(5.) + K::d_r) );
    H.g_vent[1] = std::tgamma( TF(0.5) * (TF(5.) + K::d_s) );
    H.g_vent[2] = std::tgamma( TF(0.5) * (TF(5.) + K::d_g) );
    H.dt = TF(dt);
    const TF b_c[3] = {K::b_r, K::b_s, K::b_g}, d_c[3] = {K::d_r, K::d_s, K::d_g};
    for (int s=0; s<3; ++s)
        H.sed_g_bd1[s] = std::tgamma(b_c[s] + nsw6_runtime(d_c[s]) + TF(1.));
    return H;
}
// What depends on the level alone (:143-185, the ventilation roots of :382-430, the three latent factors of :596-647)
template<class TF> struct Nsw6Level { TF rho, p, exner, r0, fac[7], vent[3], lv, ls, lf; };
template<class TF> MHH_HD Nsw6Level<TF> nsw6_level(const Nsw6Tab<TF>& H, TF rho_kstart, TF rho, TF p, TF exner)
{
    typedef Nsw6C<TF> K; typedef MoistC<TF> M;
    Nsw6Level<TF> L;
    L.rho = rho; L.p = p; L.exner = exner;
    L.r0 = std::sqrt(rho_kstart/rho);
    for (int n=0; n<7; ++n) L.fac[n] = H.fac[n] * L.r0;
    L.vent[0] = std::sqrt(K::c_r * L.r0 / K::nu);
    L.vent[1] = std::sqrt(K::c_s * L.r0 / K::nu);
    L.vent[2] = std::sqrt(K::c_g * L.r0 / K::nu);
    L.lv = M::Lv / (M::cp * exner); L.ls = M::Ls / (M::cp * exner); L.lf = M::Lf / (M::cp * exner);
    return L;
}
// The powers of one species' slope parameter. NSW6_POW: std::pow wherever the reference has it, with its arguments. NSW6_SQRT: b = 3
// makes lambda a fourth root and every other exponent of the file a multiple of 1/8, so each is a product of integer powers of
// lambda, lambda^(1/2), lambda^(1/4) and lambda^(1/8). S: 0 rain, 1 snow, 2 graupel (d_s = 1/4, d_r = d_g = 1/2).
template<class TF> struct Nsw6Pow { TF l, l2, l3, p4, p5, p6, md, p3d, pv, p6d; };
template<int FORM, int S, class TF> MHH_HD Nsw6Pow<TF> nsw6_powers(TF x)
{
    typedef Nsw6C<TF> K;
    const TF b = (S == 0) ? K::b_r : (S == 1) ? K::b_s : K::b_g;
    const TF d = (S == 0) ? K::d_r : (S == 1) ? K::d_s : K::d_g;
    Nsw6Pow<TF> P;
    if (FORM == NSW6_POW)
    {
        P.l = std::pow(x, TF(1.) / (b + TF(1.)));
        P.l2 = P.l*P.l; P.l3 = P.l*P.l*P.l;
        P.p4 = std::pow(P.l, b + TF(1.)); P.p5 = std::pow(P.l, b + TF(2.)); P.p6 = std::pow(P.l, b + TF(3.));
        P.md = std::pow(P.l, -d);
        P.p3d = std::pow(P.l, TF(3.) + d);
        P.pv = std::pow(P.l, TF(0.5) * (TF(5.) + d));
        P.p6d = std::pow(P.l, TF(6.) + d);
    }
    else
    {
        P.l = std::sqrt(std::sqrt(x));
        const TF h = std::sqrt(P.l), q = std::sqrt(h);
        P.l2 = P.l*P.l; P.l3 = P.l2*P.l;
        P.p4 = P.l2*P.l2; P.p5 = P.p4*P.l; P.p6 = P.p4*P.l2;
        if (S == 1) { P.md = TF(1.)/q; P.p3d = P.l3*q; P.pv = P.l2*h*std::sqrt(q); P.p6d = P.p6*q; }
        else        { P.md = TF(1.)/h; P.p3d = P.l3*h; P.pv = P.l2*h*q;            P.p6d = P.p6*h; }
    }
    return P;
}
template<class TF> MHH_HD bool nsw6_idle(TF ql, TF qi, TF qr, TF qs, TF qg)
{
    typedef Nsw6C<TF> K;
    return !((ql > K::ql_min) || (qi > K::qi_min) || (qr > K::qr_min) || (qs > K::qs_min) || (qg > K::qg_min));      // :209
}
// The ventilation bracket of :381-384 and its siblings
template<class TF> MHH_HD TF nsw6_vent(TF f1g2, TF f_2, TF vent, TF g_vent, const Nsw6Pow<TF>& P)
{
    return f1g2 / P.l2 + f_2 * vent * g_vent / P.pv;
}
// conversion (:125-650) on one cell that is not idle: the five tendencies take the fifteen transfers in the reference's order.
template<class TF> struct Nsw6Tend { TF qrt, qst, qgt, qtt, thlt; };
template<int FORM, class TF> MHH_HD void nsw6_conversion(Nsw6Tend<TF>& t, const Nsw6Tab<TF>& H, const Nsw6Level<TF>& L, TF qr, TF qs, TF qg, TF qt,
                                                         TF thl, TF ql, TF qi)
{
    typedef Nsw6C<TF> K; typedef MoistC<TF> M;
    const TF rho = L.rho;
    const TF T = L.exner*thl + M::Lv/M::cp*ql + M::Ls/M::cp*qi;
    const TF qv = qt - ql - qi;
    const TF T_pos = TF(T >= M::T0);
    const TF T_neg = TF(1.) - T_pos;
    const bool has_vapor = (qv > K::qv_min), has_liq = (ql > K::ql_min), has_ice = (qi > K::qi_min);
    const bool has_rain = (qr > K::qr_min), has_snow = (qs > K::qs_min), has_graupel = (qg > K::qg_min);

    // Tomita Eq. 27
    const Nsw6Pow<TF> R = nsw6_powers<FORM, 0>(H.lam[0] / (rho * (qr + K::q_tiny)));
    const Nsw6Pow<TF> S = nsw6_powers<FORM, 1>(H.lam[1] / (rho * (qs + K::q_tiny)));
    const Nsw6Pow<TF> G = nsw6_powers<FORM, 2>(H.lam[2] / (rho * (qg + K::q_tiny)));
    // Eq. 28
    const TF V_Tr = !(has_rain)    ? TF(0.) : K::c_r * L.r0 * H.g_bd1[0] / H.g_b1 * R.md;
    const TF V_Ts = !(has_snow)    ? TF(0.) : K::c_s * L.r0 * H.g_bd1[1] / H.g_b1 * S.md;
    const TF V_Tg = !(has_graupel) ? TF(0.) : K::c_g * L.r0 * H.g_bd1[2] / H.g_b1 * G.md;

    // accretion, Eq. 29-38
    const TF P_iacr = !(has_rain && has_ice) ? TF(0.) : L.fac[0] / R.p6d * qi;
    const TF delta_1 = TF(qr >= TF(1.e-4));
    TF P_iacr_s = (TF(1.) - delta_1) * P_iacr;
    TF P_iacr_g = delta_1 * P_iacr;
    const TF P_raci = !(has_rain && has_ice) ? TF(0.) : L.fac[1] / R.p3d * qi;
    TF P_raci_s = (TF(1.) - delta_1) * P_raci;
    TF P_raci_g = delta_1 * P_raci;
    TF P_racw = !(has_liq && has_rain) ? TF(0.) : L.fac[2] / R.p3d * ql;
    TF P_sacw = !(has_liq && has_snow) ? TF(0.) : L.fac[3] / S.p3d * ql;
    const TF E_si = std::exp(K::gamma_sacr * (T - M::T0));                                                // Eq. 39
    TF P_saci = !(has_snow && has_ice)    ? TF(0.) : L.fac[4] * E_si / S.p3d * qi;
    TF P_gacw = !(has_graupel && has_liq) ? TF(0.) : L.fac[5] / G.p3d * ql;
    TF P_gaci = !(has_graupel && has_ice) ? TF(0.) : L.fac[6] / G.p3d * qi;

    // accretion of falling hydrometeors, Eq. 41-49
    const TF delta_2 = TF(1.) - TF( (qr >= TF(1.e-4)) || (qs >= TF(1.e-4)) );
    TF P_racs = !(has_rain && has_snow) ? TF(0.) :
        (TF(1.) - delta_2)
        * K::pi * K::a_s * tabs(V_Tr - V_Ts) * K::E_sr * K::N_0s * K::N_0r / (TF(4.)*rho)
        * (   H.acc[2] / ( S.p6 * R.l )
            + H.acc[1] / ( S.p5 * R.l2 )
            + H.acc[0] / ( S.p4 * R.l3 ) );
    const TF P_sacr = !(has_snow && has_rain) ? TF(0.) :
          K::pi * K::a_r * tabs(V_Ts - V_Tr) * K::E_sr * K::N_0r * K::N_0s / (TF(4.)*rho)
        * (   H.acc[0] / ( R.p4 * S.l3 )
            + H.acc[1] / ( R.p5 * S.l2 )
            + H.acc[2] / ( R.p6 * S.l ) );
    TF P_sacr_g = (TF(1.) - delta_2) * P_sacr;
    TF P_sacr_s = delta_2 * P_sacr;
    const TF E_gs = tmin( TF(1.), TF(std::exp(K::gamma_gacs * (T - M::T0))) );
    TF P_gacr = !(has_graupel && has_rain) ? TF(0.) :
          K::pi * K::a_r * tabs(V_Tg - V_Tr) * K::E_gr * K::N_0g * K::N_0r / (TF(4.)*rho)
        * (   H.acc[0] / ( R.p4 * G.l3 )
            + H.acc[1] / ( R.p5 * G.l2 )
            + H.acc[2] / ( R.p6 * G.l ) );
    TF P_gacs = !(has_graupel && has_snow) ? TF(0.) :
          K::pi * K::a_s * tabs(V_Tg - V_Ts) * E_gs * K::N_0g * K::N_0s / (TF(4.)*rho)
        * (   H.acc[0] / ( S.p4 * G.l3 )
            + H.acc[1] / ( S.p5 * G.l2 )
            + H.acc[2] / ( S.p6 * G.l ) );

    // autoconversion, Eq. 50-54. beta_2 is min(0, 0*exp(..)) as written; the second form spends no exp on it.
    constexpr TF q_icrt = TF(0.);
    constexpr TF q_scrt = TF(6.e-4);
    const TF beta_1 = tmin( K::beta_saut, TF(K::beta_saut*std::exp(K::gamma_saut * (T - M::T0))) );
    const TF beta_2 = (FORM == NSW6_POW) ? tmin( K::beta_gaut, TF(K::beta_gaut*std::exp(K::gamma_gaut * (T - M::T0))) ) : K::beta_gaut;
    TF P_raut = !(has_liq) ? TF(0.) :
        TF(16.7)/rho * sq(rho*ql) / (TF(5.) + H.nc_c / (H.D_d*rho*ql));
    TF P_saut = !(has_ice)  ? TF(0.) : tmax(beta_1*(qi - q_icrt), TF(0.));
    TF P_gaut = !(has_snow) ? TF(0.) : tmax(beta_2*(qs - q_scrt), TF(0.));

    // phase changes, Eq. 57-65; the exp of esat_ice once for G_i and S_i
    const TF es_liq = moist_esat_liq(T), es_ice = moist_esat_ice(T);
    const TF G_w = TF(1.) / (
        M::Lv / (K::K_a * T) * (M::Lv / (M::Rv * T) - TF(1.))
        + M::Rv*T / (K::K_d * es_liq) );
    const TF G_i = TF(1.) / (
        M::Ls / (K::K_a * T) * (M::Ls / (M::Rv * T) - TF(1.))
        + M::Rv*T / (K::K_d * es_ice) );
    const TF S_w = (qt - ql - qi) / (M::ep*es_liq/(L.p-(TF(1.)-M::ep)*es_liq));
    const TF S_i = (qt - ql - qi) / (M::ep*es_ice/(L.p-(TF(1.)-M::ep)*es_ice));
    const TF delta_3 = TF(S_i <= TF(1.));
    const TF vent_r = nsw6_vent(H.f1g2[0], K::f_2r, L.vent[0], H.g_vent[0], R);
    const TF vent_s = nsw6_vent(H.f1g2[1], K::f_2s, L.vent[1], H.g_vent[1], S);
    const TF vent_g = nsw6_vent(H.f1g2[2], K::f_2g, L.vent[2], H.g_vent[2], G);
    TF P_revp = !(has_rain) ? TF(0.) :
        - TF(2.)*K::pi * K::N_0r * (tmin(S_w, TF(1.)) - TF(1.)) * G_w / rho * vent_r;
    const TF P_sdep_ssub = TF(2.)*K::pi * K::N_0s * (S_i - TF(1.)) * G_i / rho * vent_s;
    const TF P_gdep_gsub = TF(2.)*K::pi * K::N_0g * (S_i - TF(1.)) * G_i / rho * vent_g;
    TF P_sdep = !(has_vapor)   ? TF(0.) : (TF(1.) - delta_3) * P_sdep_ssub;
    TF P_gdep = !(has_vapor)   ? TF(0.) : (TF(1.) - delta_3) * P_gdep_gsub;
    TF P_ssub = !(has_snow)    ? TF(0.) : - delta_3 * P_sdep_ssub;
    TF P_gsub = !(has_graupel) ? TF(0.) : - delta_3 * P_gdep_gsub;

    // freezing and melting, Eq. 67-70
    TF P_smlt = !(has_snow) ? TF(0.) :
        TF(2.)*K::pi * K::K_a * (T - M::T0) * K::N_0s / (rho*M::Lf) * vent_s
        + K::C_l * (T - M::T0) / M::Lf * (P_sacw + P_sacr);
    TF P_gmlt = !(has_graupel) ? TF(0.) :
        TF(2.)*K::pi * K::K_a * (T - M::T0) * K::N_0g / (rho*M::Lf) * vent_g
        + K::C_l * (T - M::T0) / M::Lf * (P_gacw + P_gacr);
    constexpr TF A_prime = TF(0.66);
    constexpr TF B_prime = TF(100.);
    TF P_gfrz = !(has_rain) ? TF(0.) :
        TF(20.) * K::pi_2 * B_prime * K::N_0r * K::rho_w / rho
        * (TF(std::exp(A_prime * (M::T0 - T))) - TF(1.)) / (R.l*R.l*R.l*R.l*R.l*R.l*R.l);

    // limit the production terms on the availability of their source (:444-486)
    const TF dt = H.dt;
    const TF dqv_dt_max = qv / dt, dqi_dt_max = qi / dt, dql_dt_max = ql / dt;
    const TF dqr_dt_max = qr / dt, dqs_dt_max = qs / dt, dqg_dt_max = qg / dt;
#define NSW6_LIMIT(tend, lim) tend = tmax(TF(0.), tmin(tend, lim))
    NSW6_LIMIT(P_iacr_s, dqr_dt_max); NSW6_LIMIT(P_iacr_g, dqr_dt_max); NSW6_LIMIT(P_raci_s, dqi_dt_max); NSW6_LIMIT(P_raci_g, dqi_dt_max);
    NSW6_LIMIT(P_racw, dql_dt_max);   NSW6_LIMIT(P_sacw, dql_dt_max);   NSW6_LIMIT(P_saci, dqi_dt_max);   NSW6_LIMIT(P_gacw, dql_dt_max);
    NSW6_LIMIT(P_gaci, dqi_dt_max);   NSW6_LIMIT(P_racs, dqs_dt_max);   NSW6_LIMIT(P_sacr_s, dqr_dt_max); NSW6_LIMIT(P_sacr_g, dqr_dt_max);
    NSW6_LIMIT(P_gacr, dqr_dt_max);   NSW6_LIMIT(P_gacs, dqs_dt_max);
    NSW6_LIMIT(P_raut, dql_dt_max);   NSW6_LIMIT(P_saut, dqi_dt_max);   NSW6_LIMIT(P_gaut, dqs_dt_max);
    NSW6_LIMIT(P_revp, dqr_dt_max);   NSW6_LIMIT(P_sdep, dqv_dt_max);   NSW6_LIMIT(P_ssub, dqs_dt_max);   NSW6_LIMIT(P_gdep, dqv_dt_max);
    NSW6_LIMIT(P_gsub, dqg_dt_max);   NSW6_LIMIT(P_smlt, dqs_dt_max);   NSW6_LIMIT(P_gmlt, dqg_dt_max);   NSW6_LIMIT(P_gfrz, dqr_dt_max);
#undef NSW6_LIMIT

    TF vapor_to_snow = P_sdep;
    TF vapor_to_graupel = P_gdep;
    TF cloud_to_rain = P_racw + P_sacw * T_pos + P_raut;
    TF cloud_to_graupel = P_gacw;
    TF cloud_to_snow = P_sacw * T_neg;
    TF rain_to_vapor = P_revp;
    TF rain_to_graupel = P_gacr + P_iacr_g + P_sacr_g * T_neg + P_gfrz * T_neg;
    TF rain_to_snow = P_sacr_s * T_neg + P_iacr_s;
    TF ice_to_snow = P_raci_s + P_saci + P_saut;
    TF ice_to_graupel = P_raci_g + P_gaci;
    TF snow_to_graupel = P_gacs + P_racs + P_gaut;
    TF snow_to_rain = P_smlt;
    TF snow_to_vapor = P_ssub;
    TF graupel_to_rain = P_gmlt * T_pos;
    TF graupel_to_vapor = P_gsub;

    const TF dqv_dt = - vapor_to_snow - vapor_to_graupel;
    const TF dql_dt = - cloud_to_rain - cloud_to_graupel - cloud_to_snow;
    const TF dqi_dt = - ice_to_snow - ice_to_graupel;
    const TF dqr_dt = + cloud_to_rain + snow_to_rain + graupel_to_rain - rain_to_vapor - rain_to_graupel - rain_to_snow;
    const TF dqs_dt = + cloud_to_snow + ice_to_snow + vapor_to_snow - snow_to_graupel - snow_to_vapor - snow_to_rain;
    const TF dqg_dt = + cloud_to_graupel + rain_to_graupel + ice_to_graupel + vapor_to_graupel + snow_to_graupel - graupel_to_rain - graupel_to_vapor;
#define NSW6_FACTOR(tend, lim) (((tend) < TF(0.)) ? tmin(-(lim)/(tend), TF(1.)) : TF(1.))
    const TF dqv_dt_fac = NSW6_FACTOR(dqv_dt, dqv_dt_max), dql_dt_fac = NSW6_FACTOR(dql_dt, dql_dt_max), dqi_dt_fac = NSW6_FACTOR(dqi_dt, dqi_dt_max);
    const TF dqr_dt_fac = NSW6_FACTOR(dqr_dt, dqr_dt_max), dqs_dt_fac = NSW6_FACTOR(dqs_dt, dqs_dt_max), dqg_dt_fac = NSW6_FACTOR(dqg_dt, dqg_dt_max);
#undef NSW6_FACTOR
    vapor_to_snow    *= dqv_dt_fac * dqs_dt_fac;
    vapor_to_graupel *= dqv_dt_fac * dqg_dt_fac;
    cloud_to_rain    *= dql_dt_fac * dqr_dt_fac;
    cloud_to_graupel *= dql_dt_fac * dqg_dt_fac;
    cloud_to_snow    *= dql_dt_fac * dqs_dt_fac;
    rain_to_vapor    *= dqr_dt_fac * dqv_dt_fac;
    rain_to_graupel  *= dqr_dt_fac * dqg_dt_fac;
    rain_to_snow     *= dqr_dt_fac * dqs_dt_fac;
    ice_to_snow      *= dqi_dt_fac * dqs_dt_fac;
    ice_to_graupel   *= dqi_dt_fac * dqg_dt_fac;
    snow_to_graupel  *= dqs_dt_fac * dqg_dt_fac;
    snow_to_vapor    *= dqs_dt_fac * dqv_dt_fac;
    snow_to_rain     *= dqs_dt_fac * dqr_dt_fac;
    graupel_to_rain  *= dqg_dt_fac * dqr_dt_fac;
    graupel_to_vapor *= dqg_dt_fac * dqv_dt_fac;

    // :593-647
    t.qtt -= cloud_to_rain;    t.qrt += cloud_to_rain;    t.thlt += L.lv * cloud_to_rain;
    t.qtt -= cloud_to_graupel; t.qgt += cloud_to_graupel; t.thlt += L.ls * cloud_to_graupel;
    t.qtt -= cloud_to_snow;    t.qst += cloud_to_snow;    t.thlt += L.ls * cloud_to_snow;
    t.qrt -= rain_to_vapor;    t.qtt += rain_to_vapor;    t.thlt -= L.lv * rain_to_vapor;
    t.qrt -= rain_to_graupel;  t.qgt += rain_to_graupel;  t.thlt += L.lf * rain_to_graupel;
    t.qrt -= rain_to_snow;     t.qst += rain_to_snow;     t.thlt += L.lf * rain_to_snow;
    t.qtt -= ice_to_snow;      t.qst += ice_to_snow;      t.thlt += L.ls * ice_to_snow;
    t.qtt -= ice_to_graupel;   t.qgt += ice_to_graupel;   t.thlt += L.ls * ice_to_graupel;
    t.qst -= snow_to_graupel;  t.qgt += snow_to_graupel;
    t.qst -= snow_to_vapor;    t.qtt += snow_to_vapor;    t.thlt -= L.ls * snow_to_vapor;
    t.qst -= snow_to_rain;     t.qrt += snow_to_rain;     t.thlt -= L.lf * snow_to_rain;
    t.qgt -= graupel_to_rain;  t.qrt += graupel_to_rain;  t.thlt -= L.lf * graupel_to_rain;
    t.qgt -= graupel_to_vapor; t.qtt += graupel_to_vapor; t.thlt -= L.ls * graupel_to_vapor;
}
// The terminal velocity of one level of sedimentation_ss08 / calc_cfl_ss08 (:704-735, :846-877): no q_tiny here, clamped to
// [0.1, 10] m/s, zero without the species. S as in nsw6_powers.
template<int FORM, int S, class TF> MHH_HD TF nsw6_w_sedi(const Nsw6Tab<TF>& H, TF qc, TF rho, TF r0)
{
    typedef Nsw6C<TF> K;
    const TF c_c = (S == 0) ? K::c_r : (S == 1) ? K::c_s : K::c_g;
    const TF d_c = (S == 0) ? K::d_r : (S == 1) ? K::d_s : K::d_g;
    const TF b_c = (S == 0) ? K::b_r : (S == 1) ? K::b_s : K::b_g;
    const TF qc_min = (S == 0) ? K::qr_min : (S == 1) ? K::qs_min : K::qg_min;
    if (!(qc > qc_min))
        return TF(0.);
    const TF x = H.lam[S] / (rho * qc);
    TF md;
    if (FORM == NSW6_POW)
    {
        const TF lambda_c = std::pow(x, TF(1.) / (b_c + TF(1.)));
        md = std::pow(lambda_c, -d_c);
    }
    else
    {
        const TF h = std::sqrt(std::sqrt(std::sqrt(x)));                      // lambda^(1/2)
        md = TF(1.) / ((S == 1) ? std::sqrt(h) : h);
    }
    const TF V_T = c_c * r0 * H.sed_g_bd1[S] / H.g_b1 * md;
    return tmax(K::V_Tmin, tmin(V_T, K::V_Tmax));
}

} // namespace mhh
