// ref_cross_shim.cpp -- TEST infrastructure: the reference's own Cross kernels behind a C interface.
//
// Compiled by tests/cross_ref.py into a temporary directory with the reference's src and include directories and
// tests/stubs_syntax_only on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections
// collected at link time); nothing compiled from it is kept. The translation unit is included in place, so that the four kernels of
// its anonymous namespace (calc_lngrad_4th, calc_lngrad_2nd, calc_cross_path, calc_cross_height_threshold) are visible here. What
// is written here is the calls only, with the arguments Cross::cross_lngrad (:653-703), cross_path (:705-725) and
// cross_height_threshold (:738-760) pass. Cross::create is a member behind Master and Grid: tests/test_cross_indices.py restates it.
#include "cross.cxx"
#include "ref_shim.h"

namespace
{
    template<typename TF>
    void lngrad(const Dims& d, int order, const TF* a, TF* out, double dxi, double dyi, const TF* dzi)
    {
        if (order == 2)
            calc_lngrad_2nd<TF>(a, out, TF(dxi), TF(dyi), dzi, d.icells, d.ijcells, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend);
        else
            calc_lngrad_4th<TF>(a, out, TF(dxi), TF(dyi), dzi, d.icells, d.ijcells, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend);
    }

    // tmp is a whole field; the path sits on level kstart (cross_path hands &tmp[kstart*ijcells] to cross_plane)
    template<typename TF>
    void path(const Dims& d, const TF* data, TF* tmp, const TF* rhoref, const TF* dz)
    {
        calc_cross_path<TF>(data, tmp, rhoref, dz, d.icells, d.ijcells, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend);
    }

    template<typename TF>
    void height(const Dims& d, const TF* data, TF* height, const TF* z, double threshold, int upward)
    {
        TF fillvalue = -1e-9;      // :748
        calc_cross_height_threshold<TF>(data, height, z, TF(threshold), upward != 0, fillvalue,
                d.icells, d.ijcells, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend);
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API void ref_cross_lngrad(int dtype, const Dims* d, int order, const void* a, void* out, double dxi, double dyi, const void* dzi)
{
    if (dtype == 0) lngrad(*d, order, C64(a), F64(out), dxi, dyi, C64(dzi));
    else            lngrad(*d, order, C32(a), F32(out), dxi, dyi, C32(dzi));
}
REF_API void ref_cross_path(int dtype, const Dims* d, const void* data, void* tmp, const void* rhoref, const void* dz)
{
    if (dtype == 0) path(*d, C64(data), F64(tmp), C64(rhoref), C64(dz));
    else            path(*d, C32(data), F32(tmp), C32(rhoref), C32(dz));
}
REF_API void ref_cross_height(int dtype, const Dims* d, const void* data, void* out, const void* z, double threshold, int upward)
{
    if (dtype == 0) height(*d, C64(data), F64(out), C64(z), threshold, upward);
    else            height(*d, C32(data), F32(out), C32(z), threshold, upward);
}
