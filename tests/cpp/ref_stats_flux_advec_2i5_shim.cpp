// ref_stats_flux_advec_2i5_shim.cpp -- TEST infrastructure: the reference's own advec_flux_u / _v / _s of advec_2i5 and advec_flux_s_lim behind a C interface.
// A translation unit of the statistics shim (tests/stats_ref.py compiles it with the others into a temporary directory; nothing
// compiled from it is kept); src/advec_2i5.cxx is included in place so that the kernels of its anonymous namespace are visible. What is
// written here is the call only, with the arguments Advec_2i5::get_advec_flux passes. kind: 0 scalar, 1 u, 2 v, 3 a scalar of fluxlimit_list.
#include "advec_2i5.cxx"
#include "ref_shim.h"
namespace
{
    template<typename TF> void flux(const Dims& d, int kind, TF* st, const TF* s, const TF* w)
    {
        if (kind == 1)      advec_flux_u(st, s, w, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        else if (kind == 2) advec_flux_v(st, s, w, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        else if (kind == 3) advec_flux_s_lim(st, s, w, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        else                advec_flux_s(st, s, w, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
    }
}
REF_API void ref_stats_flux_advec_2i5(int dtype, const Dims* d, int kind, void* st, const void* s, const void* w)
{
    if (dtype == 0) flux(*d, kind, static_cast<double*>(st), static_cast<const double*>(s), static_cast<const double*>(w));
    else            flux(*d, kind, static_cast<float*>(st), static_cast<const float*>(s), static_cast<const float*>(w));
}
