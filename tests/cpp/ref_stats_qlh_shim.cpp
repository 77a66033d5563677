// ref_stats_qlh_shim.cpp -- TEST infrastructure: the reference's own calc_liquid_water_h behind a C interface.
//
// The second translation unit of the statistics shim (tests/stats_ref.py compiles it together with ref_stats_shim.cpp, with the same
// flags, into a temporary directory; nothing compiled from it is kept). thermo_moist.cxx is included in place so that the kernel of
// its anonymous namespace is visible; it cannot share a translation unit with stats.cxx, because the reference's
// finite_difference.h is reached twice there without a guard that holds. What is written here is the call only, with the arguments
// Thermo_moist::get_thermo_field(fld, "ql_h", ...) (:1460-1465) passes: two 2-D slices of a tmp field for thlh and qth.
#include "thermo_moist.cxx"

#include <vector>
#include "ref_shim.h"

namespace
{
    template<typename TF>
    void qlh(const Dims& d, TF* out, const TF* thl, const TF* qt, const TF* prefh)
    {
        std::vector<TF> tmp((size_t)2*d.ijcells, TF(0));
        calc_liquid_water_h<TF>(out, const_cast<TF*>(thl), const_cast<TF*>(qt), const_cast<TF*>(prefh), &tmp[0], &tmp[d.ijcells],
                                d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
    }
}

REF_API void ref_stats_ql_h(int dtype, const Dims* d, void* out, const void* thl, const void* qt, const void* prefh)
{
    if (dtype == 0) qlh(*d, static_cast<double*>(out), static_cast<const double*>(thl), static_cast<const double*>(qt), static_cast<const double*>(prefh));
    else            qlh(*d, static_cast<float*>(out), static_cast<const float*>(thl), static_cast<const float*>(qt), static_cast<const float*>(prefh));
}
