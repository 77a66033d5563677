// ref_stats_flux_diff_2_shim.cpp -- TEST infrastructure: the reference's own calc_diff_flux of diff_2 behind a C interface.
// A translation unit of the statistics shim (tests/stats_ref.py compiles it with the others into a temporary directory; nothing
// compiled from it is kept); src/diff_2.cxx is included in place. The call is Diff_2::diff_flux's (:192-196).
#include "diff_2.cxx"
#include "ref_shim.h"
REF_API void ref_stats_flux_diff_2(int dtype, const Dims* d, void* out, const void* data, double visc, const void* dzhi)
{
    if (dtype == 0) calc_diff_flux(static_cast<double*>(out), static_cast<const double*>(data), visc, static_cast<const double*>(dzhi),
                                   d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
    else            calc_diff_flux(static_cast<float*>(out), static_cast<const float*>(data), float(visc), static_cast<const float*>(dzhi),
                                   d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
}
