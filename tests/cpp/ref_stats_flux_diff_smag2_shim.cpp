// ref_stats_flux_diff_smag2_shim.cpp -- TEST infrastructure: the reference's own calc_diff_flux_c / _u / _v / _bc of diff_smag2 behind
// a C interface. A translation unit of the statistics shim (tests/stats_ref.py compiles it with the others into a temporary directory;
// nothing compiled from it is kept); src/diff_smag2.cxx is included in place. The calls are Diff_smag2::diff_flux's (:1217-1276) in
// both of its forms. kind: 0 scalar, 1 u, 2 v; di is gd.dxi for u and gd.dyi for v.
#include "diff_smag2.cxx"
#include "ref_shim.h"
namespace
{
    template<typename TF> void flux(const Dims& d, int kind, int sm, TF* out, const TF* data, const TF* w, const TF* evisc, const TF* bot, const TF* top,
                                    TF di, const TF* dzhi, TF tPr, TF visc)
    {
        if (sm)
        {
            calc_diff_flux_bc(out, bot, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.icells, d.ijcells);
            calc_diff_flux_bc(out, top, d.istart, d.iend, d.jstart, d.jend, d.kend, d.icells, d.ijcells);
            if (kind == 1)      calc_diff_flux_u<TF, Surface_model::Enabled>(out, data, w, evisc, di, dzhi, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
            else if (kind == 2) calc_diff_flux_v<TF, Surface_model::Enabled>(out, data, w, evisc, di, dzhi, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
            else                calc_diff_flux_c<TF, Surface_model::Enabled>(out, data, evisc, dzhi, tPr, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        }
        else
        {
            if (kind == 1)      calc_diff_flux_u<TF, Surface_model::Disabled>(out, data, w, evisc, di, dzhi, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
            else if (kind == 2) calc_diff_flux_v<TF, Surface_model::Disabled>(out, data, w, evisc, di, dzhi, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
            else                calc_diff_flux_c<TF, Surface_model::Disabled>(out, data, evisc, dzhi, tPr, visc, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        }
    }
}
#define P64(x) static_cast<const double*>(x)
#define P32(x) static_cast<const float*>(x)
REF_API void ref_stats_flux_diff_smag2(int dtype, const Dims* d, int kind, int sm, void* out, const void* data, const void* w, const void* evisc, const void* bot,
                               const void* top, double di, const void* dzhi, double tPr, double visc)
{
    if (dtype == 0) flux(*d, kind, sm, static_cast<double*>(out), P64(data), P64(w), P64(evisc), P64(bot), P64(top), di, P64(dzhi), tPr, visc);
    else            flux(*d, kind, sm, static_cast<float*>(out), P32(data), P32(w), P32(evisc), P32(bot), P32(top), float(di), P32(dzhi), float(tPr), float(visc));
}
