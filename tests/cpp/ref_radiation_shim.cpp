// ref_radiation_shim.cpp -- TEST infrastructure: the reference's own Radiation_gcss kernels behind a C interface.
//
// Compiled by tests/radiation_ref.py into a temporary directory with the reference's src and include directories on the include
// path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections collected at link time, together with the
// reference's master.cxx and master_serial.cxx); nothing compiled from it is kept. The translation unit is included in place, so
// that the kernels of its anonymous namespace (calc_zenith, calc_gcss_rad_LW, calc_gcss_rad_SW, exec_gcss_rad) are visible here.
// What is written here is the calls only, with the arguments Radiation_gcss::exec (:353-379) and get_radiation_field (:392-436) pass.
#include "radiation_gcss.cxx"

#include <vector>
#include "ref_shim.h"

namespace
{
    template<typename TF>
    void rad_exec(const Dims& d, double xka, double fr0, double fr1, double div, double mu, TF* tt, const TF* ql, const TF* qt, TF* flx, TF* swn,
                  const TF* rhoref, const TF* z, const TF* dzhi)
    {
        std::vector<TF> lwp((size_t)d.ijcells * d.kcells, TF(0));
        exec_gcss_rad<TF>(tt, ql, qt, lwp.data(), flx, swn, rhoref, TF(mu), TF(0.035), TF(fr0), TF(fr1), TF(xka), TF(div), z, dzhi,
                          d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells, d.ijcells * d.kcells);
    }
    template<typename TF>
    void rad_lw(const Dims& d, double xka, double fr0, double fr1, double div, const TF* ql, const TF* qt, TF* flx, const TF* rhoref, const TF* z, const TF* dzi)
    {
        std::vector<TF> lwp((size_t)d.ijcells * d.kcells, TF(0));
        calc_gcss_rad_LW<TF>(ql, qt, lwp.data(), flx, rhoref, TF(fr0), TF(fr1), TF(xka), TF(div), z, dzi,
                             d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
    }
    template<typename TF>
    void rad_sw(const Dims& d, double mu, TF* swn, const TF* ql, const TF* qt, const TF* rhoref, const TF* z, const TF* dzi)
    {
        calc_gcss_rad_SW<TF>(swn, ql, qt, rhoref, z, dzi, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells,
                             d.ijcells * d.kcells, TF(mu));
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API double ref_rad_zenith(int dtype, double lat, double lon, double day_of_year)
{
    return dtype == 0 ? calc_zenith<double>(lat, lon, day_of_year) : (double)calc_zenith<float>((float)lat, (float)lon, day_of_year);
}
REF_API void ref_rad_exec(int dtype, const Dims* d, double xka, double fr0, double fr1, double div, double mu, void* tt, const void* ql, const void* qt,
                          void* flx, void* swn, const void* rhoref, const void* z, const void* dzhi)
{
    if (dtype == 0) rad_exec(*d, xka, fr0, fr1, div, mu, F64(tt), C64(ql), C64(qt), F64(flx), F64(swn), C64(rhoref), C64(z), C64(dzhi));
    else            rad_exec(*d, xka, fr0, fr1, div, mu, F32(tt), C32(ql), C32(qt), F32(flx), F32(swn), C32(rhoref), C32(z), C32(dzhi));
}
REF_API void ref_rad_lw(int dtype, const Dims* d, double xka, double fr0, double fr1, double div, const void* ql, const void* qt, void* flx,
                        const void* rhoref, const void* z, const void* dzi)
{
    if (dtype == 0) rad_lw(*d, xka, fr0, fr1, div, C64(ql), C64(qt), F64(flx), C64(rhoref), C64(z), C64(dzi));
    else            rad_lw(*d, xka, fr0, fr1, div, C32(ql), C32(qt), F32(flx), C32(rhoref), C32(z), C32(dzi));
}
REF_API void ref_rad_sw(int dtype, const Dims* d, double mu, void* swn, const void* ql, const void* qt, const void* rhoref, const void* z, const void* dzi)
{
    if (dtype == 0) rad_sw(*d, mu, F64(swn), C64(ql), C64(qt), C64(rhoref), C64(z), C64(dzi));
    else            rad_sw(*d, mu, F32(swn), C32(ql), C32(qt), C32(rhoref), C32(z), C32(dzi));
}
