// ref_micro_shim.cpp -- TEST infrastructure: the reference's own Microphys_2mom_warm and Limiter kernels behind a C interface.
//
// Compiled by tests/micro_ref.py into a temporary directory with the reference's src and include directories on the include path
// (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections collected at link time, together with the
// reference's master.cxx and master_serial.cxx); nothing compiled from it is kept. The two translation units are included in place:
// mp3d:: and mp2d:: are named namespaces, the kernels of their anonymous namespaces (remove_negative_values, tendency_limiter) are
// visible to the including file. What is written here is the call sequence of Microphys_2mom_warm::exec (:639-752) with one process
// of a mask at a time, and ql as calc_condensate (src/thermo_moist.cxx:454) gives it with the Exner table for exner(p[k]).
#include "microphys_2mom_warm.cxx"
#include "limiter.cxx"

#include <vector>
#include "ref_shim.h"

namespace
{
    enum { AUTO = 1, ACCR = 2, EVAP = 4, SCBR = 8, SEDI = 16, CLIP = 32 };

    template<typename TF>
    void micro_exec(const Dims& d, int mask, double Nc0, double dt, TF* qr, TF* nr, const TF* thl, const TF* qt, TF* ql, TF* qrt, TF* nrt, TF* thlt,
                    TF* qtt, TF* rr_bot, const TF* rho, const TF* rhoh, const TF* p, const TF* exner, const TF* dz, const TF* dzi, TF* dr_out)
    {
        if (mask & CLIP)
        {
            remove_negative_values(qr, d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
            remove_negative_values(nr, d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        }
        for (int k=d.kstart; k<d.kend; k++)
            for (int j=d.jstart; j<d.jend; j++)
                for (int i=d.istart; i<d.iend; i++)
                {
                    const int ijk = i + j*d.icells + k*d.ijcells;
                    ql[ijk] = std::max(qt[ijk] - Thermo_moist_functions::sat_adjust(thl[ijk], qt[ijk], p[k], exner[k]).qs, TF(0.));
                }
        const int ikcells = d.icells * d.kcells;
        std::vector<TF> tmp(12 * (size_t)ikcells, TF(0));
        TF* s = tmp.data();
        TF *w_qr = s, *w_nr = s + ikcells, *c_qr = s + 2*ikcells, *c_nr = s + 3*ikcells, *slope_qr = s + 4*ikcells, *slope_nr = s + 5*ikcells;
        TF *flux_qr = s + 6*ikcells, *flux_nr = s + 7*ikcells, *rain_mass = s + 8*ikcells, *rain_diam = s + 9*ikcells;
        TF *lambda_r = s + 10*ikcells, *mu_r = s + 11*ikcells;

        if (mask & AUTO)
            mp3d::autoconversion(qrt, nrt, qtt, thlt, qr, ql, rho, exner, TF(Nc0), d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        if (mask & ACCR)
            mp3d::accretion(qrt, qtt, thlt, qr, ql, rho, exner, d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        for (int j=d.jstart; j<d.jend; ++j)
        {
            mp2d::prepare_microphysics_slice(rain_mass, rain_diam, mu_r, lambda_r, qr, nr, rho, d.istart, d.iend, d.kstart, d.kend, d.icells, d.ijcells, j);
            if (dr_out)
                for (int k=d.kstart; k<d.kend; k++)
                    for (int i=d.istart; i<d.iend; i++)
                        dr_out[i + j*d.icells + k*d.ijcells] = rain_diam[i + k*d.icells];
            if (mask & EVAP)
                mp2d::evaporation(qrt, nrt, qtt, thlt, qr, nr, ql, qt, thl, rho, exner, p, rain_mass, rain_diam,
                                  d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells, j);
            if (mask & SCBR)
                mp2d::selfcollection_breakup(nrt, qr, nr, rho, rain_mass, rain_diam, lambda_r,
                                             d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells, j);
            if (mask & SEDI)
                mp2d::sedimentation_ss08(qrt, nrt, rr_bot, w_qr, w_nr, c_qr, c_nr, slope_qr, slope_nr, flux_qr, flux_nr, mu_r, lambda_r, qr, nr,
                                         rho, rhoh, dzi, dz, dt, d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.kcells, d.ijcells, j);
        }
    }

    template<typename TF>
    double micro_cfl(const Dims& d, const TF* qr, const TF* nr, const TF* rho, const TF* dzi, double dt)
    {
        std::vector<TF> w((size_t)d.ijcells * d.kcells, TF(0));
        return mp3d::calc_max_sedimentation_cfl(w.data(), qr, nr, rho, dzi, dt, d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API void ref_micro_exec(int dtype, const Dims* d, int mask, double Nc0, double dt, void* qr, void* nr, const void* thl, const void* qt, void* ql,
                            void* qrt, void* nrt, void* thlt, void* qtt, void* rr_bot, const void* rho, const void* rhoh, const void* p,
                            const void* exner, const void* dz, const void* dzi, void* dr_out)
{
    if (dtype == 0) micro_exec(*d, mask, Nc0, dt, F64(qr), F64(nr), C64(thl), C64(qt), F64(ql), F64(qrt), F64(nrt), F64(thlt), F64(qtt), F64(rr_bot),
                               C64(rho), C64(rhoh), C64(p), C64(exner), C64(dz), C64(dzi), F64(dr_out));
    else            micro_exec(*d, mask, Nc0, dt, F32(qr), F32(nr), C32(thl), C32(qt), F32(ql), F32(qrt), F32(nrt), F32(thlt), F32(qtt), F32(rr_bot),
                               C32(rho), C32(rhoh), C32(p), C32(exner), C32(dz), C32(dzi), F32(dr_out));
}
REF_API double ref_micro_cfl(int dtype, const Dims* d, const void* qr, const void* nr, const void* rho, const void* dzi, double dt)
{
    return dtype == 0 ? micro_cfl(*d, C64(qr), C64(nr), C64(rho), C64(dzi), dt) : micro_cfl(*d, C32(qr), C32(nr), C32(rho), C32(dzi), dt);
}
REF_API void ref_limiter(int dtype, const Dims* d, void* at, const void* a, double dt)
{
    if (dtype == 0) tendency_limiter<double>(F64(at), C64(a), dt, d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
    else            tendency_limiter<float>(F32(at), C32(a), (float)dt, d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
}
