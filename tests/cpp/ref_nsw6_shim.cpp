// ref_nsw6_shim.cpp -- TEST infrastructure: the reference's own Microphys_nsw6 kernels behind a C interface.
//
// Compiled by tests/nsw6_ref.py into a temporary directory with the reference's src and include directories on the include path
// (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections collected at link time, together with the
// reference's master.cxx and master_serial.cxx); nothing compiled from it is kept. The translation unit is included in place: the
// kernels and the constants of its anonymous namespaces (conversion, sedimentation_ss08, calc_cfl_ss08, a_r ... qg_min) are visible
// to the including file. What is written here is the argument lists of Microphys_nsw6::exec (:997-1061) and get_time_limit
// (:1128-1166) for one species at a time, and ql, qi as get_thermo_field("ql"), ("qi") give them (src/thermo_moist.cxx:247, :431)
// with the Exner table for exner(p[k]).
#include "microphys_nsw6.cxx"

#include <vector>
#include "ref_shim.h"

namespace
{
    template<typename TF>
    void nsw6_conversion(const Dims& d, double Nc0, double dt, TF* qrt, TF* qst, TF* qgt, TF* qtt, TF* thlt, const TF* qr, const TF* qs, const TF* qg,
                         const TF* qt, const TF* thl, const TF* ql, const TF* qi, const TF* rho, const TF* exner, const TF* p, const TF* dzi, const TF* dzhi)
    {
        conversion(qrt, qst, qgt, qtt, thlt, qr, qs, qg, qt, thl, ql, qi, rho, exner, p, dzi, dzhi, TF(Nc0), TF(dt),
                   d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
    }

    template<typename TF>
    void nsw6_sedimentation(const Dims& d, int species, double dt, TF* qct, TF* rc_bot, const TF* qc, const TF* rho, const TF* dzi, const TF* dz)
    {
        const size_t n = (size_t)d.ijcells * d.kcells;
        std::vector<TF> tmp(4*n, TF(0));
        TF* s = tmp.data();
        if (species == 0)
            sedimentation_ss08(qct, rc_bot, s, s+n, s+2*n, s+3*n, qc, rho, dzi, dz, dt, a_r<TF>, b_r<TF>, c_r<TF>, d_r<TF>, N_0r<TF>, qr_min<TF>,
                               d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        else if (species == 1)
            sedimentation_ss08(qct, rc_bot, s, s+n, s+2*n, s+3*n, qc, rho, dzi, dz, dt, a_s<TF>, b_s<TF>, c_s<TF>, d_s<TF>, N_0s<TF>, qs_min<TF>,
                               d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        else
            sedimentation_ss08(qct, rc_bot, s, s+n, s+2*n, s+3*n, qc, rho, dzi, dz, dt, a_g<TF>, b_g<TF>, c_g<TF>, d_g<TF>, N_0g<TF>, qg_min<TF>,
                               d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
    }

    template<typename TF>
    double nsw6_cfl(const Dims& d, int species, double dt, const TF* qc, const TF* rho, const TF* dzi, const TF* dz)
    {
        std::vector<TF> w((size_t)d.ijcells * d.kcells, TF(0));
        if (species == 0)
            return calc_cfl_ss08(w.data(), qc, rho, dzi, dz, dt, a_r<TF>, b_r<TF>, c_r<TF>, d_r<TF>, N_0r<TF>, qr_min<TF>,
                                 d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        if (species == 1)
            return calc_cfl_ss08(w.data(), qc, rho, dzi, dz, dt, a_s<TF>, b_s<TF>, c_s<TF>, d_s<TF>, N_0s<TF>, qs_min<TF>,
                                 d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
        return calc_cfl_ss08(w.data(), qc, rho, dzi, dz, dt, a_g<TF>, b_g<TF>, c_g<TF>, d_g<TF>, N_0g<TF>, qg_min<TF>,
                             d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells);
    }

    // returns the number of cells on which sat_adjust threw (their ql and qi stay as they were)
    template<typename TF>
    int nsw6_ql_qi(const Dims& d, const TF* thl, const TF* qt, const TF* p, const TF* exner, TF* ql, TF* qi, TF* T)
    {
        int threw = 0;
        for (int k=d.kstart; k<d.kend; k++)
            for (int j=d.jstart; j<d.jend; j++)
                for (int i=d.istart; i<d.iend; i++)
                {
                    const int ijk = i + j*d.icells + k*d.ijcells;
                    try
                    {
                        const auto ssa = Thermo_moist_functions::sat_adjust(thl[ijk], qt[ijk], p[k], exner[k]);
                        ql[ijk] = ssa.ql; qi[ijk] = ssa.qi; T[ijk] = ssa.t;
                    }
                    catch (...) { ++threw; }
                }
        return threw;
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API void ref_nsw6_conversion(int dtype, const Dims* d, double Nc0, double dt, void* qrt, void* qst, void* qgt, void* qtt, void* thlt, const void* qr,
                                 const void* qs, const void* qg, const void* qt, const void* thl, const void* ql, const void* qi, const void* rho,
                                 const void* exner, const void* p, const void* dzi, const void* dzhi)
{
    if (dtype == 0) nsw6_conversion(*d, Nc0, dt, F64(qrt), F64(qst), F64(qgt), F64(qtt), F64(thlt), C64(qr), C64(qs), C64(qg), C64(qt), C64(thl), C64(ql),
                                    C64(qi), C64(rho), C64(exner), C64(p), C64(dzi), C64(dzhi));
    else            nsw6_conversion(*d, Nc0, dt, F32(qrt), F32(qst), F32(qgt), F32(qtt), F32(thlt), C32(qr), C32(qs), C32(qg), C32(qt), C32(thl), C32(ql),
                                    C32(qi), C32(rho), C32(exner), C32(p), C32(dzi), C32(dzhi));
}
REF_API void ref_nsw6_sedimentation(int dtype, const Dims* d, int species, double dt, void* qct, void* rc_bot, const void* qc, const void* rho,
                                    const void* dzi, const void* dz)
{
    if (dtype == 0) nsw6_sedimentation(*d, species, dt, F64(qct), F64(rc_bot), C64(qc), C64(rho), C64(dzi), C64(dz));
    else            nsw6_sedimentation(*d, species, dt, F32(qct), F32(rc_bot), C32(qc), C32(rho), C32(dzi), C32(dz));
}
REF_API double ref_nsw6_cfl(int dtype, const Dims* d, int species, double dt, const void* qc, const void* rho, const void* dzi, const void* dz)
{
    return dtype == 0 ? nsw6_cfl(*d, species, dt, C64(qc), C64(rho), C64(dzi), C64(dz)) : nsw6_cfl(*d, species, dt, C32(qc), C32(rho), C32(dzi), C32(dz));
}
REF_API int ref_nsw6_ql_qi(int dtype, const Dims* d, const void* thl, const void* qt, const void* p, const void* exner, void* ql, void* qi, void* T)
{
    return dtype == 0 ? nsw6_ql_qi(*d, C64(thl), C64(qt), C64(p), C64(exner), F64(ql), F64(qi), F64(T))
                      : nsw6_ql_qi(*d, C32(thl), C32(qt), C32(p), C32(exner), F32(ql), F32(qi), F32(T));
}
