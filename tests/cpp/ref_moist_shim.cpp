// ref_moist_shim.cpp -- TEST infrastructure: the reference's own Thermo_moist_functions behind a C interface.
//
// Compiled by tests/moist_ref.py (tests/refshim.py holds the command) into a temporary directory with the reference's include
// directory on the include path; nothing compiled from it is kept. What comes from the reference at
// compile time: thermo_moist_functions.h (sat_adjust and every point function, exner, calc_base_state) with constants.h and
// fast_math.h. What is written here: the file-local loops of src/thermo_moist.cxx, which sit in an anonymous namespace and cannot
// be linked (calc_top_and_bot, calc_buoyancy_tend_2nd, calc_buoyancy, calc_liquid_water, calc_ice, calc_T, calc_N2), restated with
// the reference's expressions in its order, without their slice temporaries.
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#define restrict __restrict__
#include "thermo_moist_functions.h"
#include "ref_shim.h"

namespace tmf = Thermo_moist_functions;

namespace
{
    template<typename TF>
    int sat_cells(long long n, const TF* thl, const TF* qt, const TF* p, const TF* exn, TF* ql, TF* qi, TF* t, TF* qs, int* threw)
    {
        int nthrown = 0;
        for (long long c=0; c<n; ++c)
        {
            threw[c] = 0;
            try
            {
                const tmf::Struct_sat_adjust<TF> s = tmf::sat_adjust(thl[c], qt[c], p[c], exn[c]);
                ql[c] = s.ql; qi[c] = s.qi; t[c] = s.t; qs[c] = s.qs;
            }
            catch (const std::runtime_error&) { threw[c] = 1; ++nthrown; }
        }
        return nthrown;
    }

    template<typename TF>
    void top_and_bot(TF* thl0, TF* qt0, const TF* z, const TF* zh, const TF* dzhi, const int kstart, const int kend)
    {
        TF thl0s, qt0s, thl0t, qt0t;
        thl0s = thl0[kstart] - z[kstart]*(thl0[kstart+1]-thl0[kstart])*dzhi[kstart+1];
        qt0s  = qt0[kstart]  - z[kstart]*(qt0[kstart+1] -qt0[kstart] )*dzhi[kstart+1];
        thl0t = thl0[kend-1] + (zh[kend]-z[kend-1])*(thl0[kend-1]-thl0[kend-2])*dzhi[kend-1];
        qt0t  = qt0[kend-1]  + (zh[kend]-z[kend-1])*(qt0[kend-1]- qt0[kend-2] )*dzhi[kend-1];
        thl0[kstart-1]  = TF(2.)*thl0s - thl0[kstart];
        thl0[kend]      = TF(2.)*thl0t - thl0[kend-1];
        qt0[kstart-1]   = TF(2.)*qt0s  - qt0[kstart];
        qt0[kend]       = TF(2.)*qt0t  - qt0[kend-1];
    }

    // calc_buoyancy_tend_2nd; nsat counts the cells with ql + qi > 0
    template<typename TF>
    int tend_2nd(const Dims& d, TF* wt, const TF* thl, const TF* qt, const TF* ph, const TF* thvrefh)
    {
        int nsat = 0;
        const int jj = d.icells, kk = d.ijcells;
        for (int k=d.kstart+1; k<d.kend; k++)
        {
            const TF exnh = tmf::exner(ph[k]);
            for (int j=d.jstart; j<d.jend; j++)
                for (int i=d.istart; i<d.iend; i++)
                {
                    const int ijk = i + j*jj + k*kk;
                    const TF thlh = TF(0.5)*(thl[ijk-kk] + thl[ijk]);
                    const TF qth  = TF(0.5)*(qt[ijk-kk] + qt[ijk]);
                    const tmf::Struct_sat_adjust<TF> ssa = tmf::sat_adjust(thlh, qth, ph[k], exnh);
                    nsat += (ssa.ql + ssa.qi > TF(0.));
                    wt[ijk] += tmf::buoyancy(exnh, thlh, qth, ssa.ql, ssa.qi, thvrefh[k]);
                }
        }
        return nsat;
    }

    // calc_buoyancy, calc_liquid_water, calc_ice, calc_T
    template<typename TF>
    void fields(const Dims& d, const TF* thl, const TF* qt, const TF* p, const TF* exnref, const TF* thvref, TF* b, TF* ql, TF* qi, TF* T)
    {
        const int jj = d.icells, kk = d.ijcells;
        for (int k=0; k<d.kcells; k++)
        {
            const TF ex = tmf::exner(p[k]);
            const bool in = (k >= d.kstart && k < d.kend);
            for (int j=d.jstart; j<d.jend; j++)
                for (int i=d.istart; i<d.iend; i++)
                {
                    const int ijk = i + j*jj + k*kk;
                    TF l = 0., c = 0.;
                    if (in)
                    {
                        const tmf::Struct_sat_adjust<TF> ssa = tmf::sat_adjust(thl[ijk], qt[ijk], p[k], ex);
                        l = ssa.ql; c = ssa.qi;
                        ql[ijk] = ssa.ql;
                        qi[ijk] = ssa.qi;
                        T[ijk]  = tmf::sat_adjust(thl[ijk], qt[ijk], p[k], exnref[k]).t;
                    }
                    b[ijk] = tmf::buoyancy(ex, thl[ijk], qt[ijk], l, c, thvref[k]);
                }
        }
    }

    template<typename TF>
    void calc_N2(const Dims& d, TF* N2, const TF* thl, const TF* dzi, const TF* thvref)
    {
        using namespace Constants;
        const int jj = d.icells, kk = d.ijcells;
        for (int k=d.kstart; k<d.kend; ++k)
            for (int j=d.jstart; j<d.jend; ++j)
                for (int i=d.istart; i<d.iend; ++i)
                {
                    const int ijk = i + j*jj + k*kk;
                    N2[ijk] = grav<TF>/thvref[k]*TF(0.5)*(thl[ijk+kk] - thl[ijk-kk])*dzi[k];
                }
    }

    template<typename TF>
    void base_state(int kstart, int kend, int top_bot, TF* thl0, TF* qt0, double pbot, const TF* z, const TF* zh, const TF* dz, const TF* dzh, const TF* dzhi,
                    TF* pref, TF* prefh, TF* rho, TF* rhoh, TF* thv, TF* thvh, TF* ex, TF* exh)
    {
        if (top_bot) top_and_bot(thl0, qt0, z, zh, dzhi, kstart, kend);
        tmf::calc_base_state(pref, prefh, rho, rhoh, thv, thvh, ex, exh, thl0, qt0, TF(pbot), kstart, kend, z, dz, dzh);
    }
}

// Thermo_moist's hooks for the surface layer on n columns: calc_buoyancy_bot (src/thermo_moist.cxx:637-655), calc_buoyancy_fluxbot
// (:675-693) and get_db_ref (:1713-1717) with thvref = thvref[kstart], thvrefh = thvrefh[kstart]
template<typename TF>
void surf_hooks(int n, const TF* thl, const TF* qt, const TF* thlbot, const TF* qtbot, const TF* thlflux, const TF* qtflux,
                       TF thvref, TF thvrefh, TF* b, TF* bbot, TF* bfluxbot, TF* db_ref)
{
    for (int ij=0; ij<n; ++ij)
    {
        bbot[ij] = tmf::buoyancy_no_ql(thlbot[ij], qtbot[ij], thvrefh);
        b[ij]    = tmf::buoyancy_no_ql(thl[ij], qt[ij], thvref);
        bfluxbot[ij] = tmf::buoyancy_flux_no_ql(thl[ij], thlflux[ij], qt[ij], qtflux[ij], thvrefh);
    }
    *db_ref = Constants::grav<TF>/thvref*(thvref - thvrefh);
}
#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

#pragma GCC visibility push(default)      // the entry points: every function of this block
extern "C"
{
int ref_moist_sat_adjust(int dtype, long long n, const void* thl, const void* qt, const void* p, const void* exn,
                         void* ql, void* qi, void* t, void* qs, int* threw)
{
    return dtype == 0 ? sat_cells(n, C64(thl), C64(qt), C64(p), C64(exn), F64(ql), F64(qi), F64(t), F64(qs), threw)
                      : sat_cells(n, C32(thl), C32(qt), C32(p), C32(exn), F32(ql), F32(qi), F32(t), F32(qs), threw);
}
void ref_moist_exner(int dtype, int n, const void* p, void* out)
{
    for (int k=0; k<n; ++k)
        if (dtype == 0) F64(out)[k] = tmf::exner(C64(p)[k]);
        else            F32(out)[k] = tmf::exner(C32(p)[k]);
}
int ref_moist_tend(int dtype, const Dims* d, void* wt, const void* thl, const void* qt, const void* ph, const void* thvrefh)
{
    return dtype == 0 ? tend_2nd(*d, F64(wt), C64(thl), C64(qt), C64(ph), C64(thvrefh))
                      : tend_2nd(*d, F32(wt), C32(thl), C32(qt), C32(ph), C32(thvrefh));
}
void ref_moist_fields(int dtype, const Dims* d, const void* thl, const void* qt, const void* p, const void* exnref, const void* thvref,
                      void* b, void* ql, void* qi, void* T)
{
    if (dtype == 0) fields(*d, C64(thl), C64(qt), C64(p), C64(exnref), C64(thvref), F64(b), F64(ql), F64(qi), F64(T));
    else            fields(*d, C32(thl), C32(qt), C32(p), C32(exnref), C32(thvref), F32(b), F32(ql), F32(qi), F32(T));
}
void ref_moist_N2(int dtype, const Dims* d, void* N2, const void* thl, const void* dzi, const void* thvref)
{
    if (dtype == 0) calc_N2(*d, F64(N2), C64(thl), C64(dzi), C64(thvref));
    else            calc_N2(*d, F32(N2), C32(thl), C32(dzi), C32(thvref));
}
void ref_moist_surf_hooks(int dtype, int n, const void* thl, const void* qt, const void* thlbot, const void* qtbot, const void* thlflux,
                          const void* qtflux, double thvref, double thvrefh, void* b, void* bbot, void* bfluxbot, void* db_ref)
{
    if (dtype == 0) surf_hooks(n, C64(thl), C64(qt), C64(thlbot), C64(qtbot), C64(thlflux), C64(qtflux), thvref, thvrefh, F64(b), F64(bbot), F64(bfluxbot), F64(db_ref));
    else            surf_hooks(n, C32(thl), C32(qt), C32(thlbot), C32(qtbot), C32(thlflux), C32(qtflux), (float)thvref, (float)thvrefh, F32(b), F32(bbot), F32(bfluxbot), F32(db_ref));
}
void ref_moist_base_state(int dtype, int kstart, int kend, int top_bot, void* thl0, void* qt0, double pbot,
                          const void* z, const void* zh, const void* dz, const void* dzh, const void* dzhi,
                          void* pref, void* prefh, void* rho, void* rhoh, void* thv, void* thvh, void* ex, void* exh)
{
    if (dtype == 0) base_state(kstart, kend, top_bot, F64(thl0), F64(qt0), pbot, C64(z), C64(zh), C64(dz), C64(dzh), C64(dzhi),
                               F64(pref), F64(prefh), F64(rho), F64(rhoh), F64(thv), F64(thvh), F64(ex), F64(exh));
    else            base_state(kstart, kend, top_bot, F32(thl0), F32(qt0), pbot, C32(z), C32(zh), C32(dz), C32(dzh), C32(dzhi),
                               F32(pref), F32(prefh), F32(rho), F32(rhoh), F32(thv), F32(thvh), F32(ex), F32(exh));
}
}
#pragma GCC visibility pop
