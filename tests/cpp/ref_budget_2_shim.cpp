// ref_budget_2_shim.cpp -- TEST infrastructure: the reference's own Budget_2 kernels behind a C interface.
//
// Compiled by tests/budget_ref.py into a temporary directory with the command tests/stats_ref.py uses for its shims (the
// reference's src and include directories and tests/stubs_syntax_only on the include path, g++ -std=c++17 -O2 -ffp-contract=off
// -DRESTRICTKEYWORD=__restrict__, sections collected at link time); nothing compiled from it is kept. The translation unit is
// included in place, so that the calc_* functions of its anonymous namespace are visible here. What is written here is the calls
// only, with the arguments Budget_2<TF>::exec_stats (:1414-1818) passes. Grid::interpolate_2nd (wx, wy) is a member of Grid<TF> and
// cannot be reached without an object: tests/budget_ref.py restates that one expression in NumPy float64.
#include "budget_2.cxx"
#include "ref_shim.h"

namespace
{
    // out: the term fields of the group, in the library's order (the LES diffusion group: two more, the helper fields wz and evisch);
    // in: u, v, w, p, evisc, b, ufluxbot, vfluxbot, wx, wy;
    // prof: umodel, vmodel, wmodel, bmean, pmean, dzi, dzhi; par: utrans, vtrans, fc, dxi, dyi
    template<typename TF>
    void group(const Dims& d, int grp, void* const* out, const void* const* in, const void* const* prof, const double* par)
    {
        auto O = [&](int n) { return static_cast<TF*>(out[n]); };
        auto I = [&](int n) { return static_cast<const TF*>(in[n]); };
        auto P = [&](int n) { return static_cast<const TF*>(prof[n]); };
        const TF *u = I(0), *v = I(1), *w = I(2), *p = I(3), *b = I(5), *wx = I(8), *wy = I(9);
        const TF *um = P(0), *vm = P(1), *wm = P(2), *bmean = P(3), *pmean = P(4), *dzi = P(5), *dzhi = P(6);
        const TF utrans = par[0], vtrans = par[1], fc = par[2], dxi = par[3], dyi = par[4];
        switch (grp)
        {
            case 0: calc_kinetic_energy(O(0), O(1), u, v, w, um, vm, wm, utrans, vtrans,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 1: calc_shear_terms(O(0), O(1), O(2), O(3), O(4), u, v, w, um, vm, wm, wx, wy, dzi, dzhi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 2: calc_turb_terms(O(0), O(1), O(2), O(3), O(4), O(5), u, v, w, um, vm, wm, wx, wy, dzi, dzhi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 3: calc_coriolis_terms(O(0), O(1), O(2), O(3), u, v, w, um, vm, wm, fc,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 4: calc_pressure_transport_terms(O(0), O(1), O(2), O(3), u, v, w, p, um, vm, wm, dzi, dzhi, dxi, dyi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 5: calc_pressure_redistribution_terms(O(0), O(1), O(2), O(3), O(4), u, v, w, p, um, vm, wm, dzi, dzhi, dxi, dyi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 6: calc_diffusion_terms_les(O(0), O(1), O(2), O(3), O(4), O(5), O(6), O(7), u, v, w, I(6), I(7), I(4), um, vm, wm, dzi, dzhi, dxi, dyi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells/d.icells, d.ijcells); break;
            case 7: calc_buoyancy_terms(O(0), O(1), O(2), O(3), u, v, w, b, um, vm, wm, bmean,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 8: calc_buoyancy_terms_scalar(O(0), b, b, bmean, bmean,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 9: calc_advection_terms_scalar(O(0), O(1), O(2), O(3), w, b, bmean, dzi, dzhi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            case 10: calc_pressure_terms_scalar(O(0), O(1), b, p, bmean, pmean, dzi, dzhi,
                            d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells); break;
            default: break;
        }
    }
}

REF_API void ref_budget_2_group(int dtype, const Dims* d, int grp, void* const* out, const void* const* in, const void* const* prof, const double* par)
{
    if (dtype == 0) group<double>(*d, grp, out, in, prof, par);
    else            group<float>(*d, grp, out, in, prof, par);
}
