// integration/adaptor_thermo_moist.cxx -- replaces the USECUDA half of the reference's Thermo_moist::exec and get_thermo_field_g
// (src/thermo_moist.cu:786-960). The parity target is the CPU path, src/thermo_moist.cxx:1273-1303 and :1418-1500. The base state is
// recomputed on the device from fld_mean_g of thl and qt: no copy of the means to the host and of eight profiles back
// (src/thermo_moist.cu:806-844), nothing between the two calls of exec leaves the stream.
#include <memory>
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "field3d_operators.h"
#include "field3d_io.h"
#include "thermo_moist.h"
#include "stats.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
template<typename TF>
void Thermo_moist<TF>::exec(const double, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    if (grid.get_spatial_order() == Grid_order::Fourth)
        throw std::runtime_error("mhh: Thermo_moist is second order only (the reference's calc_buoyancy_tend_4th is never called)");
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    TF* thl = fields.sp.at("thl")->fld_g; TF* qt = fields.sp.at("qt")->fld_g;
    // the counter of cells on which the CPU path would throw is the caller's to add (a device int); without one nothing is counted
    if (bs.swupdatebasestate)
        mhh_check(mhh_thermo_moist_base_state(&g, fields.sp.at("thl")->fld_mean_g, fields.sp.at("qt")->fld_mean_g, bs.pbot,
                                              bs.pref_g, bs.prefh_g, bs.rhoref_g, bs.rhorefh_g, bs.thvref_g, bs.thvrefh_g, bs.exnref_g, bs.exnrefh_g,
                                              nullptr, nullptr));
    mhh_check(mhh_thermo_moist_buoyancy_tend(&g, fields.mt.at("w")->fld_g, thl, qt, bs.prefh_g, bs.exnrefh_g, bs.thvrefh_g, nullptr, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    stats.calc_tend(*fields.mt.at("w"), tend_name);
}

template<typename TF>
void Thermo_moist<TF>::get_thermo_field_g(Field3d<TF>& fld, const std::string& name, const bool)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    TF* thl = fields.sp.at("thl")->fld_g; TF* qt = fields.sp.at("qt")->fld_g;
    if (name != "b" && name != "ql" && name != "qi" && name != "T" && name != "N2")
        throw std::runtime_error("mhh: get_thermo_field_g \"" + name + "\" is not built (b | ql | qi | T | N2)");
    // the pressure and Exner profiles from the current means (src/thermo_moist.cxx:1425-1432); thvref stays
    if (bs.swupdatebasestate)
        mhh_check(mhh_thermo_moist_base_state(&g, fields.sp.at("thl")->fld_mean_g, fields.sp.at("qt")->fld_mean_g, bs.pbot,
                                              bs.pref_g, bs.prefh_g, nullptr, nullptr, nullptr, nullptr, bs.exnref_g, bs.exnrefh_g, nullptr, nullptr));
    if (name == "N2")
        mhh_check(mhh_calc_N2(&g, fld.fld_g, thl, bs.thvref_g, 9.81, nullptr));
    else
        mhh_check(mhh_thermo_moist_fields(&g, thl, qt, bs.pref_g, bs.exnref_g, bs.thvref_g, name == "b" ? fld.fld_g : nullptr,
                                          name == "ql" ? fld.fld_g : nullptr, name == "qi" ? fld.fld_g : nullptr, name == "T" ? fld.fld_g : nullptr,
                                          nullptr, nullptr));
}
#endif
