// integration/adaptor_radiation_gcss.cxx -- replaces the USECUDA half of the reference's Radiation_gcss (src/radiation_gcss.cu: exec,
// exec_column, get_radiation_field_g). The parity target is the CPU path, src/radiation_gcss.cxx:253-309, :353-379 and :392-436; the
// CUDA file differs from it in physics (no max(0, .), dz for z[k]-z[k-1], lwp subtracted on the way up, the flux difference shifted
// by a level). ql comes from the thermodynamics into a tmp field, as the reference's exec takes it; two more tmp fields are the
// library's scratch (the reference's CPU path holds four).
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "thermo.h"
#include "stats.h"
#include "column.h"
#include "timeloop.h"
#include "radiation.h"
#include "radiation_gcss.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
namespace
{
    // calc_zenith (:39-76) for gd.lat, gd.lon and Timeloop::calc_day_of_year(), with the host's C library in TF
    template<typename TF, class GD, class TL>
    double mhh_zenith(const GD& gd, TL& timeloop)
    {
        double mu = 0;
        mhh_check(mhh_radiation_gcss_zenith_host(mhh_dtype<TF>(), gd.lat, gd.lon, timeloop.calc_day_of_year(), &mu));
        return mu;
    }
}

template<typename TF>
void Radiation_gcss<TF>::exec(Thermo<TF>& thermo, double time, Timeloop<TF>& timeloop, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto ql = fields.get_tmp_g();
    std::shared_ptr<Field3d<TF>> tmp[2] = {fields.get_tmp_g(), fields.get_tmp_g()};
    thermo.get_thermo_field_g(*ql, "ql", false);
    mhh_radiation_gcss_params p{};
    p.xka = xka; p.fr0 = fr0; p.fr1 = fr1; p.div = div; p.mu = mhh_zenith<TF>(gd, timeloop); p.parts = MHH_RAD_LW | MHH_RAD_SW;
    void* const scratch[2] = {tmp[0]->fld_g, tmp[1]->fld_g};
    mhh_check(mhh_radiation_gcss_exec(&g, &p, fields.st.at("thl")->fld_g, ql->fld_g, nullptr, fields.sp.at("qt")->fld_g, fields.rhoref_g,
                                      nullptr, nullptr, nullptr, nullptr, scratch, nullptr, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    fields.release_tmp_g(ql);
    for (auto& t : tmp)
        fields.release_tmp_g(t);
    stats.calc_tend(*fields.st.at("thl"), tend_name);
}

template<typename TF>
void Radiation_gcss<TF>::exec_column(Column<TF>& column, Thermo<TF>& thermo, Timeloop<TF>& timeloop)
{
    const TF no_offset = 0.;
    auto flx = fields.get_tmp_g();
    get_radiation_field_g(*flx, "lflx", thermo, timeloop);
    column.calc_column("lflx", flx->fld_g, no_offset);
    get_radiation_field_g(*flx, "sflx", thermo, timeloop);
    column.calc_column("sflx", flx->fld_g, no_offset);
    fields.release_tmp_g(flx);
}

template<typename TF>
void Radiation_gcss<TF>::get_radiation_field_g(Field3d<TF>& fld, std::string name, Thermo<TF>& thermo, Timeloop<TF>& timeloop)
{
    if (name != "lflx" && name != "sflx")
        throw std::runtime_error("get_radiation_field_g: \"" + name + "\" is not a field of radiation_gcss (lflx | sflx)");
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto ql = fields.get_tmp_g();
    std::shared_ptr<Field3d<TF>> tmp[2] = {fields.get_tmp_g(), fields.get_tmp_g()};
    thermo.get_thermo_field_g(*ql, "ql", false);
    mhh_radiation_gcss_params p{};
    p.xka = xka; p.fr0 = fr0; p.fr1 = fr1; p.div = div; p.mu = mhh_zenith<TF>(gd, timeloop); p.parts = MHH_RAD_LW | MHH_RAD_SW;
    // (mu_min = 0.035 is the library's too: at night sflx is the zero fill)
    if (!(mu_min == TF(0.035))) throw std::runtime_error("radiation_gcss: mu_min");
    void* const scratch[2] = {tmp[0]->fld_g, tmp[1]->fld_g};
    mhh_check(mhh_radiation_gcss_exec(&g, &p, nullptr, ql->fld_g, nullptr, fields.ap.at("qt")->fld_g, fields.rhoref_g, nullptr, nullptr,
                                      name == "lflx" ? fld.fld_g : nullptr, name == "sflx" ? fld.fld_g : nullptr, scratch, nullptr, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    fields.release_tmp_g(ql);
    for (auto& t : tmp)
        fields.release_tmp_g(t);
}
#endif
