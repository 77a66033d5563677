// integration/adaptor_force.cxx -- replaces the USECUDA half of the reference's Force (src/force.cu): exec. The parity target is
// the CPU path, src/force.cxx:46-311,581-729. prepare_device / clear_device / update_time_dependent stay the reference's (they
// fill ug_g, vg_g, wls_g, nudge_factor_g, lsprofs_g, nudgeprofs_g). scalednudgelist (rescale_nudgeprof, a host-side edit of a
// host profile that depends on thermo.get_bl_depth()) is refused: see INTEGRATION.md.
#include <cmath>
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "force.h"
#include "field3d_operators.h"
#include "stats.h"
#include "thermo.h"
#include "constants.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device, 2 = device to host

template<typename TF>
void Force<TF>::exec(double dt, Thermo<TF>& thermo, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    if (swnudge == Nudging_type::Enabled && !scalednudgelist.empty())
        throw std::runtime_error("mhh: scalednudgelist is not supported by the library (rescale the host profile and upload it instead)");
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_fields f = mhh_make_fields(fields);
    mhh_force_params p{};
    std::shared_ptr<Field3d<TF>> tmp;

    auto put = [&](const std::string& name, const void* prof, const void*& u, const void*& v, const void** s)
    {
        if (name == "u") u = prof;
        else if (name == "v") v = prof;
        else if (name == "w") throw std::runtime_error("mhh: large-scale and nudging profiles of w are not supported");
        else s[mhh_scalar_index(fields, name)] = prof;
    };

    if (swlspres == Large_scale_pressure_type::Fixed_flux)
    {
        // the two volume sums stay on the device between the reduction and the pass on one rank; with npy > 1 they pass through
        // master.sum, as the reference's do (src/field3d_operators.cxx:151)
        tmp = fields.get_tmp_g();
        const unsigned long long n = mhh_field_mean_scratch_elems(&g, 2);
        if ((n + 2)*sizeof(double) > (unsigned long long)gd.ncells*sizeof(TF)) throw std::runtime_error("mhh: tmp field too small for the reduction scratch");
        double* scratch = reinterpret_cast<double*>(tmp->fld_g);
        const void* uu[2] = {fields.mp.at("u")->fld_g, fields.mt.at("u")->fld_g};
        mhh_check(mhh_field_mean_sum(&g, uu, 2, scratch + n, scratch, nullptr));
        if (master.get_MPI_data().npy > 1)
        {
            double sums[2];
            mhh_check(mhh_synchronize(nullptr));
            if (hipMemcpy(sums, scratch + n, sizeof(sums), 2) != 0) throw std::runtime_error("hipMemcpy");
            master.sum(sums, 2);
            if (hipMemcpy(scratch + n, sums, sizeof(sums), 1) != 0) throw std::runtime_error("hipMemcpy");
        }
        p.swlspres = MHH_LSPRES_UFLUX; p.uflux = uflux; p.dt = dt; p.utrans = gd.utrans; p.uflux_sums = scratch + n;
    }
    else if (swlspres == Large_scale_pressure_type::Pressure_gradient)
    {
        p.swlspres = MHH_LSPRES_DPDX; p.dpdx = dpdx;
    }
    else if (swlspres == Large_scale_pressure_type::Geo_wind)
    {
        TF fc_loc = fc;
        if (fc_loc < 0)
            fc_loc = 2. * Constants::e_rot<TF> * std::sin(gd.lat * TF(M_PI) / 180.);
        p.swlspres = MHH_LSPRES_GEO; p.order = (grid.get_spatial_order() == Grid_order::Fourth) ? 4 : 2;
        p.fc = fc_loc; p.utrans = gd.utrans; p.vtrans = gd.vtrans; p.ug = ug_g; p.vg = vg_g;
    }

    if (swls == Large_scale_tendency_type::Enabled)
    {
        p.swls = 1;
        for (auto& it : lslist) put(it, lsprofs_g.at(it), p.ls_u, p.ls_v, p.ls_s);
    }
    if (swwls != Large_scale_subsidence_type::Disabled)
    {
        p.swwls = (swwls == Large_scale_subsidence_type::Mean_field) ? MHH_WLS_MEAN : MHH_WLS_LOCAL;
        p.swwls_mom = swwls_mom; p.wls = wls_g;
    }
    // the mean profiles of fields->exec() (src/model.cxx:351)
    p.mean_u = fields.mp.at("u")->fld_mean_g; p.mean_v = fields.mp.at("v")->fld_mean_g;
    {
        int n = 0;
        for (auto& it : fields.sp) p.mean_s[n++] = it.second->fld_mean_g;
    }
    if (swnudge == Nudging_type::Enabled)
    {
        p.swnudge = 1; p.nudge_factor = nudge_factor_g;
        for (auto& it : nudgelist) put(it, nudgeprofs_g.at(it), p.nudge_u, p.nudge_v, p.nudge_s);
    }
    (void)thermo;

    mhh_check(mhh_force_exec(&g, &f, &p, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    if (tmp) fields.release_tmp_g(tmp);

    if (swlspres == Large_scale_pressure_type::Fixed_flux || swlspres == Large_scale_pressure_type::Pressure_gradient)
        stats.calc_tend(*fields.mt.at("u"), tend_name_pres);
    else if (swlspres == Large_scale_pressure_type::Geo_wind)
    {
        stats.calc_tend(*fields.mt.at("u"), tend_name_cor);
        stats.calc_tend(*fields.mt.at("v"), tend_name_cor);
    }
    if (swls == Large_scale_tendency_type::Enabled)
        for (auto& it : lslist) stats.calc_tend(*fields.at.at(it), tend_name_ls);
    if (swwls != Large_scale_subsidence_type::Disabled)
    {
        if (swwls_mom)
        {
            stats.calc_tend(*fields.mt.at("u"), tend_name_subs);
            stats.calc_tend(*fields.mt.at("v"), tend_name_subs);
            if (swwls == Large_scale_subsidence_type::Local_field) stats.calc_tend(*fields.mt.at("w"), tend_name_subs);
        }
        for (auto& it : fields.st) stats.calc_tend(*it.second, tend_name_subs);
    }
    if (swnudge == Nudging_type::Enabled)
        for (auto& it : nudgelist) stats.calc_tend(*fields.at.at(it), tend_name_nudge);
}
#endif
