// integration/adaptor_boundary_surface.cxx -- replaces the USECUDA exec of the reference's Boundary_surface
// (src/boundary_surface.cu:360-527). The parity target is the CPU path, src/boundary_surface.cxx:830-983, with the lookup solver.
// prepare_device / forward_device / backward_device / clear_device stay the reference's: they allocate and copy obuk_g, ustar_g,
// z0m_g, z0h_g, dudz_mo_g, dvdz_mo_g, dbdz_mo_g, nobuk_g, zL_sl_g and f_sl_g, which is all the state this call needs (the table is
// the one init_solver made on the host). swconstantz0 = false and swcharnock are refused by the library: see INTEGRATION.md.
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "boundary.h"
#include "boundary_surface.h"
#include "thermo.h"
#include "constants.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
template<typename TF>
void Boundary_surface<TF>::exec(
        Thermo<TF>& thermo, Radiation<TF>& radiation,
        Microphys<TF>& microphys, Timeloop<TF>& timeloop)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_fields f = mhh_make_fields(fields);
    f.dudz = dudz_mo_g; f.dvdz = dvdz_mo_g; f.dbdz = dbdz_mo_g; f.z0m = z0m_g;

    mhh_surface_params p{};
    p.mbcbot = static_cast<int>(mbcbot);          // Boundary_type and MHH_BC_* share their values (include/boundary.h:51)
    p.swconstantz0 = sw_constant_z0; p.swcharnock = sw_charnock;
    const std::string sw = thermo.get_switch();
    if (sw == "dry" || sw == "buoy")
    {
        const std::string name = (sw == "dry") ? "th" : "b";
        p.thermo_kind = (sw == "dry") ? MHH_THERMO_DRY : MHH_THERMO_BUOY;
        p.thermo_index = mhh_scalar_index(fields, name);
        p.thermobc = static_cast<int>(thermobc);
        if (sw == "dry")
        {
            p.thref_kstart  = thermo.get_basestate_vector("th") [gd.kstart];
            p.threfh_kstart = thermo.get_basestate_vector("thh")[gd.kstart];
        }
        else
            p.bg_n2 = thermo.get_db_ref();            // Thermo_buoy::get_db_ref returns bs.n2 (include/thermo_buoy.h:66)
        p.grav = Constants::grav<TF>;
    }
    else if (sw != "0")
        throw std::runtime_error("mhh: the surface layer covers swthermo = 0, dry and buoy");
    p.zL = zL_sl_g; p.f = f_sl_g; p.z0m = z0m_g; p.z0h = z0h_g;
    p.ustar = ustar_g; p.obuk = obuk_g; p.nobuk = nobuk_g;
    p.ubot = fields.mp.at("u")->fld_bot_g; p.vbot = fields.mp.at("v")->fld_bot_g;
    p.ugradbot = fields.mp.at("u")->grad_bot_g; p.vgradbot = fields.mp.at("v")->grad_bot_g;
    int n = 0;
    for (auto& it : fields.sp)
    {
        p.sbot[n] = it.second->fld_bot_g; p.sgradbot[n] = it.second->grad_bot_g;
        p.sbcbot[n] = static_cast<int>(sbc.at(it.first).bcbot);
        ++n;
    }

    auto dutot = fields.get_tmp_g();
    const int rc = mhh_boundary_surface_exec(&g, &f, &p, dutot->fld_g, nullptr);
    const int rs = rc ? 0 : mhh_synchronize(nullptr);
    fields.release_tmp_g(dutot);          // before a refusal (swcharnock, swconstantz0 = false) throws
    mhh_check(rc); mhh_check(rs);
    (void)radiation; (void)microphys; (void)timeloop;
}
#endif
