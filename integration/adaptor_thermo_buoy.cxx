// integration/adaptor_thermo_buoy.cxx -- replaces the USECUDA half of the reference's Thermo_buoy (src/thermo_buoy.cu:322-479):
// exec and get_thermo_field_g ("N2", "b"). The parity target is the CPU path, src/thermo_buoy.cxx:347-415.
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "thermo_buoy.h"
#include "stats.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
// the device-to-device copy of get_thermo_field_g("b") is the HIP runtime's (the maintainer's build links it already)
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 3 = device to device

template<typename TF>
void Thermo_buoy<TF>::exec(const double, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    if (swbaroclinic) throw std::runtime_error("mhh: swbaroclinic is not supported by the library");
    const int order = (grid.get_spatial_order() == Grid_order::Fourth) ? 4 : 2;
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_fields f = mhh_make_fields(fields);
    // alpha == 0 and n2 == 0: the flat form (wt only); otherwise the slope / stratified form on ut, wt and bt, one launch. A caller
    // with a fused RHS pass may fold the flat form instead (mhh_diff_params::buoyancy_kind = 1) and skip this.
    mhh_check(mhh_thermo_buoy_tend(&g, order, &f, mhh_scalar_index(fields, "b"), bs.alpha, bs.n2, gd.utrans, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    stats.calc_tend(*fields.mt.at("w"), tend_name);
}

template<typename TF>
void Thermo_buoy<TF>::get_thermo_field_g(Field3d<TF>& fld, const std::string& name, const bool)
{
    auto& gd = grid.get_grid_data();
    if (name == "b")
    {
        if (hipMemcpy(fld.fld_g, fields.sp.at("b")->fld_g, gd.ncells*sizeof(TF), 3) != 0) throw std::runtime_error("hipMemcpy");
    }
    else if (name == "N2")
    {
        mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
        mhh_check(mhh_thermo_buoy_N2(&g, fld.fld_g, fields.sp.at("b")->fld_g, bs.n2, nullptr));
    }
    else
        throw std::runtime_error("Illegal thermo field");
}
#endif
