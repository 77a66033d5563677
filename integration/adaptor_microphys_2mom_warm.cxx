// integration/adaptor_microphys_2mom_warm.cxx -- replaces the USECUDA half of the reference's Microphys_2mom_warm
// (src/microphys_2mom_warm.cu: exec, get_time_limit, get_surface_rain_rate_g, prepare_device, clear_device, backward_device). The parity
// target is the CPU path, src/microphys_2mom_warm.cxx:639-752 and :965-982. ql is evaluated per cell from thl and qt (no 3-D tmp field
// through get_thermo_field_g), sedimentation's CFL numbers and slopes take four tmp fields where the reference takes six at a time.
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
#include "microphys.h"
#include "microphys_2mom_warm.h"
#include "mhh_adaptor.h"

// entry points the maintainer's build already links; declared here so that this file needs no HIP header
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);
extern "C" int hipMemset(void* dst, int value, size_t size);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 2 = device to host, 3 = device to device

#ifdef USECUDA
using namespace Micro_2mom_warm_constants;

template<typename TF>
void Microphys_2mom_warm<TF>::exec(Thermo<TF>& thermo, const double dt, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_micro_params p{};
    p.Nc0 = Nc0<TF>; p.dt = dt; p.processes = MHH_MICRO_ALL;
    std::shared_ptr<Field3d<TF>> tmp[4] = {fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g()};
    void* const scratch[4] = {tmp[0]->fld_g, tmp[1]->fld_g, tmp[2]->fld_g, tmp[3]->fld_g};
    // the Exner table of the thermodynamics for exner(p[k]); the counter of non-converged cells is the caller's to add
    mhh_check(mhh_micro_2mom_warm_exec(&g, &p, fields.sp.at("qr")->fld_g, fields.sp.at("nr")->fld_g, fields.sp.at("thl")->fld_g, fields.sp.at("qt")->fld_g,
                                       fields.st.at("qr")->fld_g, fields.st.at("nr")->fld_g, fields.st.at("thl")->fld_g, fields.st.at("qt")->fld_g, rr_bot_g,
                                       fields.rhoref_g, thermo.get_basestate_fld_g("pref"), thermo.get_basestate_fld_g("exner"), scratch, nullptr, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    for (auto& t : tmp)
        fields.release_tmp_g(t);
    stats.calc_tend(*fields.st.at("thl"), tend_name);
    stats.calc_tend(*fields.st.at("qt"),  tend_name);
    stats.calc_tend(*fields.st.at("qr"),  tend_name);
    stats.calc_tend(*fields.st.at("nr"),  tend_name);
}

template<typename TF>
unsigned long Microphys_2mom_warm<TF>::get_time_limit(unsigned long idt, const double dt)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto work = fields.get_tmp_g();
    double out = 0;
    mhh_check(mhh_micro_2mom_warm_cfl(&g, fields.sp.at("qr")->fld_g, fields.sp.at("nr")->fld_g, fields.rhoref_g, dt, work->fld_g, &out, nullptr));
    fields.release_tmp_g(work);
    TF cfl = TF(out);
    master.max(&cfl, 1);
    return idt * cflmax / cfl;
}

template<typename TF>
void Microphys_2mom_warm<TF>::get_surface_rain_rate_g(TF* rr_out)
{
    auto& gd = grid.get_grid_data();
    if (hipMemcpy(rr_out, rr_bot_g, gd.ijcells*sizeof(TF), 3) != 0) throw std::runtime_error("hipMemcpy");
}

template<typename TF>
void Microphys_2mom_warm<TF>::prepare_device()
{
    auto& gd = grid.get_grid_data();
    if (hipMalloc(reinterpret_cast<void**>(&rr_bot_g), gd.ijcells*sizeof(TF)) != 0) throw std::runtime_error("hipMalloc");
    if (hipMemset(rr_bot_g, 0, gd.ijcells*sizeof(TF)) != 0) throw std::runtime_error("hipMemset");
}

template<typename TF>
void Microphys_2mom_warm<TF>::backward_device()
{
    auto& gd = grid.get_grid_data();
    if (hipMemcpy(rr_bot.data(), rr_bot_g, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
}

template<typename TF>
void Microphys_2mom_warm<TF>::clear_device()
{
    if (hipFree(rr_bot_g) != 0) throw std::runtime_error("hipFree");
}
#endif
