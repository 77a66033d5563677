// integration/adaptor_microphys_nsw6.cxx -- replaces the USECUDA half of the reference's Microphys_nsw6 (src/microphys_nsw6.cu: exec,
// get_time_limit, get_surface_rain_rate_g, prepare_device, clear_device, backward_device). The parity target is the CPU path,
// src/microphys_nsw6.cxx:983-1073 and :1119-1177. ql and qi are evaluated per cell from thl and qt inside the conversion kernel (no
// 3-D tmp fields through get_thermo_field_g); sedimentation's CFL numbers and slopes take six tmp fields, two per species, where the
// reference takes four for one species at a time.
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
#include "microphys_nsw6.h"
#include "mhh_adaptor.h"

// entry points the maintainer's build already links; declared here so that this file needs no HIP header
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);
extern "C" int hipMemset(void* dst, int value, size_t size);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 2 = device to host, 3 = device to device

#ifdef USECUDA
template<typename TF>
void Microphys_nsw6<TF>::exec(Thermo<TF>& thermo, const double dt, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_micro_params p{};
    p.Nc0 = this->Nc0; p.dt = dt; p.processes = MHH_NSW6_ALL;
    std::shared_ptr<Field3d<TF>> tmp[6] = {fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g(), fields.get_tmp_g()};
    void* const scratch[6] = {tmp[0]->fld_g, tmp[1]->fld_g, tmp[2]->fld_g, tmp[3]->fld_g, tmp[4]->fld_g, tmp[5]->fld_g};
    // ql, qi null: sat_adjust per cell with the Exner table of the thermodynamics for exner(p[k]); the counter of non-converged cells
    // is the caller's to add
    mhh_check(mhh_micro_nsw6_exec(&g, &p, fields.sp.at("qr")->fld_g, fields.sp.at("qs")->fld_g, fields.sp.at("qg")->fld_g,
                                  fields.sp.at("thl")->fld_g, fields.sp.at("qt")->fld_g, nullptr, nullptr,
                                  fields.st.at("qr")->fld_g, fields.st.at("qs")->fld_g, fields.st.at("qg")->fld_g,
                                  fields.st.at("thl")->fld_g, fields.st.at("qt")->fld_g, rr_bot_g, rs_bot_g, rg_bot_g,
                                  fields.rhoref_g, thermo.get_basestate_fld_g("pref"), thermo.get_basestate_fld_g("exner"), scratch, nullptr, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    for (auto& t : tmp)
        fields.release_tmp_g(t);
    stats.calc_tend(*fields.st.at("thl"), tend_name);
    stats.calc_tend(*fields.st.at("qt"),  tend_name);
    stats.calc_tend(*fields.st.at("qr"),  tend_name);
    stats.calc_tend(*fields.st.at("qs"),  tend_name);
    stats.calc_tend(*fields.st.at("qg"),  tend_name);
}

template<typename TF>
unsigned long Microphys_nsw6<TF>::get_time_limit(unsigned long idt, const double dt)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto work = fields.get_tmp_g();
    double cfl = 0;      // the largest of the three species', at least 1e-5
    mhh_check(mhh_micro_nsw6_cfl(&g, fields.sp.at("qr")->fld_g, fields.sp.at("qs")->fld_g, fields.sp.at("qg")->fld_g, fields.rhoref_g, dt, work->fld_g,
                                 &cfl, nullptr));
    fields.release_tmp_g(work);
    master.max(&cfl, 1);
    return idt * this->cflmax / cfl;
}

// rain plus snow plus graupel (:1194-1202), added on the host: three [ijcells] arrays once per surface update
template<typename TF>
void Microphys_nsw6<TF>::get_surface_rain_rate_g(TF* rr_out)
{
    auto& gd = grid.get_grid_data();
    std::vector<TF> sum(gd.ijcells), part(gd.ijcells);
    if (hipMemcpy(sum.data(), rr_bot_g, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
    for (TF* rate : {rs_bot_g, rg_bot_g})
    {
        if (hipMemcpy(part.data(), rate, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
        for (int ij=0; ij<gd.ijcells; ++ij)
            sum[ij] += part[ij];
    }
    if (hipMemcpy(rr_out, sum.data(), gd.ijcells*sizeof(TF), 1) != 0) throw std::runtime_error("hipMemcpy");
}

template<typename TF>
void Microphys_nsw6<TF>::prepare_device()
{
    auto& gd = grid.get_grid_data();
    for (TF** rate : {&rr_bot_g, &rs_bot_g, &rg_bot_g})
    {
        if (hipMalloc(reinterpret_cast<void**>(rate), gd.ijcells*sizeof(TF)) != 0) throw std::runtime_error("hipMalloc");
        if (hipMemset(*rate, 0, gd.ijcells*sizeof(TF)) != 0) throw std::runtime_error("hipMemset");
    }
}

template<typename TF>
void Microphys_nsw6<TF>::backward_device()
{
    auto& gd = grid.get_grid_data();
    if (hipMemcpy(rr_bot.data(), rr_bot_g, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
    if (hipMemcpy(rs_bot.data(), rs_bot_g, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
    if (hipMemcpy(rg_bot.data(), rg_bot_g, gd.ijcells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
}

template<typename TF>
void Microphys_nsw6<TF>::clear_device()
{
    for (TF* rate : {rr_bot_g, rs_bot_g, rg_bot_g})
        if (hipFree(rate) != 0) throw std::runtime_error("hipFree");
}
#endif
