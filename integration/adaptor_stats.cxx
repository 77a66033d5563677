// integration/adaptor_stats.cxx -- the device form of the sampling members of the reference's Stats<TF> (src/stats.cxx has no .cu:
// its GPU build copies every field to the host, src/model.cxx:444-451): initialize_masks (:1214-1227), set_mask_thres (:1264-1301),
// finalize_masks (:1229-1262), calc_stats (:1607-1890) and calc_tend (:1893-1919); calc_stats_2d keeps the reference's host form. Build
// src/stats.cxx with these members left out under USECUDA and this file in their place; the profiles land in the reference's own
// Mask::profs / tseries / nmask, so the NetCDF writer stays as it is. The mask words, the counts and the sums live in device memory
// allocated once here. The fluxes _w, _diff and _flux take the schemes from advec.get_switch() and diff.get_switch(); what Stats
// cannot see from where it stands -- whether there is a surface model, diff.tPr, advec.fluxlimit_list -- is mhh_stats_flux_config,
// which the model sets once after create. Not built: everything DESIGN.md §8 lists.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "stats.h"
#include "advec.h"
#include "diff.h"
#include "mhh_adaptor.h"
// Mask<TF> holds Netcdf_variable members by value, so instantiating Stats<TF> needs their definition. Where the NetCDF header is
// not installed (a type check of this file alone) empty stand-ins complete the types; a real build has netcdf.h and takes the
// reference's own.
#if __has_include(<netcdf.h>)
#include "netcdf_interface.h"
#else
class Netcdf_file {};
template<typename T> class Netcdf_variable {};
#endif

#ifdef USECUDA
// what the fluxes need and Stats<TF> has no reference to: boundary.get_switch() != "default", diff.tPr, advec.fluxlimit_list
struct Mhh_stats_flux_config { bool surface_model = true; double tPr = 1./3.; std::vector<std::string> fluxlimit_list; };
Mhh_stats_flux_config mhh_stats_flux_config;

// entry points the maintainer's build already links; declared here so that this file needs no HIP header
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipMemset(void* dst, int value, size_t size);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device, 2 = device to host, 3 = device to device

namespace
{
    struct Device
    {
        unsigned int* mfield = nullptr; unsigned int* mfield_bot = nullptr;
        void* zero2d = nullptr; int* nmask = nullptr; double* scratch = nullptr; double* sums = nullptr; double* csums = nullptr; void* out = nullptr;
        void* mean = nullptr; void* wmean = nullptr;             // the finished means of the variable in hand and of w: [nmasks][kcells]
        int nmasks = 0;
    };
    Device dev;

    template<class T> T* mhh_alloc(size_t n)
    {
        void* p = nullptr;
        if (hipMalloc(&p, n*sizeof(T)) != 0 || hipMemset(p, 0, n*sizeof(T)) != 0) throw std::runtime_error("hipMalloc");
        return static_cast<T*>(p);
    }
    template<typename TF, class GD>
    void mhh_stats_alloc(const GD& gd, const mhh_grid& g, int nmasks)
    {
        if (dev.mfield) return;
        if (nmasks > MHH_STATS_MAX_MASKS) throw std::runtime_error("mhh: more than MHH_STATS_MAX_MASKS masks");
        dev.nmasks = nmasks;
        dev.mfield = mhh_alloc<unsigned int>(gd.ncells); dev.mfield_bot = mhh_alloc<unsigned int>(gd.ijcells);
        dev.zero2d = mhh_alloc<TF>(gd.ijcells); dev.nmask = mhh_alloc<int>((size_t)nmasks*(2*gd.kcells + 1));
        dev.scratch = mhh_alloc<double>(mhh_stats_scratch_elems(&g, nmasks, MHH_STATS_MAX_JOBS));
        dev.sums = mhh_alloc<double>((size_t)MHH_STATS_MAX_JOBS*nmasks*gd.kcells); dev.csums = mhh_alloc<double>((size_t)2*nmasks*gd.kcells + 3*nmasks);
        dev.out = mhh_alloc<TF>((size_t)MHH_STATS_MAX_JOBS*nmasks*gd.kcells);
        dev.mean = mhh_alloc<TF>((size_t)nmasks*gd.kcells); dev.wmean = mhh_alloc<TF>((size_t)nmasks*gd.kcells);
        mhh_stats_device() = Mhh_stats_device{dev.mfield, dev.nmask, nmasks};      // Budget_2::exec_stats averages under the same words
    }
    inline int mhh_mask_index(unsigned int flag) { int n = 0; while ((1u << (2*n)) != flag) ++n; return n; }   // flag = 1 << 2n (:841-850)
    void mhh_d2h(void* dst, const void* src, size_t bytes) { if (hipMemcpy(dst, src, bytes, 2) != 0) throw std::runtime_error("hipMemcpy"); }
    void mhh_h2d(void* dst, const void* src, size_t bytes) { if (hipMemcpy(dst, src, bytes, 1) != 0) throw std::runtime_error("hipMemcpy"); }
    // master.sum over the ranks of n device doubles (one rank: nothing)
    void mhh_sum_ranks(Master& master, double* d, int n)
    {
        const MPI_data& md = master.get_MPI_data();
        if (md.npx*md.npy == 1) return;
        std::vector<double> h(n);
        mhh_d2h(h.data(), d, n*sizeof(double));
        master.sum(h.data(), n);
        mhh_h2d(d, h.data(), n*sizeof(double));
    }
}

template<typename TF>
void Stats<TF>::initialize_masks()
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_stats_alloc<TF>(gd, g, (int)masks.size());
    mhh_check(mhh_stats_mask_init(&g, dev.mfield, dev.mfield_bot, dev.nmasks, nullptr));
}

template<typename TF>
void Stats<TF>::set_mask_thres(std::string mask_name, Field3d<TF>& fld, Field3d<TF>& fldh, TF threshold, Stats_mask_type mode)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto it = masks.find(mask_name);
    if (it == masks.end())
        throw std::runtime_error("Invalid mask name in set_mask_thres()");
    if (mode != Stats_mask_type::Plus && mode != Stats_mask_type::Min)
        throw std::runtime_error("Invalid mask type in set_mask_thres()");
    // the reference hands fldh's fld_bot over, for a tmp field whatever it last held: zeros here (nmask_bot is overwritten below)
    mhh_check(mhh_stats_mask_thres(&g, dev.mfield, dev.mfield_bot, mhh_mask_index(it->second.flag), fld.fld_g, fldh.fld_g,
                                   fldh.fld_bot_g ? static_cast<const void*>(fldh.fld_bot_g) : dev.zero2d, threshold,
                                   mode == Stats_mask_type::Plus ? MHH_STATS_MASK_PLUS : MHH_STATS_MASK_MIN, nullptr));
}

template<typename TF>
void Stats<TF>::finalize_masks()
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    const int nm = dev.nmasks, kc = gd.kcells;
    TF* area = static_cast<TF*>(dev.out);
    mhh_check(mhh_stats_mask_count(&g, dev.mfield, dev.mfield_bot, nm, dev.csums, dev.scratch, nullptr));
    mhh_sum_ranks(master, dev.csums, 2*nm*kc);
    mhh_check(mhh_stats_mask_finish(&g, nm, dev.csums, dev.nmask, dev.nmask + (size_t)nm*2*kc, area, area + (size_t)nm*kc, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    for (auto& it : masks)
    {
        const int n = mhh_mask_index(it.second.flag);
        mhh_d2h(it.second.nmask.data(),  dev.nmask + ((size_t)n*2 + 0)*kc, kc*sizeof(int));
        mhh_d2h(it.second.nmaskh.data(), dev.nmask + ((size_t)n*2 + 1)*kc, kc*sizeof(int));
        it.second.nmask_bot = it.second.nmaskh[gd.kstart];
        if (std::find(varlist.begin(), varlist.end(), "area") != varlist.end())
            mhh_d2h(it.second.profs.at("area").data.data(), area + (size_t)n*kc, kc*sizeof(TF));
        if (std::find(varlist.begin(), varlist.end(), "areah") != varlist.end())
            mhh_d2h(it.second.profs.at("areah").data.data(), area + ((size_t)nm + n)*kc, kc*sizeof(TF));
    }
}

namespace
{
    // sums, the sum over the ranks, finish; then profile `names[j]` of every mask from out[j][mask][kcells]
    template<typename TF, class Masks>
    void mhh_stats_run(Master& master, const mhh_grid& g, Masks& masks, const std::vector<mhh_stats_job>& jobs, const std::vector<std::string>& names, int kcells)
    {
        const int nm = dev.nmasks, nj = (int)jobs.size();
        mhh_check(mhh_stats_sums(&g, dev.mfield, nm, jobs.data(), nj, dev.sums, dev.scratch, nullptr));
        mhh_sum_ranks(master, dev.sums, nj*nm*kcells);
        mhh_check(mhh_stats_finish(&g, nm, jobs.data(), nj, dev.sums, dev.nmask, dev.out, nullptr));
        mhh_check(mhh_synchronize(nullptr));
        for (auto& it : masks)
        {
            const int n = mhh_mask_index(it.second.flag);
            for (int j=0; j<nj; ++j)
                mhh_d2h(it.second.profs.at(names[j]).data.data(), static_cast<TF*>(dev.out) + ((size_t)j*nm + n)*kcells, kcells*sizeof(TF));
        }
    }
}

template<typename TF>
void Stats<TF>::calc_stats(const std::string& varname, const Field3d<TF>& fld, const TF offset, const TF threshold)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto listed = [&](const std::string& name) { return std::find(varlist.begin(), varlist.end(), name) != varlist.end(); };
    auto job = [&](int op, const void* mean) { mhh_stats_job j{}; j.fld = fld.fld_g; j.mean = mean; j.loc = fld.loc[2]; j.op = op; j.offset = offset; j.threshold = threshold; return j; };
    const int nm = dev.nmasks, kc = gd.kcells;
    // pass A: the mean, which pass B and the fluxes read from the device (a copy of its own; w's is kept for the fluxes of the others)
    if (listed(varname))
    {
        mhh_stats_run<TF>(master, g, masks, {job(MHH_STATS_MEAN, nullptr)}, {varname}, kc);
        if (hipMemcpy(dev.mean, dev.out, (size_t)nm*kc*sizeof(TF), 3) != 0) throw std::runtime_error("hipMemcpy");
        if (varname == "w" && hipMemcpy(dev.wmean, dev.out, (size_t)nm*kc*sizeof(TF), 3) != 0) throw std::runtime_error("hipMemcpy");
    }
    const void* mean_g = dev.mean;
    std::vector<mhh_stats_job> jobs; std::vector<std::string> names;
    for (int power=2; power<=4; ++power)
        if (listed(varname + "_" + std::to_string(power)) && !listed(varname))
            throw std::runtime_error("mhh: a moment of " + varname + " needs its mean in the varlist");
    for (int power=2; power<=4; ++power)
        if (listed(varname + "_" + std::to_string(power))) { jobs.push_back(job(power, mean_g)); names.push_back(varname + "_" + std::to_string(power)); }
    if (listed(varname + "_frac")) { jobs.push_back(job(MHH_STATS_FRAC, nullptr)); names.push_back(varname + "_frac"); }
    if (listed(varname + "_grad")) { jobs.push_back(job(MHH_STATS_GRAD, nullptr)); names.push_back(varname + "_grad"); }
    if (!jobs.empty())
        mhh_stats_run<TF>(master, g, masks, jobs, names, kc);
    // the fluxes: Fields::exec_stats samples w first, so its mean under flagh is in dev.wmean by now
    if (listed(varname + "_w") || listed(varname + "_diff") || listed(varname + "_flux"))
    {
        if (fld.loc[2] != 0) throw std::runtime_error("mhh: cannot deliver the flux of a half-level variable");
        if (!(listed(varname) && listed(varname + "_w") && listed(varname + "_diff")))
            throw std::runtime_error("mhh: the fluxes of " + varname + " need its mean, _w and _diff in the varlist");
        const Advection_type at = advec.get_switch();
        const Diffusion_type dt = diff.get_switch();
        if (at != Advection_type::Advec_2 && at != Advection_type::Advec_2i5) throw std::runtime_error("mhh: the resolved flux of this advection scheme is not built");
        if (dt != Diffusion_type::Diff_2 && dt != Diffusion_type::Diff_smag2) throw std::runtime_error("mhh: the diffusive flux of this diffusion scheme is not built");
        const Mhh_stats_flux_config& c = mhh_stats_flux_config;
        const bool smag = (dt == Diffusion_type::Diff_smag2);
        const bool momentum = (fld.loc[0] == 1 || fld.loc[1] == 1);
        mhh_stats_job base = job(MHH_STATS_FLUX_W, mean_g);
        base.kind = fld.loc[0] == 1 ? 1 : (fld.loc[1] == 1 ? 2 : 0);
        base.w = fields.mp.at("w")->fld_g; base.wmean = dev.wmean;
        base.evisc = smag ? fields.sd.at("evisc")->fld_g : nullptr; base.flux_bot = fld.flux_bot_g; base.flux_top = fld.flux_top_g;
        base.surface_model = c.surface_model; base.tPr = c.tPr; base.visc = (smag && momentum) ? fields.visc : fld.visc;
        base.limit = std::find(c.fluxlimit_list.begin(), c.fluxlimit_list.end(), varname) != c.fluxlimit_list.end();
        mhh_stats_job jw = base, jd = base, js = base;
        jw.scheme = (at == Advection_type::Advec_2) ? MHH_ADVEC_2 : MHH_ADVEC_2I5;
        jd.op = MHH_STATS_FLUX_DIFF; jd.scheme = smag ? MHH_DIFF_SMAG2 : MHH_DIFF_2;
        js.op = MHH_STATS_FLUX_SUM; js.a = 0; js.b = 1;
        std::vector<mhh_stats_job> fj = {jw, jd}; std::vector<std::string> fn = {varname + "_w", varname + "_diff"};
        if (listed(varname + "_flux")) { fj.push_back(js); fn.push_back(varname + "_flux"); }
        mhh_stats_run<TF>(master, g, masks, fj, fn, kc);
    }
    if (listed(varname + "_path") || listed(varname + "_cover"))
    {
        double* colsums = dev.csums + (size_t)2*nm*kc;
        mhh_check(mhh_stats_columns(&g, dev.mfield, nm, fld.fld_g, fld.loc[2], offset, threshold, fields.rhoref_g, colsums, dev.scratch, nullptr));
        mhh_sum_ranks(master, colsums, 3*nm);
        mhh_check(mhh_stats_columns_finish(&g, nm, colsums, dev.out, nullptr));
        mhh_check(mhh_synchronize(nullptr));
        std::vector<TF> h((size_t)nm*2);
        mhh_d2h(h.data(), dev.out, h.size()*sizeof(TF));
        for (auto& m : masks)
        {
            const int n = mhh_mask_index(m.second.flag);
            if (listed(varname + "_cover")) m.second.tseries.at(varname + "_cover").data = h[n*2];
            if (listed(varname + "_path"))  m.second.tseries.at(varname + "_path").data = h[n*2 + 1];
        }
    }
}

template<typename TF>
void Stats<TF>::calc_tend(Field3d<TF>& fld, const std::string& tend_name)
{
    if (!doing_tendency)
        return;
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    const std::string name = fld.name + "_" + tend_name;
    if (std::find(varlist.begin(), varlist.end(), name) == varlist.end())
        return;
    tendency_order.at(fld.name).push_back(tend_name);
    mhh_stats_job j{}; j.fld = fld.fld_g; j.loc = fld.loc[2]; j.op = MHH_STATS_MEAN;
    mhh_stats_run<TF>(master, g, masks, {j}, {name}, gd.kcells);
}

// the members alone: the class itself is instantiated by src/stats.cxx
#define MHH_STATS_MEMBERS(TF) \
    template void Stats<TF>::initialize_masks(); \
    template void Stats<TF>::set_mask_thres(std::string, Field3d<TF>&, Field3d<TF>&, TF, Stats_mask_type); \
    template void Stats<TF>::finalize_masks(); \
    template void Stats<TF>::calc_stats(const std::string&, const Field3d<TF>&, const TF, const TF); \
    template void Stats<TF>::calc_tend(Field3d<TF>&, const std::string&);
MHH_STATS_MEMBERS(double)
MHH_STATS_MEMBERS(float)
#endif
