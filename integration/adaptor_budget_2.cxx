// integration/adaptor_budget_2.cxx -- the device form of Budget_2<TF>::exec_stats (src/budget_2.cxx:1414-1818; the file has no .cu:
// the reference's GPU build runs it on the host after backward_device()). Build src/budget_2.cxx with exec_stats left out under
// USECUDA and this file in its place. The three calc_mask_mean_profile calls are mhh_budget_2_model_sums + _model_finish, b->fld_mean
// and p->fld_mean are mhh_field_mean_profile, and every calc_* loop with the calc_mask_stats that follows it is mhh_budget_2_sums +
// mhh_budget_2_finish; between a sums call and its finish call the double sums go through master.sum. The group bits follow create()
// (:1315-1412). The profiles land in the reference's own Mask::profs, so the NetCDF writer stays as it is. The mask words and the
// counts are the ones adaptor_stats.cxx left on the device (mhh_stats_device() of mhh_adaptor.h): Stats::finalize_masks has run by
// the time Model calls exec_stats. Not built: the DNS diffusion terms (diff_2 / diff_4), which are refused here as the library does.
#include <stdexcept>
#include <string>
#include <vector>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "stats.h"
#include "thermo.h"
#include "diff.h"
#include "advec.h"
#include "force.h"
#include "budget.h"
#include "budget_2.h"
#include "mhh_adaptor.h"
#if __has_include(<netcdf.h>)
#include "netcdf_interface.h"
#else
class Netcdf_file {};
template<typename T> class Netcdf_variable {};
#endif

#ifdef USECUDA
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipMemset(void* dst, int value, size_t size);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device, 2 = device to host

namespace
{
    struct Budget_device { double* scratch = nullptr; double* mscratch = nullptr; double* sums = nullptr; void* model = nullptr; void* means = nullptr; void* out = nullptr; };
    Budget_device bdev;

    template<class T> T* mhh_balloc(size_t n)
    {
        void* p = nullptr;
        if (hipMalloc(&p, n*sizeof(T)) != 0 || hipMemset(p, 0, n*sizeof(T)) != 0) throw std::runtime_error("hipMalloc");
        return static_cast<T*>(p);
    }
    inline int mhh_budget_mask_index(unsigned int flag) { int n = 0; while ((1u << (2*n)) != flag) ++n; return n; }   // flag = 1 << 2n (src/stats.cxx:841-850)
    // master.sum over the ranks of n device values (one rank: nothing)
    template<class T>
    void mhh_budget_sum_ranks(Master& master, T* d, int n)
    {
        const MPI_data& md = master.get_MPI_data();
        if (md.npx*md.npy == 1) return;
        std::vector<T> h(n);
        if (hipMemcpy(h.data(), d, n*sizeof(T), 2) != 0) throw std::runtime_error("hipMemcpy");
        master.sum(h.data(), n);
        if (hipMemcpy(d, h.data(), n*sizeof(T), 1) != 0) throw std::runtime_error("hipMemcpy");
    }
}

template<typename TF>
void Budget_2<TF>::exec_stats(Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    const Mhh_stats_device& sd = mhh_stats_device();
    if (!sd.mfield) throw std::runtime_error("mhh: Budget_2::exec_stats needs the masks of Stats::finalize_masks on the device");
    const int nm = sd.nmasks, kc = gd.kcells;

    // the groups of create() (:1315-1412)
    unsigned int groups = MHH_BUDGET_KE | MHH_BUDGET_SHEAR | MHH_BUDGET_TURB | MHH_BUDGET_PRES | MHH_BUDGET_RDSTR;
    if (force.get_switch_lspres() == Large_scale_pressure_type::Geo_wind) groups |= MHH_BUDGET_COR;
    const Diffusion_type dt = diff.get_switch();
    if (dt == Diffusion_type::Diff_smag2) groups |= MHH_BUDGET_DIFF;
    else if (dt != Diffusion_type::Disabled) throw std::runtime_error("mhh: the DNS diffusion terms of Budget_2 are not built");
    const bool has_thermo = thermo.get_switch() != "0";
    if (has_thermo)
    {
        groups |= MHH_BUDGET_BUOY | MHH_BUDGET_BW_BUOY | MHH_BUDGET_PRES_S;
        if (advec.get_switch() != Advection_type::Disabled) groups |= MHH_BUDGET_ADV_S;
    }
    const int np = mhh_budget_2_nprofs(groups);

    if (!bdev.scratch)
    {
        bdev.scratch = mhh_balloc<double>(mhh_budget_2_scratch_elems(&g, nm));
        bdev.mscratch = mhh_balloc<double>(mhh_field_mean_scratch_elems(&g, 2));
        bdev.sums = mhh_balloc<double>((size_t)mhh_budget_2_nprofs(0x7ffu)*nm*kc);
        bdev.model = mhh_balloc<TF>((size_t)3*nm*kc); bdev.means = mhh_balloc<TF>((size_t)2*kc);
        bdev.out = mhh_balloc<TF>((size_t)mhh_budget_2_nprofs(0x7ffu)*nm*kc);
    }
    TF* model = static_cast<TF*>(bdev.model); TF* means = static_cast<TF*>(bdev.means); TF* out = static_cast<TF*>(bdev.out);
    const TF* u = fields.mp.at("u")->fld_g; const TF* v = fields.mp.at("v")->fld_g; const TF* w = fields.mp.at("w")->fld_g;

    // stats.calc_mask_mean_profile(umodel | vmodel | wmodel, m, ...) of every mask (:1426-1428)
    mhh_check(mhh_budget_2_model_sums(&g, sd.mfield, nm, u, v, w, bdev.sums, bdev.scratch, nullptr));
    mhh_budget_sum_ranks(master, bdev.sums, 3*nm*kc);
    mhh_check(mhh_budget_2_model_finish(&g, nm, bdev.sums, sd.nmask, model, nullptr));

    mhh_budget_2_desc d{};
    d.u = u; d.v = v; d.w = w; d.p = fields.sd.at("p")->fld_g;
    d.evisc = fields.sd.count("evisc") ? fields.sd.at("evisc")->fld_g : nullptr;
    d.u_fluxbot = fields.mp.at("u")->flux_bot_g; d.v_fluxbot = fields.mp.at("v")->flux_bot_g;
    d.umodel = model; d.vmodel = model + (size_t)nm*kc; d.wmodel = model + (size_t)2*nm*kc;
    d.utrans = gd.utrans; d.vtrans = gd.vtrans; d.fc = force.get_coriolis_parameter();
    d.order = 2; d.diff_scheme = (dt == Diffusion_type::Diff_smag2) ? MHH_DIFF_SMAG2 : MHH_DIFF_2; d.groups = groups;

    std::shared_ptr<Field3d<TF>> b;
    if (has_thermo)
    {
        // thermo.get_thermo_field(*b, "b", true, true) and the two calc_mean_profile calls (:1700-1705); a rank holds its share
        b = fields.get_tmp_g();
        thermo.get_thermo_field_g(*b, "b", true);
        const void* flds[2] = {b->fld_g, d.p}; void* profs[2] = {means, means + kc};
        mhh_check(mhh_field_mean_profile(&g, flds, 2, profs, bdev.mscratch, nullptr));
        mhh_budget_sum_ranks(master, means, 2*kc);
        d.b = b->fld_g; d.bmean = means; d.pmean = means + kc;
    }

    mhh_check(mhh_budget_2_sums(&g, sd.mfield, nm, &d, bdev.sums, bdev.scratch, nullptr));
    mhh_budget_sum_ranks(master, bdev.sums, np*nm*kc);
    mhh_check(mhh_budget_2_finish(&g, nm, &d, bdev.sums, sd.nmask, out, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    if (b) fields.release_tmp_g(b);

    for (auto& m : stats.get_masks())
    {
        const int n = mhh_budget_mask_index(m.second.flag);
        for (int j=0; j<np; ++j)
        {
            auto it = m.second.profs.find(mhh_budget_2_prof_name(groups, j, nullptr));
            if (it == m.second.profs.end()) continue;                 // not in the varlist (calc_mask_stats returns, src/stats.cxx:1350-1390)
            if (hipMemcpy(it->second.data.data(), out + ((size_t)j*nm + n)*kc, kc*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
        }
    }
}

// the member alone: the class itself is instantiated by src/budget_2.cxx
template void Budget_2<double>::exec_stats(Stats<double>&);
template void Budget_2<float>::exec_stats(Stats<float>&);
#endif
