// ref_stats_shim.cpp -- TEST infrastructure: the reference's own Stats kernels behind a C interface.
//
// Compiled by tests/stats_ref.py into a temporary directory with the reference's src and include directories and
// tests/stubs_syntax_only on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections
// collected at link time); nothing compiled from it is kept. The translation unit is included in place, so that the kernels of its
// anonymous namespace (calc_mask_thres, calc_nmask, calc_area, calc_mean, calc_mean_2d, calc_moment, calc_frac, calc_path,
// calc_cover, set_fillvalue_prof) are visible here. What is written here is the calls only, with the arguments
// Stats::set_mask_thres (:1264-1301), finalize_masks (:1229-1262), calc_stats (:1607-1890) and calc_stats_2d (:1921-1937) pass.
// calc_grad_2nd is a member of Stats<TF> and cannot be reached without an object: tests/stats_ref.py restates that one loop in NumPy
// float64, in row order. calc_liquid_water_h of thermo_moist.cxx is behind ref_stats_qlh_shim.cpp, a translation unit of its own.
#include "stats.cxx"
#include "ref_shim.h"

namespace
{
    template<typename TF>
    void thres(const Dims& d, int mode, unsigned int* mfield, unsigned int* mfield_bot, unsigned int flag, unsigned int flagh,
               const TF* fld, const TF* fldh, const TF* fld_bot, double threshold)
    {
        if (mode == 0)
            calc_mask_thres<TF, Stats_mask_type::Plus>(mfield, mfield_bot, flag, flagh, fld, fldh, fld_bot, TF(threshold),
                    d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells, d.kcells);
        else
            calc_mask_thres<TF, Stats_mask_type::Min>(mfield, mfield_bot, flag, flagh, fld, fldh, fld_bot, TF(threshold),
                    d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, d.ijcells, d.kcells);
    }

    // finalize_masks after the cyclic fills: calc_nmask over 0 .. kcells, nmask_bot = nmaskh[kstart], the two areas
    template<typename TF>
    void counts(const Dims& d, int ijtot, const unsigned int* mfield, const unsigned int* mfield_bot, unsigned int flag, unsigned int flagh,
                int* nmask, int* nmaskh, int* nmask_bot, TF* area, TF* areah)
    {
        calc_nmask<TF>(nmask, nmaskh, *nmask_bot, mfield, mfield_bot, flag, flagh, d.istart, d.iend, d.jstart, d.jend, 0, d.kcells,
                       d.icells, d.ijcells, d.kcells);
        *nmask_bot = nmaskh[d.kstart];
        const int sloc[3] = {0, 0, 0}, wloc[3] = {0, 0, 1};
        calc_area(area, sloc, nmask, d.kstart, d.kend, ijtot);
        calc_area(areah, wloc, nmaskh, d.kstart, d.kend, ijtot);
    }

    // one operation of calc_stats on one mask; prof enters zeroed. op: 0 mean (offset added, :1635), 2..4 moment, 5 frac
    template<typename TF>
    void prof(const Dims& d, int op, TF* prof, const TF* fld, const TF* mean, double offset, double threshold,
              const unsigned int* mfield, unsigned int flag, const int* nmask)
    {
        if (op == 0)
        {
            calc_mean(prof, fld, mfield, flag, nmask, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
            for (int k=0; k<d.kcells; ++k) prof[k] += TF(offset);
        }
        else if (op >= 2 && op <= 4)
            calc_moment(prof, fld, mean, TF(offset), mfield, flag, nmask, op, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        else
            calc_frac(prof, fld, TF(offset), TF(threshold), mfield, flag, nmask, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        set_fillvalue_prof(prof, nmask, d.kstart, d.kcells);
    }

    // out[0] = cover (:1863), out[1] = path / nmask_proj (:1837), out[2] = nmask_proj, out[3] = the path sum
    template<typename TF>
    void columns(const Dims& d, TF* out, const TF* fld, const TF* dz, const TF* rho, double offset, double threshold,
                 const unsigned int* mfield, unsigned int flag, const int* nmask)
    {
        std::pair<int, int> cover = calc_cover(fld, TF(offset), TF(threshold), mfield, flag, nmask, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend,
                                               d.icells, d.ijcells);
        out[0] = (cover.second > 0) ? TF(cover.first)/TF(cover.second) : 0.;
        std::pair<TF, int> path = calc_path(fld, dz, rho, mfield, flag, nmask, d.istart, d.iend, d.jstart, d.jend, d.kstart, d.kend, d.icells, d.ijcells);
        out[1] = path.first / path.second;
        out[2] = TF(path.second);
        out[3] = path.first;
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API void ref_stats_thres(int dtype, const Dims* d, int mode, unsigned int* mfield, unsigned int* mfield_bot, unsigned int flag, unsigned int flagh,
                             const void* fld, const void* fldh, const void* fld_bot, double threshold)
{
    if (dtype == 0) thres(*d, mode, mfield, mfield_bot, flag, flagh, C64(fld), C64(fldh), C64(fld_bot), threshold);
    else            thres(*d, mode, mfield, mfield_bot, flag, flagh, C32(fld), C32(fldh), C32(fld_bot), threshold);
}
REF_API void ref_stats_counts(int dtype, const Dims* d, int ijtot, const unsigned int* mfield, const unsigned int* mfield_bot, unsigned int flag,
                              unsigned int flagh, int* nmask, int* nmaskh, int* nmask_bot, void* area, void* areah)
{
    if (dtype == 0) counts(*d, ijtot, mfield, mfield_bot, flag, flagh, nmask, nmaskh, nmask_bot, F64(area), F64(areah));
    else            counts(*d, ijtot, mfield, mfield_bot, flag, flagh, nmask, nmaskh, nmask_bot, F32(area), F32(areah));
}
REF_API void ref_stats_prof(int dtype, const Dims* d, int op, void* out, const void* fld, const void* mean, double offset, double threshold,
                            const unsigned int* mfield, unsigned int flag, const int* nmask)
{
    if (dtype == 0) prof(*d, op, F64(out), C64(fld), C64(mean), offset, threshold, mfield, flag, nmask);
    else            prof(*d, op, F32(out), C32(fld), C32(mean), offset, threshold, mfield, flag, nmask);
}
REF_API void ref_stats_columns(int dtype, const Dims* d, void* out, const void* fld, const void* dz, const void* rho, double offset, double threshold,
                               const unsigned int* mfield, unsigned int flag, const int* nmask)
{
    if (dtype == 0) columns(*d, F64(out), C64(fld), C64(dz), C64(rho), offset, threshold, mfield, flag, nmask);
    else            columns(*d, F32(out), C32(fld), C32(dz), C32(rho), offset, threshold, mfield, flag, nmask);
}
REF_API double ref_stats_mean_2d(int dtype, const Dims* d, int itot, int jtot, const void* fld, double offset)
{
    if (dtype == 0) { double o; calc_mean_2d(o, C64(fld), d->istart, d->iend, d->jstart, d->jend, d->icells, itot, jtot); o += offset; return o; }
    float o; calc_mean_2d(o, C32(fld), d->istart, d->iend, d->jstart, d->jend, d->icells, itot, jtot); o += float(offset); return o;
}
