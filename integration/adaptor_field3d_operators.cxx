// integration/adaptor_field3d_operators.cxx -- replaces the USECUDA half of the reference's Field3d_operators
// (src/field3d_operators.cu): calc_mean_profile_g and calc_mean_g. The parity target is the CPU path,
// src/field3d_operators.cxx:45-66,132-155: double accumulators, here added in a fixed order of their own (deterministic; within
// the summation-order bound of the CPU loop). The reduction scratch is a tmp field of the reference's pool: a 3-D field holds
// far more than the [field][k][chunk] doubles of partial sums.
#include <stdexcept>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "field3d_operators.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 2 = device to host

template<typename TF>
void Field3d_operators<TF>::calc_mean_profile_g(TF* const prof, const TF* const fld)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    if (mhh_field_mean_scratch_elems(&g, 1)*sizeof(double) > (unsigned long long)gd.ncells*sizeof(TF)) throw std::runtime_error("mhh: tmp field too small for the reduction scratch");
    auto tmp = fields.get_tmp_g();
    const void* f[1] = {fld}; void* p[1] = {prof};
    mhh_check(mhh_field_mean_profile(&g, f, 1, p, tmp->fld_g, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    fields.release_tmp_g(tmp);
    // with npy > 1 each rank holds its share, already divided by the global itot*jtot: the caller's sum over the ranks of the
    // device profile (the reference's master.sum after the division, :65) completes it
}

template<typename TF>
TF Field3d_operators<TF>::calc_mean_g(const TF* const fld)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    auto tmp = fields.get_tmp_g();
    // the sum lands behind the partials, in the same tmp field
    const unsigned long long n = mhh_field_mean_scratch_elems(&g, 1);
    if ((n + 1)*sizeof(double) > (unsigned long long)gd.ncells*sizeof(TF)) throw std::runtime_error("mhh: tmp field too small for the reduction scratch");
    double* scratch = reinterpret_cast<double*>(tmp->fld_g);
    const void* f[1] = {fld};
    mhh_check(mhh_field_mean_sum(&g, f, 1, scratch + n, scratch, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    double sum = 0;
    if (hipMemcpy(&sum, scratch + n, sizeof(double), 2) != 0) throw std::runtime_error("hipMemcpy");
    fields.release_tmp_g(tmp);
    master.sum(&sum, 1);
    const TF mean = sum / (gd.itot * gd.jtot * gd.zsize);       // as src/field3d_operators.cxx:152
    return mean;
}
#endif
