// integration/adaptor_limiter.cxx -- replaces the USECUDA half of the reference's Limiter::exec (src/limiter.cu). The parity target is
// the CPU path, src/limiter.cxx:54-94: eps is the double epsilon narrowed to TF, dti = TF(1)/dt.
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "stats.h"
#include "limiter.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
template<typename TF>
void Limiter<TF>::exec(double dt, Stats<TF>& stats)
{
    if (limit_list.empty())
        return;
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    for (auto& name : limit_list)
    {
        mhh_check(mhh_limiter_exec(&g, fields.at.at(name)->fld_g, fields.ap.at(name)->fld_g, dt, nullptr));
        mhh_check(mhh_synchronize(nullptr));
        stats.calc_tend(*fields.at.at(name), tend_name);
    }
}
#endif
