// integration/adaptor_decay.cxx -- replaces the USECUDA half of the reference's Decay (src/decay.cu): exec. The parity target is the CPU
// path, src/decay.cxx:97-111: every decaying scalar in one launch, then stats.calc_tend per scalar as there. get_mask stays the
// reference's host code; mhh_decay_couvreux_sums / _field with Stats' mask words on the device are the route of mhh_host.h.
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "stats.h"
#include "decay.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
template<typename TF>
void Decay<TF>::exec(double dt, Stats<TF>& stats)
{
    auto& gd = grid.get_grid_data();
    mhh_decay_params p{};
    for (auto& it : dmap)
        if (it.second.type == Decay_type::exponential)
        {
            const int n = mhh_scalar_index(fields, it.first);
            if (n < 0 || n >= MHH_MAX_SCALARS) throw std::runtime_error("mhh: decay of a scalar the library does not carry: " + it.first);
            p.exponential[n] = 1; p.timescale[n] = it.second.timescale;
        }
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_fields f = mhh_make_fields(fields);
    mhh_check(mhh_decay_exec(&g, &f, &p, dt, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    for (auto& it : dmap)
        if (it.second.type == Decay_type::exponential)
            stats.calc_tend(*fields.st.at(it.first), tend_name);
}

template void Decay<double>::exec(double, Stats<double>&);
template void Decay<float>::exec(double, Stats<float>&);
#endif
