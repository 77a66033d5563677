// integration/adaptor_source.cxx -- replaces the USECUDA half of the reference's Source (src/source.cu): exec. The parity target is the
// CPU path, src/source.cxx:355-432, which has the moving and time-varying sources that src/source.cu:134 refuses. The class has no
// member to keep a handle in, so the handles live here, one per Source object. Source::create stays the reference's (it reads the
// lists and the profiles); the library redoes calc_shape and calc_norm when the handle is made, at the first exec.
#include <map>
#include <vector>
#include <algorithm>
#include <stdexcept>
#include <string>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "source.h"
#include "timedep.h"
#include "timeloop.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
namespace
{
    std::map<const void*, mhh_source*>& mhh_source_handles() { static std::map<const void*, mhh_source*> h; return h; }
}

template<typename TF>
void Source<TF>::exec(Timeloop<TF>& timeloop)
{
    auto& gd = grid.get_grid_data();
    if (!swsource)
        return;
    const int n = (int)sourcelist.size();
    mhh_source*& handle = mhh_source_handles()[this];
    if (!handle)
    {
        std::vector<int> rows(unique_profile_indexes.begin(), unique_profile_indexes.end());
        std::vector<TF> prof;
        for (int i : rows) prof.insert(prof.end(), profile_z.at(i).begin(), profile_z.at(i).end());
        std::vector<mhh_source_desc> d(n);
        for (int m=0; m<n; ++m)
        {
            d[m] = mhh_source_desc{};
            d[m].scalar = mhh_scalar_index(fields, sourcelist[m]);
            d[m].swvmr = sw_vmr[m];
            d[m].profile_index = sw_emission_profile ? (int)(std::find(rows.begin(), rows.end(), profile_index[m]) - rows.begin()) : -1;
            d[m].x0 = source_x0[m]; d[m].y0 = source_y0[m]; d[m].z0 = source_z0[m];
            d[m].sigma_x = sigma_x[m]; d[m].sigma_y = sigma_y[m]; d[m].sigma_z = sigma_z[m];
            d[m].line_x = line_x[m]; d[m].line_y = line_y[m]; d[m].line_z = line_z[m]; d[m].strength = strength[m];
        }
        mhh_grid gh = mhh_make_grid(gd, master.get_MPI_data());       // the set-up reads HOST metrics
        gh.z = gd.z.data(); gh.zh = gd.zh.data(); gh.dz = gd.dz.data(); gh.dzh = gd.dzh.data(); gh.dzi = gd.dzi.data(); gh.dzhi = gd.dzhi.data();
        gh.dzi4 = gd.dzi4.data(); gh.dzhi4 = gd.dzhi4.data();
        mhh_check(mhh_source_create(&gh, d.data(), n, prof.empty() ? nullptr : prof.data(), (int)rows.size(), fields.rhoref.data(), nullptr, &handle));
    }
    if (swtimedep_location || swtimedep_strength)
    {
        std::vector<double> x(n), y(n), z(n), q(n);
        for (int m=0; m<n; ++m)
        {
            if (swtimedep_location)
            {
                tdep_source_x0.at("source_x0_" + std::to_string(m))->update_time_dependent(source_x0[m], timeloop);
                tdep_source_y0.at("source_y0_" + std::to_string(m))->update_time_dependent(source_y0[m], timeloop);
                tdep_source_z0.at("source_z0_" + std::to_string(m))->update_time_dependent(source_z0[m], timeloop);
            }
            if (swtimedep_strength)
                tdep_source_strength.at("source_strength_" + std::to_string(m))->update_time_dependent(strength[m], timeloop);
            x[m] = source_x0[m]; y[m] = source_y0[m]; z[m] = source_z0[m]; q[m] = strength[m];
        }
        mhh_check(mhh_source_update(handle, -1, swtimedep_location ? x.data() : nullptr, swtimedep_location ? y.data() : nullptr,
                                    swtimedep_location ? z.data() : nullptr, swtimedep_strength ? q.data() : nullptr, nullptr));
    }
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_fields f = mhh_make_fields(fields);
    mhh_check(mhh_source_exec(handle, &g, &f, nullptr));
}

template void Source<double>::exec(Timeloop<double>&);
template void Source<float>::exec(Timeloop<float>&);
#endif
