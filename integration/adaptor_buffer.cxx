// integration/adaptor_buffer.cxx -- replaces the USECUDA half of the reference's Buffer (src/buffer.cu): exec. The parity target
// is the CPU path, src/buffer.cxx:37-58,163-206. prepare_device / clear_device stay the reference's (they fill bufferprofs_g).
// The two sponge tables are built on the host with the C library's pow, as calc_buffer does per level, and uploaded per call
// (2*kcells values); a maintainer who wants them cached adds two members next to bufferprofs_g.
#include <stdexcept>
#include <string>
#include <vector>
#include "grid.h"
#include "fields.h"
#include "master.h"
#include "buffer.h"
#include "stats.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device

template<typename TF>
void Buffer<TF>::exec(Stats<TF>& stats)
{
    if (!swbuffer) return;
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    mhh_grid gh = g;
    gh.z = gd.z.data(); gh.zh = gd.zh.data(); gh.dz = gd.dz.data(); gh.dzh = gd.dzh.data(); gh.dzi = gd.dzi.data(); gh.dzhi = gd.dzhi.data();
    gh.dzi4 = gd.dzi4.data(); gh.dzhi4 = gd.dzhi4.data();
    std::vector<TF> sg(2*gd.kcells);
    mhh_check(mhh_buffer_sigma_host(&gh, zstart, sigma, beta, 0, sg.data()));
    mhh_check(mhh_buffer_sigma_host(&gh, zstart, sigma, beta, 1, sg.data() + gd.kcells));
    auto tmp = fields.get_tmp_g();
    if (hipMemcpy(tmp->fld_g, sg.data(), sg.size()*sizeof(TF), 1) != 0) throw std::runtime_error("hipMemcpy");

    mhh_fields f = mhh_make_fields(fields);
    mhh_buffer_params b{};
    b.swbuffer = 1; b.bufferkstart = bufferkstart; b.bufferkstarth = bufferkstarth;
    b.sigma = tmp->fld_g; b.sigmah = tmp->fld_g + gd.kcells;
    // swupdate: the mean profiles of fields->exec() (src/model.cxx:351); otherwise the fixed profiles of create()
    b.abuf_u = swupdate ? fields.mp.at("u")->fld_mean_g : bufferprofs_g.at("u");
    b.abuf_v = swupdate ? fields.mp.at("v")->fld_mean_g : bufferprofs_g.at("v");
    b.abuf_w = swupdate ? fields.mp.at("w")->fld_mean_g : bufferprofs_g.at("w");
    int n = 0;
    for (auto& it : fields.sp)
        b.abuf_s[n++] = swupdate ? it.second->fld_mean_g : bufferprofs_g.at(it.first);
    mhh_check(mhh_buffer_exec(&g, &f, &b, nullptr));
    mhh_check(mhh_synchronize(nullptr));
    fields.release_tmp_g(tmp);

    stats.calc_tend(*fields.mt.at("u"), tend_name);
    stats.calc_tend(*fields.mt.at("v"), tend_name);
    stats.calc_tend(*fields.mt.at("w"), tend_name);
    for (auto it : fields.st)
        stats.calc_tend(*it.second, tend_name);
}
#endif
