// tests/cpp/host_budget.cpp -- Budget_2_sampler, the C++ host class of Budget_2 in microhh_amd/host/mhh_host.h. Built and run by
// tests/test_budget_cpp_host.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit
// for bit, with the same calls made through the Python driver.
//   host_budget IN OUT itot jtot ktot utrans vtrans fc
// IN: u v w p evisc b [ncells each], ufluxbot vfluxbot [ijcells each], then z zh dz dzh dzi dzhi [kcells each].
// Masks default, wpos (w > 0 on both levels, Plus), wneg (Min). Every group, diff_smag2.
// OUT, per mask: umodel vmodel wmodel, then every profile in the order of mhh_budget_2_prof_name [kcells each].
// gc = (3, 3, 1), second order, double.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "../../microhh_amd/host/mhh_host.h"

using namespace mhh_host;
typedef double TF;
#define HIPCHK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); std::exit(2); } } while (0)
static TF* up(const std::vector<TF>& v) { TF* d; HIPCHK(hipMalloc(&d, v.size()*sizeof(TF))); HIPCHK(hipMemcpy(d, v.data(), v.size()*sizeof(TF), hipMemcpyHostToDevice)); return d; }
template<class T> static T* dev(size_t n) { T* d; HIPCHK(hipMalloc(&d, n*sizeof(T))); HIPCHK(hipMemset(d, 0, n*sizeof(T))); return d; }

int main(int argc, char** argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 6; gd.jcells = gd.jtot + 6; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = 3; gd.kstart = 1; gd.iend = 3 + gd.itot; gd.jend = 3 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = gd.ysize = 3200.; gd.zsize = 1200.; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        for (const char* n : {"u", "v", "w"}) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); fields.mp[n] = f; }
        for (const char* n : {"p", "evisc"}) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); fields.sd[n] = f; }
        TF* b = up(rd(n3));
        fields.mp.at("u")->flux_bot_g = up(rd(n2)); fields.mp.at("v")->flux_bot_g = up(rd(n2));
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        Stats_sampler<TF> stats(grid, fields);
        const char* masks[3] = {"default", "wpos", "wneg"};
        for (const char* m : masks) stats.add_mask(m);
        stats.mfield_g = dev<unsigned int>(n3); stats.mfield_bot_g = dev<unsigned int>(n2); stats.zero2d_g = dev<TF>(n2);
        stats.nmask_g = dev<int>(stats.nmask_elems()); stats.work_g = dev<double>(stats.work_elems()); stats.prof_g = dev<TF>(stats.prof_elems());
        Field3d<TF>& w = *fields.mp.at("w");
        stats.initialize_masks();
        stats.set_mask_thres("wpos", w, w, TF(0.), Stats_mask_type::Plus);
        stats.set_mask_thres("wneg", w, w, TF(0.), Stats_mask_type::Min);
        stats.finalize_masks();

        Budget_2_sampler<TF> budget(grid, fields, stats);
        budget.groups = 0x800u;
        bool refused = false;
        try { budget.nprofs(); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        budget.groups = 0x7ffu; budget.b_g = b;
        budget.utrans = std::atof(argv[6]); budget.vtrans = std::atof(argv[7]); budget.fc = std::atof(argv[8]);
        budget.work_g = dev<double>(budget.work_elems()); budget.prof_g = dev<TF>(budget.prof_elems());
        budget.exec_stats();
        HIPCHK(hipDeviceSynchronize());
        for (int bad=0; bad<2; ++bad)
        {
            refused = false;
            try { bad ? budget.get_model(3, "default") : budget.get_model(0, "nosuch"); } catch (const std::runtime_error&) { refused = true; }
            if (!refused) return 7;
        }

        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        auto wr = [&](const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost));
                                               if (std::fwrite(v.data(), sizeof(TF), n, out) != n) std::exit(4); };
        for (const char* m : masks)
        {
            for (int i=0; i<3; ++i) wr(budget.get_model(i, m), nk);
            for (int n=0; n<budget.nprofs(); ++n) wr(budget.get_prof(m, mhh_budget_2_prof_name(budget.groups, n, nullptr)), nk);
        }
        std::fclose(out);
        std::printf("host_budget ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
