// tests/cpp/host_stats.cpp -- Stats_sampler, the C++ host class of Stats in microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_stats.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit
// for bit, with the same calls made through the Python driver.
//   host_stats IN OUT itot jtot ktot threshold offset
// IN: u w q evisc [ncells each], bot fbot ftop [ijcells each], rhoref [kcells], then z zh dz dzh dzi dzhi [kcells each].
// Masks default, wpos (w > 0 on both levels, Plus), wneg (Min). u: mean 2 3 4 grad w diff flux with the offset (advec_2i5, smag2 with a
// surface model, flux_bot = fbot, flux_top = ftop, visc 1e-5, tPr 1/3); w (zh): mean 2 grad; q: mean frac
// path cover at the threshold; bot as a time series; w's "tendency" adv as calc_tend.
// OUT, per mask: nmask nmaskh (as doubles) area areah u u_2 u_3 u_4 u_grad w w_2 w_grad q q_frac w_adv u_w u_diff u_flux [kcells each], then
// q_cover q_path bot nmask_bot.
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
    if (argc != 8) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 6; gd.jcells = gd.jtot + 6; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = 3; gd.kstart = 1; gd.iend = 3 + gd.itot; gd.jend = 3 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = gd.ysize = 3200.; gd.zsize = 1200.; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const TF threshold = std::atof(argv[6]), offset = std::atof(argv[7]);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        Field3d<TF> u, w, q;
        u.fld_g = up(rd(n3)); w.fld_g = up(rd(n3)); q.fld_g = up(rd(n3));
        auto evisc = std::make_shared<Field3d<TF>>(); evisc->fld_g = up(rd(n3)); fields.sd["evisc"] = evisc;
        auto wf = std::make_shared<Field3d<TF>>(); wf->fld_g = w.fld_g; fields.mp["w"] = wf;
        TF* bot = up(rd(n2));
        u.flux_bot_g = up(rd(n2)); u.flux_top_g = up(rd(n2));
        fields.rhoref_g = up(rd(nk));
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        Stats_sampler<TF> stats(grid, fields);
        const char* masks[3] = {"default", "wpos", "wneg"};
        bool refused = false;
        for (const char* m : masks) stats.add_mask(m);
        stats.add_profs("u", "z", {"mean", "2", "3", "4", "grad", "w", "diff", "flux"});
        stats.flux_of("u").kind = 1; stats.flux_of("u").visc = 1.e-5;
        refused = false;
        try { stats.add_profs("wbad", "zh", {"mean", "w"}); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        stats.add_profs("w", "zh", {"mean", "2", "grad"});
        stats.add_profs("q", "z", {"mean", "frac", "path", "cover"});
        stats.add_time_series("bot");
        stats.add_tendency("w", "zh", "adv");
        refused = false;
        try { stats.add_profs("v", "z", {"mean", "flux"}); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        stats.mfield_g = dev<unsigned int>(n3); stats.mfield_bot_g = dev<unsigned int>(n2); stats.zero2d_g = dev<TF>(n2);
        stats.nmask_g = dev<int>(stats.nmask_elems()); stats.work_g = dev<double>(stats.work_elems()); stats.prof_g = dev<TF>(stats.prof_elems());

        stats.initialize_masks();
        stats.set_mask_thres("wpos", w, w, TF(0.), Stats_mask_type::Plus);
        stats.set_mask_thres("wneg", w, w, TF(0.), Stats_mask_type::Min);
        refused = false;
        try { stats.set_mask_thres("nosuch", w, w, TF(0.), Stats_mask_type::Plus); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        stats.finalize_masks();
        stats.calc_stats("w", w, TF(0.), TF(0.));
        stats.calc_stats("u", u, offset, TF(0.));
        stats.calc_stats("q", q, TF(0.), threshold);
        stats.calc_stats("notlisted", q, TF(0.), threshold);
        stats.calc_stats_2d("bot", bot, offset);
        stats.calc_tend(w, "w", "adv");
        HIPCHK(hipDeviceSynchronize());

        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        auto wr = [&](const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost));
                                               if (std::fwrite(v.data(), sizeof(TF), n, out) != n) std::exit(4); };
        auto wri = [&](const int* d, size_t n) { std::vector<int> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(int), hipMemcpyDeviceToHost));
                                                 std::vector<TF> f(v.begin(), v.end()); if (std::fwrite(f.data(), sizeof(TF), n, out) != n) std::exit(4); };
        for (const char* m : masks)
        {
            wri(stats.get_nmask(m, false), nk); wri(stats.get_nmask(m, true), nk);
            for (const char* p : {"area", "areah", "u", "u_2", "u_3", "u_4", "u_grad", "w", "w_2", "w_grad", "q", "q_frac", "w_adv", "u_w", "u_diff", "u_flux"}) wr(stats.get_prof(m, p), nk);
            wr(stats.get_time_series(m, "q_cover"), 1); wr(stats.get_time_series(m, "q_path"), 1); wr(stats.get_time_series(m, "bot"), 1);
            wri(stats.get_nmask_bot(m), 1);
        }
        std::fclose(out);
        std::printf("host_stats ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
