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
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 8, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 1200.);
        const TF threshold = std::atof(argv[6]), offset = std::atof(argv[7]);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        Field3d<TF> u, w, q;
        u.fld_g = up(rd(n3)); w.fld_g = up(rd(n3)); q.fld_g = up(rd(n3));
        auto evisc = std::make_shared<Field3d<TF>>(); evisc->fld_g = up(rd(n3)); fields.sd["evisc"] = evisc;
        auto wf = std::make_shared<Field3d<TF>>(); wf->fld_g = w.fld_g; fields.mp["w"] = wf;
        TF* bot = up(rd(n2));
        u.flux_bot_g = up(rd(n2)); u.flux_top_g = up(rd(n2));
        fields.rhoref_g = up(rd(nk));
        read_metrics(grid, rd);
        rd.close();

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

        Writer wr(argv[2]);
        auto wri = [&](const int* d, size_t n) { std::vector<int> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(int), hipMemcpyDeviceToHost));
                                                 wr.host(std::vector<TF>(v.begin(), v.end())); };
        for (const char* m : masks)
        {
            wri(stats.get_nmask(m, false), nk); wri(stats.get_nmask(m, true), nk);
            for (const char* p : {"area", "areah", "u", "u_2", "u_3", "u_4", "u_grad", "w", "w_2", "w_grad", "q", "q_frac", "w_adv", "u_w", "u_diff", "u_flux"}) wr(stats.get_prof(m, p), nk);
            wr(stats.get_time_series(m, "q_cover"), 1); wr(stats.get_time_series(m, "q_path"), 1); wr(stats.get_time_series(m, "bot"), 1);
            wri(stats.get_nmask_bot(m), 1);
        }
        wr.close();
        std::printf("host_stats ok\n");
        return 0;
    });
}
