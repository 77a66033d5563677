// tests/cpp/host_budget.cpp -- Budget_2_sampler, the C++ host class of Budget_2 in microhh_amd/host/mhh_host.h. Built and run by
// tests/test_budget_cpp_host.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit
// for bit, with the same calls made through the Python driver.
//   host_budget IN OUT itot jtot ktot utrans vtrans fc
// IN: u v w p evisc b [ncells each], ufluxbot vfluxbot [ijcells each], then z zh dz dzh dzi dzhi [kcells each].
// Masks default, wpos (w > 0 on both levels, Plus), wneg (Min). Every group, diff_smag2.
// OUT, per mask: umodel vmodel wmodel, then every profile in the order of mhh_budget_2_prof_name [kcells each].
// gc = (3, 3, 1), second order, double.
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 9, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 1200.);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        for (const char* n : {"u", "v", "w"}) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); fields.mp[n] = f; }
        for (const char* n : {"p", "evisc"}) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); fields.sd[n] = f; }
        TF* b = up(rd(n3));
        fields.mp.at("u")->flux_bot_g = up(rd(n2)); fields.mp.at("v")->flux_bot_g = up(rd(n2));
        read_metrics(grid, rd);
        rd.close();

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

        Writer wr(argv[2]);
        for (const char* m : masks)
        {
            for (int i=0; i<3; ++i) wr(budget.get_model(i, m), nk);
            for (int n=0; n<budget.nprofs(); ++n) wr(budget.get_prof(m, mhh_budget_2_prof_name(budget.groups, n, nullptr)), nk);
        }
        wr.close();
        std::printf("host_budget ok\n");
        return 0;
    });
}
