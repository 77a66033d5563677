// tests/cpp/host_source.cpp -- Decay::exec and Source::create / exec / update through the C++ host classes of
// microhh_amd/host/mhh_host.h. Built and run by tests/test_cpp_host_source.py, which hands the inputs over in a file of doubles and
// compares the tendencies and norms this program writes back, bit for bit, with the same calls made through the Python binding.
//   host_source IN OUT itot jtot ktot xsize ysize zsize nplain nprofile dt
// IN: z zh dz dzh dzi dzhi [kcells each]; s0 s1 s2 st0 st1 st2 [ncells each]; rhoref [kcells]; three emission profiles [kcells each];
//     nplain + nprofile sources of 13 doubles: scalar swvmr profile_index x0 y0 z0 sigma_x sigma_y sigma_z line_x line_y line_z strength
// OUT: st0 st1 st2 after decay.exec(dt, stats); plain.exec(); prof.exec(); plain.update(moved x0, doubled strength); plain.exec();
//      then the norms of the plain sources after the update. gc = (3, 3, 1), second order, double.
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

static void fill(Source<TF>& src, const std::vector<double>& v, int n)
{
    src.swsource = n > 0;
    for (int m=0; m<n; ++m)
    {
        const double* d = v.data() + 13*m;
        src.sourcelist.push_back("s" + std::to_string((int)d[0]));
        src.sw_vmr.push_back(d[1] != 0); src.profile_index.push_back((int)d[2]);
        src.source_x0.push_back(d[3]); src.source_y0.push_back(d[4]); src.source_z0.push_back(d[5]);
        src.sigma_x.push_back(d[6]); src.sigma_y.push_back(d[7]); src.sigma_z.push_back(d[8]);
        src.line_x.push_back(d[9]); src.line_y.push_back(d[10]); src.line_z.push_back(d[11]); src.strength.push_back(d[12]);
    }
}

int main(int argc, char** argv)
{
    return run_main(argc, argv, 12, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]));
        const int nplain = std::atoi(argv[9]), nprof = std::atoi(argv[10]);
        const double dt = std::atof(argv[11]);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        Reader rd(argv[1]);
        read_metrics(grid, rd);
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        auto zero = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = dev<TF>(n3); return f; };
        for (const char* nm : {"u", "v", "w"}) { fields.mp[nm] = zero(); fields.mt[nm] = zero(); }
        for (const char* nm : {"s0", "s1", "s2"}) fields.sp[nm] = mk();
        for (const char* nm : {"s0", "s1", "s2"}) fields.st[nm] = mk();
        fields.rhoref = rd(nk);

        Source<TF> plain(grid, fields), prof(grid, fields);
        prof.sw_emission_profile = true;
        for (int p=0; p<3; ++p) prof.profile_z[p] = rd(nk);
        fill(plain, rd(13*(size_t)nplain), nplain);
        fill(prof, rd(13*(size_t)nprof), nprof);
        rd.close();
        plain.init(); plain.create(); prof.init(); prof.create();

        Stats stats;
        Decay<TF> decay(grid, fields);
        decay.dmap["s0"] = {600., Decay_type::exponential};
        decay.dmap["s1"] = {2.5, Decay_type::exponential};
        decay.dmap["s2"] = {1., Decay_type::disabled};
        decay.init(); decay.create(stats);
        if (!decay.has_mask("couvreux") || decay.has_mask("ql")) return 6;

        decay.exec(dt, stats);
        plain.exec(); prof.exec();
        for (int m=0; m<nplain; ++m) { plain.source_x0[m] += 137.; plain.strength[m] *= 2.; }
        plain.update(true, true);
        plain.exec();
        HIPCHK(hipDeviceSynchronize());
        Writer wr(argv[2]);
        for (const char* nm : {"s0", "s1", "s2"}) wr(fields.st[nm]->fld_g, n3);
        std::vector<double> norms;
        for (int m=0; m<nplain; ++m) norms.push_back(plain.get_norm(m));
        wr.host(norms);
        wr.close();
        std::printf("host_source ok: %d + %d sources\n", nplain, nprof);
        return 0;
    });
}
