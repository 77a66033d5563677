// tests/cpp/host_micro.cpp -- Microphys_2mom_warm and Limiter through the C++ host classes of microhh_amd/host/mhh_host.h. Built and
// run by tests/test_cpp_host_micro.py, which hands the inputs over in a file of doubles and compares what this program writes back,
// bit for bit, with the same calls made through the Python binding.
//   host_micro IN OUT itot jtot ktot Nc0 dt subdt idt
// IN: thl qt qr nr thlt qtt qrt nrt [ncells each], then pref exnref rhoref [kcells each], then z zh dz dzh dzi dzhi [kcells each].
// exec(thermo, dt), Limiter::exec(subdt) for qr and nr, get_time_limit(idt, dt). OUT: qr nr thlt qtt qrt nrt [ncells each], rr_bot
// [ijcells], the time limit as a double.
// gc = (3, 3, 1), second order, double, the domain of rico (12800 x 12800 x 4000 m).
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 10, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 12800., 12800., 4000.);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        const double Nc0 = std::atof(argv[6]), dt = std::atof(argv[7]), subdt = std::atof(argv[8]);
        const unsigned long idt = std::strtoul(argv[9], nullptr, 10);
        Reader rd(argv[1]);
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        for (const char* n : {"thl", "qt", "qr", "nr"}) fields.sp[n] = mk();
        for (const char* n : {"thl", "qt", "qr", "nr"}) fields.st[n] = mk();
        Thermo_moist<TF> thermo(grid, fields);
        thermo.pref_g = up(rd(nk)); thermo.exnref_g = up(rd(nk)); fields.rhoref_g = up(rd(nk));
        thermo.nonconv_g = dev<int>(1);
        read_metrics(grid, rd);
        rd.close();

        Microphys_2mom_warm<TF> micro(grid, fields);
        micro.Nc0 = Nc0;
        micro.rr_bot_g = dev<TF>(n2);
        for (TF*& s : micro.scratch_g) s = dev<TF>(n3);
        micro.work_g = dev<char>(mhh_reduce_work_bytes());
        Limiter<TF> limiter(grid, fields);
        limiter.limit_list = {"qr", "nr"};
        if (micro.get_switch() != "2mom_warm" || micro.get_surface_rain_rate() != micro.rr_bot_g) return 6;

        micro.exec(thermo, dt);
        limiter.exec(subdt);
        const unsigned long limit = micro.get_time_limit(idt, dt);
        bool refused = false;
        micro.Nc0 = 0;
        try { micro.exec(thermo, dt); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        HIPCHK(hipDeviceSynchronize());
        int nonconv = 0; HIPCHK(hipMemcpy(&nonconv, thermo.nonconv_g, sizeof(int), hipMemcpyDeviceToHost));
        if (nonconv) return 8;
        Writer wr(argv[2]);
        wr(fields.sp["qr"]->fld_g, n3); wr(fields.sp["nr"]->fld_g, n3);
        for (const char* n : {"thl", "qt", "qr", "nr"}) wr(fields.st[n]->fld_g, n3);
        wr(micro.rr_bot_g, n2);
        wr.host({(double)limit});
        wr.close();
        std::printf("host_micro ok\n");
        return 0;
    });
}
