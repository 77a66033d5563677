// tests/cpp/host_radiation.cpp -- Radiation_gcss through the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_radiation.py, which hands the inputs over in a file of doubles and compares what this program writes back,
// bit for bit, with the same calls made through the Python binding.
//   host_radiation IN OUT itot jtot ktot xka fr0 fr1 div lat lon day_of_year
// IN: thl qt thlt [ncells each], then pref exnref rhoref [kcells each], then z zh dz dzh dzi dzhi [kcells each].
// exec(thermo, day_of_year), get_radiation_field for lflx and sflx. OUT: thlt lflx sflx [ncells each], mu as a double.
// gc = (3, 3, 1), second order, double, the domain of dycoms (6400 x 6400 x 1500 m).
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 13, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 6400., 6400., 1500.);
        gd.lat = std::atof(argv[10]); gd.lon = std::atof(argv[11]);
        const double day_of_year = std::atof(argv[12]);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        for (const char* n : {"thl", "qt"}) fields.sp[n] = mk();
        fields.st["thl"] = mk();
        Thermo_moist<TF> thermo(grid, fields);
        thermo.pref_g = up(rd(nk)); thermo.exnref_g = up(rd(nk)); fields.rhoref_g = up(rd(nk));
        thermo.nonconv_g = dev<int>(1);
        read_metrics(grid, rd);
        rd.close();

        Radiation_gcss<TF> radiation(grid, fields);
        radiation.xka = std::atof(argv[6]); radiation.fr0 = std::atof(argv[7]); radiation.fr1 = std::atof(argv[8]); radiation.div = std::atof(argv[9]);
        for (TF*& s : radiation.scratch_g) s = dev<TF>(n3);
        if (radiation.get_switch() != "gcss" || radiation.get_time_limit(1000) != ~0ul || radiation.tend_name != "rad") return 6;

        radiation.exec(thermo, day_of_year);
        TF* lflx = dev<TF>(n3); TF* sflx = dev<TF>(n3);
        radiation.get_radiation_field(lflx, "lflx", thermo, day_of_year);
        radiation.get_radiation_field(sflx, "sflx", thermo, day_of_year);
        bool refused = false;
        try { radiation.get_radiation_field(sflx, "rflx", thermo, day_of_year); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        HIPCHK(hipDeviceSynchronize());
        int nonconv = 0; HIPCHK(hipMemcpy(&nonconv, thermo.nonconv_g, sizeof(int), hipMemcpyDeviceToHost));
        if (nonconv) return 8;
        Writer wr(argv[2]);
        wr(fields.st["thl"]->fld_g, n3); wr(lflx, n3); wr(sflx, n3);
        wr.host({(double)radiation.calc_zenith(day_of_year)});
        wr.close();
        std::printf("host_radiation ok\n");
        return 0;
    });
}
