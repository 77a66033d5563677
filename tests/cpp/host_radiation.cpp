// tests/cpp/host_radiation.cpp -- Radiation_gcss through the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_radiation.py, which hands the inputs over in a file of doubles and compares what this program writes back,
// bit for bit, with the same calls made through the Python binding.
//   host_radiation IN OUT itot jtot ktot xka fr0 fr1 div lat lon day_of_year
// IN: thl qt thlt [ncells each], then pref exnref rhoref [kcells each], then z zh dz dzh dzi dzhi [kcells each].
// exec(thermo, day_of_year), get_radiation_field for lflx and sflx. OUT: thlt lflx sflx [ncells each], mu as a double.
// gc = (3, 3, 1), second order, double, the domain of dycoms (6400 x 6400 x 1500 m).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include "../../microhh_amd/host/mhh_host.h"

using namespace mhh_host;
typedef double TF;
#define HIPCHK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); std::exit(2); } } while (0)
static TF* up(const std::vector<TF>& v) { TF* d; HIPCHK(hipMalloc(&d, v.size()*sizeof(TF))); HIPCHK(hipMemcpy(d, v.data(), v.size()*sizeof(TF), hipMemcpyHostToDevice)); return d; }
template<class T> static T* dev(size_t n) { T* d; HIPCHK(hipMalloc(&d, n*sizeof(T))); HIPCHK(hipMemset(d, 0, n*sizeof(T))); return d; }

int main(int argc, char** argv)
{
    if (argc != 13) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 6; gd.jcells = gd.jtot + 6; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = 3; gd.kstart = 1; gd.iend = 3 + gd.itot; gd.jend = 3 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = gd.ysize = 6400.; gd.zsize = 1500.; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        gd.lat = std::atof(argv[10]); gd.lon = std::atof(argv[11]);
        const double day_of_year = std::atof(argv[12]);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        for (const char* n : {"thl", "qt"}) fields.sp[n] = mk();
        fields.st["thl"] = mk();
        Thermo_moist<TF> thermo(grid, fields);
        thermo.pref_g = up(rd(nk)); thermo.exnref_g = up(rd(nk)); fields.rhoref_g = up(rd(nk));
        thermo.nonconv_g = dev<int>(1);
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

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
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        auto wr = [&](const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost));
                                               if (std::fwrite(v.data(), sizeof(TF), n, out) != n) std::exit(4); };
        wr(fields.st["thl"]->fld_g, n3); wr(lflx, n3); wr(sflx, n3);
        const double mu = radiation.calc_zenith(day_of_year);
        if (std::fwrite(&mu, sizeof(double), 1, out) != 1) return 4;
        std::fclose(out);
        std::printf("host_radiation ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
