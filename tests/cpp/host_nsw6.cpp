// tests/cpp/host_nsw6.cpp -- Microphys_nsw6 and Limiter through the C++ host classes of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_nsw6.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit for
// bit, with the same calls made through the Python binding.
//   host_nsw6 IN OUT itot jtot ktot Nc0 dt subdt idt
// IN: thl qt qr qs qg thlt qtt qrt qst qgt [ncells each], then pref exnref rhoref [kcells each], then z zh dz dzh dzi dzhi [kcells each].
// exec(thermo, dt), Limiter::exec(subdt) for qt, qr, qs and qg, get_time_limit(idt, dt). OUT: thlt qtt qrt qst qgt [ncells each],
// rr_bot rs_bot rg_bot [ijcells each], the time limit as a double.
// gc = (3, 3, 1), second order, double, the domain of rcemip (12800 x 12800 x 32250 m).
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
    if (argc != 10) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 6; gd.jcells = gd.jtot + 6; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = 3; gd.kstart = 1; gd.iend = 3 + gd.itot; gd.jend = 3 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = gd.ysize = 12800.; gd.zsize = 32250.; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        const double Nc0 = std::atof(argv[6]), dt = std::atof(argv[7]), subdt = std::atof(argv[8]);
        const unsigned long idt = std::strtoul(argv[9], nullptr, 10);
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        for (const char* n : {"thl", "qt", "qr", "qs", "qg"}) fields.sp[n] = mk();
        for (const char* n : {"thl", "qt", "qr", "qs", "qg"}) fields.st[n] = mk();
        Thermo_moist<TF> thermo(grid, fields);
        thermo.pref_g = up(rd(nk)); thermo.exnref_g = up(rd(nk)); fields.rhoref_g = up(rd(nk));
        thermo.nonconv_g = dev<int>(1);
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        Microphys_nsw6<TF> micro(grid, fields);
        micro.Nc0 = Nc0;
        micro.rr_bot_g = dev<TF>(n2); micro.rs_bot_g = dev<TF>(n2); micro.rg_bot_g = dev<TF>(n2);
        for (TF*& s : micro.scratch_g) s = dev<TF>(n3);
        micro.work_g = dev<char>(mhh_reduce_work_bytes());
        Limiter<TF> limiter(grid, fields);
        limiter.limit_list = {"qt", "qr", "qs", "qg"};
        if (micro.get_switch() != "nsw6" || micro.get_surface_rain_rate() != micro.rr_bot_g || micro.get_surface_graupel_rate() != micro.rg_bot_g) return 6;

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
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        auto wr = [&](const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost));
                                               if (std::fwrite(v.data(), sizeof(TF), n, out) != n) std::exit(4); };
        for (const char* n : {"thl", "qt", "qr", "qs", "qg"}) wr(fields.st[n]->fld_g, n3);
        wr(micro.rr_bot_g, n2); wr(micro.rs_bot_g, n2); wr(micro.rg_bot_g, n2);
        const double lim = (double)limit;
        if (std::fwrite(&lim, sizeof(double), 1, out) != 1) return 4;
        std::fclose(out);
        std::printf("host_nsw6 ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
