// tests/cpp/host_moist.cpp -- Thermo_moist through the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_moist.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit for
// bit, with the same calls made through the Python binding.
//   host_moist IN OUT itot jtot ktot pbot
// IN: thl qt wt [ncells each], then thl0 qt0 [ktot each]. create_basestate, the means of thl and qt, exec (base state on the device
// and the buoyancy tendency), get_thermo_field("ql"). OUT: wt ql [ncells each], then the eight tables [kcells each].
// gc = (3, 3, 1), second order, double, a uniform grid of 6400 x 6400 x 3000 m.
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
    if (argc != 7) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 6; gd.jcells = gd.jtot + 6; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = 3; gd.kstart = 1; gd.iend = 3 + gd.itot; gd.jend = 3 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = gd.ysize = 6400.; gd.zsize = 3000.; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const size_t nk = gd.kcells, n3 = gd.ncells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); f->fld_mean_g = dev<TF>(nk); return f; };
        fields.sp["thl"] = mk(); fields.sp["qt"] = mk(); fields.mt["w"] = mk();
        const std::vector<TF> thl0 = rd(gd.ktot), qt0 = rd(gd.ktot);
        // the metrics of Grid::calculate (src/grid.cxx:237-368) at second order, from the file so that both sides hold the same bits
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        Thermo_moist<TF> thermo(grid, fields);
        thermo.pbot = std::atof(argv[6]);
        TF** tabs[8] = {&thermo.pref_g, &thermo.prefh_g, &thermo.rhoref_g, &thermo.rhorefh_g, &thermo.thvref_g, &thermo.thvrefh_g, &thermo.exnref_g, &thermo.exnrefh_g};
        for (TF** t : tabs) *t = dev<TF>(nk);
        thermo.nonconv_g = dev<int>(1);
        auto upload = [](void* d, const void* s, size_t n) { HIPCHK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); };
        thermo.create_basestate(thl0, qt0, upload);
        if (fields.rhoref.size() != nk || fields.rhoref[gd.kstart] != thermo.rhoref[gd.kstart]) return 6;

        // fields->exec: the means of thl and qt
        mhh_grid g = grid.abi();
        const void* flds[2] = {fields.sp["thl"]->fld_g, fields.sp["qt"]->fld_g};
        void* profs[2] = {fields.sp["thl"]->fld_mean_g, fields.sp["qt"]->fld_mean_g};
        double* scratch = dev<double>(mhh_field_mean_scratch_elems(&g, 2));
        mhh_check(mhh_field_mean_profile(&g, flds, 2, profs, scratch, nullptr));
        thermo.exec();
        TF* ql = dev<TF>(n3);
        thermo.get_thermo_field(ql, "ql");
        bool refused = false;
        try { thermo.get_thermo_field(ql, "thv"); } catch (const std::runtime_error&) { refused = true; }
        if (!refused || thermo.get_basestate_vector("thvrefh") != thermo.thvrefh_g) return 7;
        HIPCHK(hipDeviceSynchronize());
        int nonconv = 0; HIPCHK(hipMemcpy(&nonconv, thermo.nonconv_g, sizeof(int), hipMemcpyDeviceToHost));
        if (nonconv) return 8;
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        auto wr = [&](const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost));
                                               if (std::fwrite(v.data(), sizeof(TF), n, out) != n) std::exit(4); };
        wr(fields.mt["w"]->fld_g, n3); wr(ql, n3);
        for (TF** t : tabs) wr(*t, nk);
        std::fclose(out);
        std::printf("host_moist ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
