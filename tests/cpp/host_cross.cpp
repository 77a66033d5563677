// tests/cpp/host_cross.cpp -- Cross_sampler, the C++ host class of Cross in microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_cross.py, which hands the inputs over in a file of doubles and compares the files this program writes, byte
// for byte, with the ones the Python driver (microhh_amd.cross.Cross) writes from the same fields.
//   host_cross IN OUTDIR itot jtot ktot iotime utrans threshold
// IN: u w th [ncells each], thfluxbot [ijcells], rhoref [kcells], then z zh dz dzh dzi dzhi [kcells each].
// Sections xy = 0, 610, 1200; xz = 0, 1700, 3200; yz = 1650, 3200 of u (offset utrans, at the u location), w (at the w location), th,
// thlngrad (second order), and the planes thpath, thfluxbot, thbase and thtop (th above the threshold).
// gc = (3, 3, 1), second order, double, the domain of drycblles.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "../../microhh_amd/host/mhh_host.h"

using namespace mhh_host;
typedef double TF;
#define HIPCHK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); std::exit(2); } } while (0)
static TF* up(const std::vector<TF>& v) { TF* d; HIPCHK(hipMalloc(&d, v.size()*sizeof(TF))); HIPCHK(hipMemcpy(d, v.data(), v.size()*sizeof(TF), hipMemcpyHostToDevice)); return d; }

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
        const int iotime = std::atoi(argv[6]);
        const TF utrans = std::atof(argv[7]), threshold = std::atof(argv[8]);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        Fields<TF> fields;
        TF* u = up(rd(n3)); TF* w = up(rd(n3)); TF* th = up(rd(n3));
        TF* fluxbot = up(rd(n2));
        fields.rhoref_g = up(rd(nk));
        for (std::vector<TF>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        std::fclose(in);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
        gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        Cross_sampler<TF> cross(grid, fields, argv[2]);
        cross.xy = {0., 610., 1200.}; cross.xz = {0., 1700., 3200.}; cross.yz = {1650., 3200.};
        cross.create();
        bool refused = false;
        {
            Cross_sampler<TF> bad(grid, fields, argv[2]);
            bad.xz = {3300.};
            try { bad.create(); } catch (const std::runtime_error& e) { refused = std::string(e.what()).find("in [cross][xz] is outside domain") != std::string::npos; }
        }
        if (!refused) return 7;
        HIPCHK(hipMalloc(&cross.staging_g, cross.staging_elems()*sizeof(TF)));
        cross.to_host = [](void* dst, const void* src, size_t bytes) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); };

        int nerror = 0;
        nerror += cross.cross_simple(u, utrans, "u", iotime, {1, 0, 0});
        nerror += cross.cross_simple(w, TF(0.), "w", iotime, {0, 0, 1});
        nerror += cross.cross_simple(th, TF(0.), "th", iotime, {0, 0, 0});
        nerror += cross.cross_lngrad(th, "thlngrad", iotime, 2);
        nerror += cross.cross_path(th, "thpath", iotime);
        nerror += cross.cross_plane(fluxbot, TF(0.), "thfluxbot", iotime);
        nerror += cross.cross_height_threshold(th, threshold, Cross_direction::Bottom_to_top, "thbase", iotime);
        nerror += cross.cross_height_threshold(th, threshold, Cross_direction::Top_to_bottom, "thtop", iotime);
        if (nerror) { std::fprintf(stderr, "%d files failed\n", nerror); return 6; }
        // "wbx": the same files again are refused, every one of them
        if (cross.cross_simple(th, TF(0.), "th", iotime, {0, 0, 0}) != 8 || cross.cross_path(th, "thpath", iotime) != 1) return 8;
        std::printf("host_cross ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
