// tests/cpp/host_force.cpp -- Buffer::exec and Force::exec through the C++ host classes of microhh_amd/host/mhh_host.h. Built and run
// by tests/test_cpp_host_force.py, which hands the inputs over in a file of doubles and compares the tendencies this program
// writes back, bit for bit, with the same calls made through the Python binding.
//   host_force IN OUT itot jtot ktot xsize ysize zsize zstart sigma beta fc utrans vtrans
// IN: z zh dz dzh dzi dzhi [kcells each]; u v w s0 s1 ut vt wt st0 st1 [ncells each]; abuf u v w s0 s1, ug, vg, ls_u, ls_s1 [kcells each]
// OUT: ut vt wt st0 st1 after buffer.exec(stats); force.exec(dt, thermo, stats). gc = (1, 1, 1), second order, double.
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
    if (argc != 15) { std::fprintf(stderr, "usage\n"); return 3; }
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = std::atoi(argv[3]); gd.jtot = std::atoi(argv[4]); gd.ktot = std::atoi(argv[5]); gd.igc = gd.jgc = gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 2; gd.jcells = gd.jtot + 2; gd.kcells = gd.ktot + 2; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.jstart = gd.kstart = 1; gd.iend = 1 + gd.itot; gd.jend = 1 + gd.jtot; gd.kend = 1 + gd.ktot;
        gd.xsize = std::atof(argv[6]); gd.ysize = std::atof(argv[7]); gd.zsize = std::atof(argv[8]); gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const TF zstart = std::atof(argv[9]), sigma = std::atof(argv[10]), beta = std::atof(argv[11]);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        FILE* in = std::fopen(argv[1], "rb");
        if (!in) return 4;
        auto rd = [&](size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, in) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } return v; };
        gd.z = rd(nk); gd.zh = rd(nk); gd.dz = rd(nk); gd.dzh = rd(nk); gd.dzi = rd(nk); gd.dzhi = rd(nk); gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi); gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); return f; };
        fields.mp["u"] = mk(); fields.mp["v"] = mk(); fields.mp["w"] = mk(); fields.sp["s0"] = mk(); fields.sp["s1"] = mk();
        fields.mt["u"] = mk(); fields.mt["v"] = mk(); fields.mt["w"] = mk(); fields.st["s0"] = mk(); fields.st["s1"] = mk();

        Stats stats; Thermo<TF> thermo;
        Buffer<TF> buffer(grid, fields, true, false, zstart, sigma, beta);
        buffer.init(); buffer.create(stats);
        for (const char* nm : {"u", "v", "w", "s0", "s1"}) buffer.bufferprofs_g[nm] = up(rd(nk));
        TF* sg; HIPCHK(hipMalloc((void**)&sg, 2*nk*sizeof(TF)));
        buffer.prepare_device(sg, [](void* d, const void* s, size_t n) { HIPCHK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); });

        Force<TF> force(grid, fields);
        force.swlspres = Large_scale_pressure_type::Geo_wind; force.fc = std::atof(argv[12]); force.utrans = std::atof(argv[13]); force.vtrans = std::atof(argv[14]);
        force.ug_g = up(rd(nk)); force.vg_g = up(rd(nk));
        force.swls = true; force.lslist = {"u", "s1"};
        force.lsprofs_g["u"] = up(rd(nk)); force.lsprofs_g["s1"] = up(rd(nk));
        std::fclose(in);

        buffer.exec(stats);
        force.exec(0.37, thermo, stats);
        HIPCHK(hipDeviceSynchronize());
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 4;
        for (TF* p : {fields.mt["u"]->fld_g, fields.mt["v"]->fld_g, fields.mt["w"]->fld_g, fields.st["s0"]->fld_g, fields.st["s1"]->fld_g})
        {
            std::vector<TF> v(n3); HIPCHK(hipMemcpy(v.data(), p, n3*sizeof(TF), hipMemcpyDeviceToHost));
            if (std::fwrite(v.data(), sizeof(TF), n3, out) != n3) return 4;
        }
        std::fclose(out);
        std::printf("host_force ok: bufferkstart %d bufferkstarth %d\n", buffer.get_bufferkstart(), buffer.get_bufferkstarth());
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
