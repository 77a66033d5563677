// tests/cpp/host_force.cpp -- Buffer::exec and Force::exec through the C++ host classes of microhh_amd/host/mhh_host.h. Built and run
// by tests/test_cpp_host_force.py, which hands the inputs over in a file of doubles and compares the tendencies this program
// writes back, bit for bit, with the same calls made through the Python binding.
//   host_force IN OUT itot jtot ktot xsize ysize zsize zstart sigma beta fc utrans vtrans
// IN: z zh dz dzh dzi dzhi [kcells each]; u v w s0 s1 ut vt wt st0 st1 [ncells each]; abuf u v w s0 s1, ug, vg, ls_u, ls_s1 [kcells each]
// OUT: ut vt wt st0 st1 after buffer.exec(stats); force.exec(dt, thermo, stats). gc = (1, 1, 1), second order, double.
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 15, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 1, 1, 1, std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]));
        const TF zstart = std::atof(argv[9]), sigma = std::atof(argv[10]), beta = std::atof(argv[11]);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        Reader rd(argv[1]);
        read_metrics(grid, rd);
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
        rd.close();

        buffer.exec(stats);
        force.exec(0.37, thermo, stats);
        HIPCHK(hipDeviceSynchronize());
        Writer wr(argv[2]);
        for (TF* p : {fields.mt["u"]->fld_g, fields.mt["v"]->fld_g, fields.mt["w"]->fld_g, fields.st["s0"]->fld_g, fields.st["s1"]->fld_g}) wr(p, n3);
        wr.close();
        std::printf("host_force ok: bufferkstart %d bufferkstarth %d\n", buffer.get_bufferkstart(), buffer.get_bufferkstarth());
        return 0;
    });
}
