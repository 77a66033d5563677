// tests/cpp/host_ib.cpp -- Immersed_boundary, the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_ib.py, which hands the inputs over in a file of doubles and compares what this program writes, byte for byte,
// with what the Python driver (microhh_amd.ib.Dem behind a HotPath) leaves from the same fields.
//   host_ib IN OUT itot jtot ktot n_idw sbcbot sbot visc
// IN: u v w th [ncells each], dem [ijcells, halos filled], then z zh dz dzh dzi dzhi [kcells each].
// OUT: u v w th after exec_scalars and exec_momentum [ncells each], mask maskh [ncells each], thfluxbot_ib [ijcells], then the
// ghost-cell counts of u, v, w, s.
// gc = (3, 3, 1), second order, double, the domain of drycblles.
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 10, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 1200.);
        const int n_idw = std::atoi(argv[6]), sbcbot = std::atoi(argv[7]);
        const TF sbot = std::atof(argv[8]), visc = std::atof(argv[9]);
        const size_t n3 = gd.ncells, n2 = gd.ijcells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        fields.visc = visc;
        for (const char* n : {"u", "v", "w"}) { fields.mp[n] = std::make_shared<Field3d<TF>>(); fields.mp[n]->fld_g = up(rd(n3)); }
        fields.sp["th"] = std::make_shared<Field3d<TF>>(); fields.sp["th"]->fld_g = up(rd(n3)); fields.sp["th"]->visc = visc;
        std::vector<TF> dem = rd(n2);
        read_metrics(grid, rd);
        rd.close();

        Immersed_boundary<TF> ib(grid, fields);
        ib.sbcbot = sbcbot; ib.sbc["th"] = sbot; ib.dem = dem;
        ib.alloc = [](size_t bytes) { void* d; HIPCHK(hipMalloc(&d, bytes)); return d; };
        ib.upload = [](void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); };
        ib.release = [](void* d) { HIPCHK(hipFree(d)); };
        bool refused = false;
        ib.n_idw_points = 0;
        try { ib.create(); } catch (const std::runtime_error& e) { refused = std::string(e.what()).find("n_idw_points must be at least 1") != std::string::npos; }
        if (!refused) return 7;
        ib.n_idw_points = n_idw;
        ib.create();
        ib.prepare_device();
        ib.exec_scalars();
        ib.exec_momentum();
        TF* mask = dev<TF>(n3); TF* maskh = dev<TF>(n3); TF* flux = dev<TF>(n2);
        ib.get_mask(mask, maskh);
        mhh_grid g = grid.abi();
        mhh_check(mhh_ib_fluxbot(&g, flux, ib.k_dem_g, fields.sp.at("th")->fld_g, visc, nullptr));
        mhh_check(mhh_synchronize(nullptr));

        Writer wr(argv[2]);
        for (const char* n : {"u", "v", "w"}) wr(fields.mp.at(n)->fld_g, n3);
        wr(fields.sp.at("th")->fld_g, n3);
        wr(mask, n3); wr(maskh, n3); wr(flux, n2);
        wr.host({double(ib.ghost.at("u").nghost), double(ib.ghost.at("v").nghost), double(ib.ghost.at("w").nghost), double(ib.ghost.at("s").nghost)});
        wr.close();
        ib.clear_device();
        if (ib.k_dem_g || ib.ghost.at("u").cell_g) return 8;
        std::printf("host_ib ok\n");
        return 0;
    });
}
