// tests/cpp/host_cross.cpp -- Cross_sampler, the C++ host class of Cross in microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_cross.py, which hands the inputs over in a file of doubles and compares the files this program writes, byte
// for byte, with the ones the Python driver (microhh_amd.cross.Cross) writes from the same fields.
//   host_cross IN OUTDIR itot jtot ktot iotime utrans threshold
// IN: u w th [ncells each], thfluxbot [ijcells], rhoref [kcells], then z zh dz dzh dzi dzhi [kcells each].
// Sections xy = 0, 610, 1200; xz = 0, 1700, 3200; yz = 1650, 3200 of u (offset utrans, at the u location), w (at the w location), th,
// thlngrad (second order), and the planes thpath, thfluxbot, thbase and thtop (th above the threshold).
// gc = (3, 3, 1), second order, double, the domain of drycblles.
#include "host_prog.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 9, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 1200.);
        const int iotime = std::atoi(argv[6]);
        const TF utrans = std::atof(argv[7]), threshold = std::atof(argv[8]);
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        TF* u = up(rd(n3)); TF* w = up(rd(n3)); TF* th = up(rd(n3));
        TF* fluxbot = up(rd(n2));
        fields.rhoref_g = up(rd(nk));
        read_metrics(grid, rd);
        rd.close();

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
        return 0;
    });
}
