// tests/cpp/host_surface.cpp -- Boundary_surface through the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_surface.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit
// for bit, with the same calls made through the Python binding.
//   host_surface IN OUT itot jtot ktot zsl ubot vbot sbot z0 thref threfh
// IN: u v th [ncells each]. Two calls of exec (the fused call), then -- from the same start -- two calls of exec_slab with the local
// wrap as the 2-D exchange (one rank through the slab sequence); both must agree here, and OUT holds the first:
// dutot ustar obuk ufluxbot vfluxbot ugradbot vgradbot thbot thgradbot dudz dvdz dbdz [ijcells doubles each], then nobuk as doubles.
// gc = (3, 3, 1), second order, double, mbcbot = noslip, th with sbcbot = flux (Thermo_dry).
#include "host_prog.h"
#include <cstring>

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 13, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 2.*std::atof(argv[6])*std::atoi(argv[5]));
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        gd.z.assign(nk, 0); for (int k=0; k<gd.kcells; ++k) gd.z[k] = (2.*(k - gd.kstart) + 1.)*std::atof(argv[6]);      // z[kstart] = zsl
        gd.z_g = up(gd.z);
        Reader rd(argv[1]);
        Fields<TF> fields;
        auto mk = [&](bool read) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = read ? up(rd(n3)) : nullptr;
                                   f->fld_bot_g = dev<TF>(n2); f->grad_bot_g = dev<TF>(n2); f->flux_bot_g = dev<TF>(n2); return f; };
        fields.mp["u"] = mk(true); fields.mp["v"] = mk(true); fields.sp["th"] = mk(true);
        fields.mp["w"] = mk(false); fields.mt["u"] = mk(false); fields.mt["v"] = mk(false); fields.mt["w"] = mk(false); fields.st["th"] = mk(false);
        rd.close();

        Thermo<TF> thermo; thermo.swthermo = "dry";
        auto upload = [](void* d, const void* s, size_t n) { HIPCHK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); };
        auto make = [&](Boundary_surface<TF>& b)
        {
            b.ubot = std::atof(argv[7]); b.vbot = std::atof(argv[8]); b.sbcbot["th"] = MHH_BC_FLUX; b.sbot["th"] = std::atof(argv[9]);
            b.z0m_hom = b.z0h_hom = std::atof(argv[10]); b.thref_kstart = std::atof(argv[11]); b.threfh_kstart = std::atof(argv[12]);
            b.obuk_g = dev<TF>(n2); b.ustar_g = dev<TF>(n2); b.z0m_g = dev<TF>(n2); b.z0h_g = dev<TF>(n2); b.dutot_g = dev<TF>(n2);
            b.dudz_g = dev<TF>(n2); b.dvdz_g = dev<TF>(n2); b.dbdz_g = dev<TF>(n2); b.nobuk_g = dev<int>(n2);
            b.zL_sl_g = dev<float>(MHH_SURFACE_NZL); b.f_sl_g = dev<float>(MHH_SURFACE_NZL);
            b.init(); b.init_surface(upload); b.set_values(thermo, upload);
        };
        auto collect = [&](Boundary_surface<TF>& b)
        {
            HIPCHK(hipDeviceSynchronize());
            std::vector<TF> all;
            for (TF* p : {b.dutot_g, b.ustar_g, b.obuk_g, fields.mp["u"]->flux_bot_g, fields.mp["v"]->flux_bot_g, fields.mp["u"]->grad_bot_g,
                          fields.mp["v"]->grad_bot_g, fields.sp["th"]->fld_bot_g, fields.sp["th"]->grad_bot_g, b.dudz_g, b.dvdz_g, b.dbdz_g})
            {
                std::vector<TF> v(n2); HIPCHK(hipMemcpy(v.data(), p, n2*sizeof(TF), hipMemcpyDeviceToHost));
                all.insert(all.end(), v.begin(), v.end());
            }
            std::vector<int> n(n2); HIPCHK(hipMemcpy(n.data(), b.nobuk_g, n2*sizeof(int), hipMemcpyDeviceToHost));
            for (int x : n) all.push_back(x);
            return all;
        };
        Boundary_surface<TF> one(grid, fields); make(one);
        one.exec(thermo); one.exec(thermo);
        const std::vector<TF> a = collect(one);
        Boundary_surface<TF> slab(grid, fields); make(slab);
        mhh_grid g = grid.abi();
        auto halo2d = [&](TF* p) { mhh_check(mhh_boundary_cyclic_2d(&g, p, nullptr)); };
        slab.exec_slab(thermo, halo2d); slab.exec_slab(thermo, halo2d);
        const std::vector<TF> c = collect(slab);
        if (a.size() != c.size() || std::memcmp(a.data(), c.data(), a.size()*sizeof(TF)) != 0) { std::fprintf(stderr, "exec_slab differs from exec\n"); return 6; }
        bool refused = false;
        try { Boundary_surface<TF> bad(grid, fields); bad.sw_charnock = true; bad.init(); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) return 7;
        Writer wr(argv[2]);
        wr.host(a);
        wr.close();
        std::printf("host_surface ok\n");
        return 0;
    });
}
