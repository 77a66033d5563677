// tests/cpp/buoy_step.cpp -- Thermo_buoy (swthermo = "buoy") through the C++ host classes of microhh_amd/host/mhh_host.h, driven
// the way Model<TF>::exec drives the reference operators (src/model.cxx:346-392). Built and run by tests/test_cpp_host_buoy.py.
// Synthetic fields on a (32, 24, 16) grid with a surface model, b the only scalar. Checks, each on fresh copies of the same state:
//   1. thermo.exec(); advec.exec(); diff.exec()  ==  diff.exec_with_advec(advec, stats, stream, &thermo), bit for bit, for the flat
//      form (folded into the fused pass) and the sloped form (its own launch inside the fused call);
//   2. exec_viscosity with N2 of b inline  ==  with thermo.N2_g from get_thermo_field_N2, bit for bit;
//   3. the overlapped slab sub-step Substep_slab::halo_visc_rhs (mhh_host_rccl.h) on a one-rank RCCL communicator against the
//      single-GPU sub-step, within 1e-10 of the largest value.
// Exit status 0 and "buoy_step ok" on success.
#include "host_prog.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include "../../microhh_amd/host/mhh_host.h"
#include "../../microhh_amd/host/mhh_host_rccl.h"

using namespace mhh_host;
typedef double TF;

static std::vector<TF> dn(const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost)); return v; }

struct Lcg
{
    unsigned long long s;
    TF operator()(TF lo, TF hi) { s = s*6364136223846793005ull + 1442695040888963407ull; return lo + (hi - lo)*TF((s >> 11) * (1.0/9007199254740992.0)); }
};

int main()
{
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = 32; gd.jtot = 24; gd.ktot = 16; gd.igc = 3; gd.jgc = 3; gd.kgc = 1;
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 2*gd.igc; gd.jcells = gd.jtot + 2*gd.jgc; gd.kcells = gd.ktot + 2*gd.kgc; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.igc; gd.jstart = gd.jgc; gd.kstart = gd.kgc; gd.iend = gd.istart + gd.itot; gd.jend = gd.jstart + gd.jtot; gd.kend = gd.kstart + gd.ktot;
        gd.xsize = 27.386127875258303; gd.ysize = 27.386127875258303; gd.zsize = 18.074844397670482; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const size_t nk = gd.kcells, n3 = gd.ncells, n2 = gd.ijcells;
        // uniform vertical grid (Grid::calculate, src/grid.cxx:237-368, second order)
        const TF dz = gd.zsize/gd.ktot;
        gd.z.assign(nk, 0); gd.zh.assign(nk, 0); gd.dz.assign(nk, dz); gd.dzh.assign(nk, dz); gd.dzi.assign(nk, 1./dz); gd.dzhi.assign(nk, 1./dz);
        gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
        for (size_t k=0; k<nk; ++k) { gd.z[k] = (TF(k) - gd.kstart + 0.5)*dz; gd.zh[k] = (TF(k) - gd.kstart)*dz; }
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi); gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);

        // the initial state on the host; every check starts from a fresh device copy of it
        Lcg r{666};
        std::map<std::string, std::vector<TF>> h;
        for (const char* nm : {"u", "v"}) { h[nm].resize(n3); for (auto& x : h[nm]) x = r(-1, 1); }
        h["w"].resize(n3); for (auto& x : h["w"]) x = r(-.5, .5);
        h["b"].resize(n3);
        for (size_t k=0; k<nk; ++k) for (size_t ij=0; ij<n2; ++ij) h["b"][ij + k*n2] = 0.003*gd.z[k] + r(-0.01, 0.01);
        for (size_t ij=0; ij<n2; ++ij) { h["w"][ij + gd.kstart*n2] = 0; h["w"][ij + gd.kend*n2] = 0; }
        for (const char* nm : {"ut", "vt", "wt", "bt"}) { h[nm].resize(n3); for (auto& x : h[nm]) x = r(0, 1e-3); }
        for (const char* nm : {"ufb", "uft", "vfb", "vft", "bfb", "bft", "dudz", "dvdz"}) { h[nm].resize(n2); for (auto& x : h[nm]) x = r(0, 1e-2); }
        h["dbdz"].resize(n2); for (auto& x : h["dbdz"]) x = r(0, 1e-4);
        h["z0m"].assign(n2, 0.1);

        Fields<TF> fields;
        fields.visc = 1.5e-5;
        fields.rhoref.assign(nk, 1.); fields.rhorefh.assign(nk, 1.);
        fields.rhoref_g = up(fields.rhoref); fields.rhorefh_g = up(fields.rhorefh);
        auto mk = [&](const std::vector<TF>& v) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(v); return f; };
        fields.mp["u"] = mk(h["u"]); fields.mp["v"] = mk(h["v"]); fields.mp["w"] = mk(h["w"]); fields.sp["b"] = mk(h["b"]); fields.sp["b"]->visc = 1.5e-5;
        fields.mt["u"] = mk(h["ut"]); fields.mt["v"] = mk(h["vt"]); fields.mt["w"] = mk(h["wt"]); fields.st["b"] = mk(h["bt"]);
        fields.mp["u"]->flux_bot_g = up(h["ufb"]); fields.mp["u"]->flux_top_g = up(h["uft"]);
        fields.mp["v"]->flux_bot_g = up(h["vfb"]); fields.mp["v"]->flux_top_g = up(h["vft"]);
        fields.sp["b"]->flux_bot_g = up(h["bfb"]); fields.sp["b"]->flux_top_g = up(h["bft"]);
        for (const char* nm : {"evisc", "p"}) { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(std::vector<TF>(n3, 0.)); fields.sd[nm] = f; }
        Boundary<TF> boundary; boundary.swboundary = "surface";
        boundary.dudz_g = up(h["dudz"]); boundary.dvdz_g = up(h["dvdz"]); boundary.dbdz_g = up(h["dbdz"]); boundary.z0m_g = up(h["z0m"]);

        // reset the prognostic fields, the tendencies and evisc to the initial state
        auto reset = [&]()
        {
            const std::pair<std::shared_ptr<Field3d<TF>>, const char*> all[] = {{fields.mp["u"], "u"}, {fields.mp["v"], "v"}, {fields.mp["w"], "w"}, {fields.sp["b"], "b"},
                                                                               {fields.mt["u"], "ut"}, {fields.mt["v"], "vt"}, {fields.mt["w"], "wt"}, {fields.st["b"], "bt"}};
            for (auto& a : all) HIPCHK(hipMemcpy(a.first->fld_g, h[a.second].data(), n3*sizeof(TF), hipMemcpyHostToDevice));
            HIPCHK(hipMemset(fields.sd["evisc"]->fld_g, 0, n3*sizeof(TF)));
        };
        auto result = [&]()
        {
            HIPCHK(hipDeviceSynchronize());
            std::vector<std::vector<TF>> out;
            for (TF* p : {fields.mt["u"]->fld_g, fields.mt["v"]->fld_g, fields.mt["w"]->fld_g, fields.st["b"]->fld_g, fields.sd["evisc"]->fld_g}) out.push_back(dn(p, n3));
            return out;
        };
        const char* names[] = {"ut", "vt", "wt", "bt", "evisc"};
        auto bits_equal = [&](const std::vector<std::vector<TF>>& a, const std::vector<std::vector<TF>>& b, const char* what)
        {
            for (size_t m=0; m<a.size(); ++m)
                if (std::memcmp(a[m].data(), b[m].data(), n3*sizeof(TF)))
                { std::fprintf(stderr, "%s: %s differs\n", what, names[m]); std::exit(10); }
        };

        void* work; HIPCHK(hipMalloc(&work, mhh_reduce_work_bytes()));
        TF* mlen0; HIPCHK(hipMalloc((void**)&mlen0, nk*sizeof(TF)));
        Stats stats;
        Boundary_cyclic<TF> boundary_cyclic(grid);
        auto advec = Advec<TF>::factory(grid, fields, "2i5");
        auto diff = Diff<TF>::factory(grid, fields, boundary, "smag2", 0.4, 0.23, 10.);
        advec->set_reduce_workspace(work); diff->set_reduce_workspace(work);
        diff->prepare_device(boundary, mlen0, [](void* d, const void* s, size_t n) { HIPCHK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); });
        Thermo<TF> thermo; thermo.swthermo = "buoy"; thermo.b = "b"; thermo.swspatialorder = 2;
        if (diff->params(&thermo).buoyancy_kind != 1) { std::fprintf(stderr, "params: buoyancy_kind\n"); return 7; }

        auto cyclic = [&]() { for (auto& it : fields.mp) boundary_cyclic.exec_g(it.second->fld_g); for (auto& it : fields.sp) boundary_cyclic.exec_g(it.second->fld_g); };
        // ---- 1. thermo, advec, diff as three calls against the fused call with the buoyancy folded in
        const TF forms[2][3] = {{0., 0., 0.}, {0.5235, 1., 0.13}};          // flat; sloped (alpha, N2, utrans)
        std::vector<std::vector<TF>> single;
        for (int fm=0; fm<2; ++fm)
        {
            thermo.alpha = forms[fm][0]; thermo.n2 = forms[fm][1]; thermo.utrans = forms[fm][2];
            reset(); cyclic(); diff->exec_viscosity(thermo);
            thermo.exec(grid, fields); advec->exec(stats); diff->exec(stats);
            const auto three = result();
            reset(); cyclic(); diff->exec_viscosity(thermo);
            diff->exec_with_advec(*advec, stats, nullptr, &thermo);
            const auto fused = result();
            bits_equal(three, fused, fm ? "sloped: three calls vs exec_with_advec" : "flat: three calls vs exec_with_advec");
            if (std::memcmp(three[2].data(), h["wt"].data(), n3*sizeof(TF)) == 0) { std::fprintf(stderr, "wt unchanged\n"); return 8; }
            if (fm == 0) single = three;
        }
        // ---- 2. N2 of b inline against N2 through thermo.N2_g (get_thermo_field("N2"))
        thermo.alpha = 0; thermo.n2 = 0.7; thermo.utrans = 0;
        reset(); cyclic(); diff->exec_viscosity(thermo);
        const auto ev_inline = result();
        TF* N2; HIPCHK(hipMalloc((void**)&N2, n3*sizeof(TF)));
        reset(); cyclic(); thermo.get_thermo_field_N2(grid, fields, N2); thermo.N2_g = N2; diff->exec_viscosity(thermo); thermo.N2_g = nullptr;
        bits_equal(ev_inline, result(), "evisc: N2 inline vs N2 through a pointer");
        HIPCHK(hipFree(N2));
        // ---- 3. the overlapped slab sub-step on one rank against the single-GPU sub-step (flat form, folded in neither: thermo.exec first)
        thermo.n2 = 0;
        {
            Master_rccl master;
            master.init(1, 0, Master_rccl::unique_id(), nullptr);
            Boundary_cyclic_slab<TF> halo(master, grid);
            Substep_slab<TF> sub(master, grid, fields, halo);
            if (!sub.can_overlap(*advec, *diff)) { std::fprintf(stderr, "can_overlap\n"); return 7; }
            reset();
            thermo.exec(grid, fields, master.stream);
            sub.halo_visc_rhs(*advec, *diff, thermo);
            const auto slab = result();
            for (size_t m=0; m<slab.size(); ++m)
            {
                TF dmax = 0, amax = 0;
                for (int k=gd.kstart; k<gd.kend; ++k) for (int j=gd.jstart; j<gd.jend; ++j) for (int i=gd.istart; i<gd.iend; ++i)
                {
                    const size_t c = i + j*gd.icells + k*gd.ijcells;
                    dmax = std::max(dmax, std::abs(slab[m][c] - single[m][c])); amax = std::max(amax, std::abs(single[m][c]));
                }
                if (!(dmax <= 1e-10*amax)) { std::fprintf(stderr, "slab sub-step: %s differs by %g of %g\n", names[m], dmax, amax); return 11; }
            }
        }
        std::printf("buoy_step ok\n");
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
