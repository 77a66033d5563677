// tests/cpp/pres4_slab.cpp -- Pres_4::exec through the C++ host classes twice on the same fields: the single-GPU Pres(grid, fields, 4)
// of microhh_amd/host/mhh_host.h and the slab driver Pres_slab(master, grid, fields, 4) of microhh_amd/host/mhh_host_rccl.h on a
// one-rank RCCL communicator (the halos of vt and p and both transposes go through ncclSend / ncclRecv to self). Input and output
// are raw binary files written / read by tests/test_slab4_gpu_ranks.py, which compares the two.
#include "host_prog.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "../../microhh_amd/host/mhh_host.h"
#include "../../microhh_amd/host/mhh_host_rccl.h"

using namespace mhh_host;
typedef double TF;

static std::vector<TF> rd(FILE* f, size_t n) { std::vector<TF> v(n); if (std::fread(v.data(), sizeof(TF), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(3); } return v; }
static void dn(FILE* f, const TF* d, size_t n) { std::vector<TF> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(TF), hipMemcpyDeviceToHost)); std::fwrite(v.data(), sizeof(TF), n, f); }

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: pres4_slab in.bin out.bin\n"); return 1; }
    FILE* in = std::fopen(argv[1], "rb"); if (!in) return 1;
    int hdr[7]; if (std::fread(hdr, sizeof(int), 7, in) != 7) return 1;
    double par[4]; if (std::fread(par, sizeof(double), 4, in) != 4) return 1;
    try
    {
        Grid<TF> grid; auto& gd = grid.gd;
        gd.itot = hdr[0]; gd.jtot = hdr[1]; gd.ktot = hdr[2]; gd.igc = hdr[3]; gd.jgc = hdr[4]; gd.kgc = hdr[5];
        const int nchunks = hdr[6];
        gd.imax = gd.itot; gd.jmax = gd.jtot; gd.kmax = gd.ktot;
        gd.icells = gd.itot + 2*gd.igc; gd.jcells = gd.jtot + 2*gd.jgc; gd.kcells = gd.ktot + 2*gd.kgc; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
        gd.istart = gd.igc; gd.jstart = gd.jgc; gd.kstart = gd.kgc; gd.iend = gd.istart + gd.itot; gd.jend = gd.jstart + gd.jtot; gd.kend = gd.kstart + gd.ktot;
        gd.xsize = par[0]; gd.ysize = par[1]; gd.zsize = par[2]; gd.dx = gd.xsize/gd.itot; gd.dy = gd.ysize/gd.jtot;
        const double dt = par[3];
        const size_t nk = gd.kcells, n3 = gd.ncells;
        gd.z = rd(in, nk); gd.zh = rd(in, nk); gd.dz = rd(in, nk); gd.dzh = rd(in, nk); gd.dzi = rd(in, nk); gd.dzhi = rd(in, nk); gd.dzi4 = rd(in, nk); gd.dzhi4 = rd(in, nk);
        gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi); gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);
        const std::vector<TF> rho = rd(in, nk), rhoh = rd(in, nk);
        std::vector<std::vector<TF>> host;
        for (int n = 0; n < 6; ++n) host.push_back(rd(in, n3));                 // u, v, w, ut, vt, wt
        std::fclose(in);

        // the same fields twice: one set for each driver
        auto make = [&](Fields<TF>& f)
        {
            f.rhoref = rho; f.rhorefh = rhoh; f.rhoref_g = up(rho); f.rhorefh_g = up(rhoh);
            const char* nm[3] = {"u", "v", "w"};
            for (int n = 0; n < 3; ++n)
            {
                f.mp[nm[n]] = std::make_shared<Field3d<TF>>(); f.mp[nm[n]]->fld_g = up(host[n]);
                f.mt[nm[n]] = std::make_shared<Field3d<TF>>(); f.mt[nm[n]]->fld_g = up(host[3 + n]);
            }
            f.sd["p"] = std::make_shared<Field3d<TF>>(); f.sd["p"]->fld_g = up(std::vector<TF>(n3, 0.));
        };
        Fields<TF> f1, f2;
        make(f1); make(f2);
        void* work; HIPCHK(hipMalloc(&work, mhh_reduce_work_bytes()));
        Stats stats;

        Pres<TF> pres(grid, f1, 4);
        pres.set_reduce_workspace(work);
        pres.prepare_device();
        pres.exec(dt, stats);
        const double div1 = pres.check_divergence();
        HIPCHK(hipDeviceSynchronize());

        Master_rccl master;
        master.init(1, 0, Master_rccl::unique_id(), nullptr);
        Pres_slab<TF> pres_slab(master, grid, f2, 4);
        pres_slab.set_reduce_workspace(work);
        pres_slab.prepare_device();
        if (nchunks > 1) { pres_slab.set_chunks(nchunks); if (pres_slab.chunks() != nchunks) { std::fprintf(stderr, "set_chunks\n"); return 7; } }
        pres_slab.exec(dt, stats);
        const double div2 = pres_slab.check_divergence();
        HIPCHK(hipDeviceSynchronize());
        pres_slab.clear_device();
        pres.clear_device();

        FILE* out = std::fopen(argv[2], "wb");
        double sc[2] = {div1, div2}; std::fwrite(sc, sizeof(double), 2, out);
        for (Fields<TF>* f : {&f1, &f2})
        {
            dn(out, f->sd["p"]->fld_g, n3);
            dn(out, f->mt["u"]->fld_g, n3); dn(out, f->mt["v"]->fld_g, n3); dn(out, f->mt["w"]->fld_g, n3);
        }
        std::fclose(out);
        // an order the slab driver does not have throws
        bool threw = false;
        try { Pres_slab<TF> bad(master, grid, f2, 3); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::fprintf(stderr, "Pres_slab(order 3) did not throw\n"); return 4; }
        std::printf("pres4_slab ok div=%.17g %.17g\n", div1, div2);
    }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
    return 0;
}
