// tests/cpp/ib_host_setup.cpp -- TEST infrastructure: a stand-alone program over the three host set-up functions of
// csrc/immersed_boundary.h (mhh_ib_ghost_cells_host, mhh_ib_k_dem_host, mhh_ib_interp_dem_host) on the 16 x 8 x 16 sine terrain, for
// runs of HOST code under a sanitizer. It needs no GPU and no Python: link it with the CPU build of the library's own sources
// (tests/emul), all compiled with the sanitizer, e.g. from tests/emul
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -I. -I../../microhh_amd/csrc \
//       -Wno-attributes -Wno-unused-value -x c++ ../../microhh_amd/csrc/k_*.hip emul_globals.cpp ../cpp/ib_host_setup.cpp -o ib_host_setup
// (k_stencil.hip, which holds the set-up, refers to three launch routines of the marching kernels; with -Wl,--unresolved-symbols=ignore-all
// it links alone, in a tenth of the time). It also walks the refusals, whose early returns are where a set-up would leak or read what it
// was not given.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/mhh_hip.h"

static int fails = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "FAILED: %s (%s)\n", what, mhh_last_error()); ++fails; } }

int main()
{
    const int itot = 16, jtot = 8, ktot = 16, igc = 2, jgc = 2, kgc = 1, n_idw = 5;
    const double xsize = 3200., ysize = 1600., zsize = 1200., pi = 3.14159265358979323846;
    mhh_grid g{};
    g.itot = g.imax = itot; g.jtot = g.jmax = jtot; g.ktot = g.kmax = ktot; g.igc = igc; g.jgc = jgc; g.kgc = kgc;
    g.icells = itot + 2*igc; g.jcells = jtot + 2*jgc; g.kcells = ktot + 2*kgc; g.ijcells = g.icells*g.jcells; g.ncells = (long long)g.ijcells*g.kcells;
    g.istart = igc; g.jstart = jgc; g.kstart = kgc; g.iend = igc + itot; g.jend = jgc + jtot; g.kend = kgc + ktot;
    g.dtype = MHH_F64; g.npx = g.npy = 1; g.xsize = xsize; g.ysize = ysize; g.zsize = zsize; g.dx = xsize/itot; g.dy = ysize/jtot;
    std::vector<double> x(g.icells), xh(g.icells), y(g.jcells), yh(g.jcells), z(g.kcells), zh(g.kcells), dz(g.kcells), dzh(g.kcells);
    for (int i=0; i<g.icells; ++i) { xh[i] = (i-igc)*g.dx; x[i] = xh[i] + 0.5*g.dx; }
    for (int j=0; j<g.jcells; ++j) { yh[j] = (j-jgc)*g.dy; y[j] = yh[j] + 0.5*g.dy; }
    const double d = zsize/ktot;
    for (int k=0; k<g.kcells; ++k) { zh[k] = (k-kgc)*d; z[k] = zh[k] + 0.5*d; dz[k] = d; dzh[k] = d; }
    g.z = z.data(); g.zh = zh.data(); g.dz = dz.data(); g.dzh = dzh.data();
    std::vector<double> dem(g.ijcells);
    for (int j=0; j<g.jcells; ++j)
        for (int i=0; i<g.icells; ++i)          // periodic, so the halos are the cyclic images
            dem[i + j*g.icells] = zsize*(0.25 + 0.15*std::sin(2.*pi*x[i]/xsize)*std::cos(2.*pi*y[j]/ysize));

    struct Loc { const char* name; const double *x, *y, *z, *dz; int bc; };
    const Loc locs[] = {{"u", xh.data(), y.data(), z.data(), dz.data(), MHH_IB_DIRICHLET}, {"v", x.data(), yh.data(), z.data(), dz.data(), MHH_IB_DIRICHLET},
                        {"w", x.data(), y.data(), zh.data(), dzh.data(), MHH_IB_DIRICHLET}, {"s", x.data(), y.data(), z.data(), dz.data(), MHH_IB_FLUX},
                        {"s", x.data(), y.data(), z.data(), dz.data(), MHH_IB_NEUMANN}};
    std::vector<double> xb, yb;
    for (const Loc& l : locs)
    {
        int n = 0;
        expect(mhh_ib_ghost_cells_host(&g, dem.data(), l.x, l.y, l.z, l.dz, n_idw, l.bc, igc, jgc, &n, nullptr) == MHH_OK && n > 0, "count");
        std::vector<int> ii(n), jj(n), kk(n), pi_(n*n_idw), pj(n*n_idw), pk(n*n_idw);
        std::vector<double> r[8], pd(n*n_idw), c(n*n_idw);
        for (auto& v : r) v.assign(n, 0.);
        mhh_ib_ghost_lists out{ii.data(), jj.data(), kk.data(), r[0].data(), r[1].data(), r[2].data(), r[3].data(), r[4].data(), r[5].data(), r[6].data(),
                               pi_.data(), pj.data(), pk.data(), pd.data(), c.data(), r[7].data()};
        expect(mhh_ib_ghost_cells_host(&g, dem.data(), l.x, l.y, l.z, l.dz, n_idw, l.bc, igc, jgc, &n, &out) == MHH_OK, "fill");
        double sum = 0;
        for (double v : c) sum += v;
        std::printf("%s bc %d: %d ghost cells, sum of the weights %.17g\n", l.name, l.bc, n, sum);
        xb = r[0]; yb = r[1];
        int wrong = n - 1;
        expect(mhh_ib_ghost_cells_host(&g, dem.data(), l.x, l.y, l.z, l.dz, n_idw, l.bc, igc, jgc, &wrong, &out) == MHH_EINVAL, "room for another count");
    }
    std::vector<unsigned int> k_dem(g.ijcells, 0u);
    expect(mhh_ib_k_dem_host(&g, dem.data(), z.data(), k_dem.data()) == MHH_OK, "k_dem");
    std::vector<double> at(xb.size());
    expect(mhh_ib_interp_dem_host(&g, dem.data(), x.data(), y.data(), xb.data(), yb.data(), (int)xb.size(), igc, jgc, at.data()) == MHH_OK, "interp");
    // the refusals
    int n = 0;
    const Loc& s = locs[3];
    expect(mhh_ib_ghost_cells_host(&g, dem.data(), s.x, s.y, s.z, s.dz, n_idw, s.bc, igc, -40, &n, nullptr) == MHH_EINVAL && std::strstr(mhh_last_error(), "out of bounds"), "out of bounds");
    expect(mhh_ib_ghost_cells_host(&g, dem.data(), s.x, s.y, s.z, s.dz, 0, s.bc, igc, jgc, &n, nullptr) == MHH_EINVAL, "n_idw < 1");
    expect(mhh_ib_ghost_cells_host(&g, dem.data(), s.x, s.y, s.z, s.dz, n_idw, 9, igc, jgc, &n, nullptr) == MHH_EINVAL, "boundary type");
    {
        int m = 0;
        expect(mhh_ib_ghost_cells_host(&g, dem.data(), s.x, s.y, s.z, s.dz, 73, s.bc, igc, jgc, &m, nullptr) == MHH_OK && m > 0, "count with 73 points");
        std::vector<int> iv(m*73); std::vector<double> rv(m*73);
        mhh_ib_ghost_lists out{iv.data(), iv.data(), iv.data(), rv.data(), rv.data(), rv.data(), rv.data(), rv.data(), rv.data(), rv.data(),
                               iv.data(), iv.data(), iv.data(), rv.data(), rv.data(), rv.data()};
        expect(mhh_ib_ghost_cells_host(&g, dem.data(), s.x, s.y, s.z, s.dz, 73, s.bc, igc, jgc, &m, &out) == MHH_EINVAL && std::strstr(mhh_last_error(), "only found"), "too few neighbours");
    }
    std::vector<double> high(g.ijcells, 0.5*(z[g.kend-4] + z[g.kend-3]));
    expect(mhh_ib_ghost_cells_host(&g, high.data(), s.x, s.y, s.z, s.dz, n_idw, s.bc, igc, jgc, &n, nullptr) == MHH_EINVAL && std::strstr(mhh_last_error(), "too close to the top"), "top");
    double far = -1e4;
    expect(mhh_ib_interp_dem_host(&g, dem.data(), x.data(), y.data(), &far, &far, 1, igc, jgc, at.data()) == MHH_EINVAL, "interp out of bounds");
    std::printf(fails ? "ib_host_setup: %d checks failed\n" : "ib_host_setup ok\n", fails);
    return fails ? 1 : 0;
}
