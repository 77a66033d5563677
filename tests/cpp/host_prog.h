// tests/cpp/host_prog.h -- TEST infrastructure: what the C++ host programs of this directory share. tests/hostprog.py builds and
// runs them. Exit statuses: 2 a HIP error, 3 usage, 4 input or output, 5 an exception, 6 and above a program's own checks.
#ifndef MHH_TESTS_HOST_PROG_H
#define MHH_TESTS_HOST_PROG_H
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <vector>
#include "../../microhh_amd/host/mhh_host.h"

#define HIPCHK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); std::exit(2); } } while (0)

// a host vector on the device
template<class T> static T* up(const std::vector<T>& v) { T* d; HIPCHK(hipMalloc(&d, v.size()*sizeof(T))); HIPCHK(hipMemcpy(d, v.data(), v.size()*sizeof(T), hipMemcpyHostToDevice)); return d; }
// n zeroed elements on the device
template<class T> static T* dev(size_t n) { T* d; HIPCHK(hipMalloc(&d, n*sizeof(T))); HIPCHK(hipMemset(d, 0, n*sizeof(T))); return d; }

// the input file of doubles: rd(n) gives the next n of them
struct Reader
{
    FILE* f;
    explicit Reader(const char* path) : f(std::fopen(path, "rb")) { if (!f) std::exit(4); }
    std::vector<double> operator()(size_t n)
    {
        std::vector<double> v(n);
        if (std::fread(v.data(), sizeof(double), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); }
        return v;
    }
    void close() { std::fclose(f); }
};

// the output file of doubles: wr(d, n) appends n doubles of device memory, wr.host(v) a host vector
struct Writer
{
    FILE* f;
    explicit Writer(const char* path) : f(std::fopen(path, "wb")) { if (!f) std::exit(4); }
    void host(const std::vector<double>& v) { if (std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(4); }
    void operator()(const double* d, size_t n) { std::vector<double> v(n); HIPCHK(hipMemcpy(v.data(), d, n*sizeof(double), hipMemcpyDeviceToHost)); host(v); }
    void close() { std::fclose(f); }
};

// every member of Grid_data that follows from the sizes and the ghost cells; the metric profiles are read_metrics'
static inline void make_grid(mhh_host::Grid<double>& grid, int itot, int jtot, int ktot, int igc, int jgc, int kgc, double xsize, double ysize, double zsize)
{
    auto& gd = grid.gd;
    gd.itot = itot; gd.jtot = jtot; gd.ktot = ktot; gd.igc = igc; gd.jgc = jgc; gd.kgc = kgc;
    gd.imax = itot; gd.jmax = jtot; gd.kmax = ktot;
    gd.icells = itot + 2*igc; gd.jcells = jtot + 2*jgc; gd.kcells = ktot + 2*kgc; gd.ijcells = gd.icells*gd.jcells; gd.ncells = gd.ijcells*gd.kcells;
    gd.istart = igc; gd.jstart = jgc; gd.kstart = kgc; gd.iend = igc + itot; gd.jend = jgc + jtot; gd.kend = kgc + ktot;
    gd.xsize = xsize; gd.ysize = ysize; gd.zsize = zsize; gd.dx = xsize/itot; gd.dy = ysize/jtot;
}

// z zh dz dzh dzi dzhi [kcells each] from the file, so that both sides hold the same bits (Grid::calculate, src/grid.cxx:237-368, at
// second order), and the fourth-order pair as zeros; all eight on the device
static inline void read_metrics(mhh_host::Grid<double>& grid, Reader& rd)
{
    auto& gd = grid.gd;
    const size_t nk = gd.kcells;
    for (std::vector<double>* v : {&gd.z, &gd.zh, &gd.dz, &gd.dzh, &gd.dzi, &gd.dzhi}) *v = rd(nk);
    gd.dzi4.assign(nk, 0); gd.dzhi4.assign(nk, 0);
    gd.z_g = up(gd.z); gd.zh_g = up(gd.zh); gd.dz_g = up(gd.dz); gd.dzh_g = up(gd.dzh); gd.dzi_g = up(gd.dzi); gd.dzhi_g = up(gd.dzhi);
    gd.dzi4_g = up(gd.dzi4); gd.dzhi4_g = up(gd.dzhi4);
}

// main's frame: body() returns the program's status
template<class Body> static int run_main(int argc, char** argv, int nargs, Body body)
{
    if (argc != nargs) { std::fprintf(stderr, "usage: %s takes %d arguments (its header comment names them)\n", argv[0], nargs - 1); return 3; }
    try { return body(); }
    catch (const std::exception& e) { std::cerr << "EXCEPTION: " << e.what() << std::endl; return 5; }
}

#endif
