// ref_ib_shim.cpp -- TEST infrastructure: the reference's own Immersed_boundary kernels behind a C interface.
//
// Compiled by tests/ib_ref.py into a temporary directory with the reference's src and include directories and
// tests/stubs_syntax_only on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections
// collected at link time); nothing compiled from it is kept. The translation unit is included in place, so that the functions of its
// anonymous namespace (interp2_dem, calc_ghost_cells, set_ghost_cells, calc_mask, find_k_dem, calc_fluxes) are visible here. What is
// written here is the calls only, with the arguments Immersed_boundary::create (:766-918), exec_momentum / exec_scalars (:640-696),
// get_mask (:930-946) and exec_cross (:950-985) pass.
#include "immersed_boundary.cxx"
#include "ref_shim.h"
#include <cstring>

namespace
{
    char message[512];

    template<typename TF> Ghost_cells<TF>& lists() { static Ghost_cells<TF> g; return g; }

    Boundary_type type_of(int bc)
    {
        return bc == 0 ? Boundary_type::Dirichlet_type : bc == 1 ? Boundary_type::Neumann_type : Boundary_type::Flux_type;
    }

    // Ghost_cells<TF> of one location into the static object; its size, or -1 with the text of what was thrown
    template<typename TF>
    int ghost(const Dims& d, const TF* dem, const TF* x, const TF* y, const TF* z, const TF* dz, int bc, double dx, double dy, int n_idw, int offx, int offy)
    {
        const int jcells = d.ijcells / d.icells;
        const std::vector<TF> vdem(dem, dem + d.ijcells), vx(x, x + d.icells), vy(y, y + jcells), vz(z, z + d.kcells), vdz(dz, dz + d.kcells);
        lists<TF>() = Ghost_cells<TF>();
        message[0] = 0;
        try
        {
            calc_ghost_cells<TF>(lists<TF>(), vdem, vx, vy, vz, type_of(bc), TF(dx), TF(dy), vdz, n_idw,
                    d.istart, d.jstart, d.kstart, d.iend, d.jend, d.kend, d.icells, jcells, d.ijcells, offx, offy);
        }
        catch (const std::exception& e) { std::strncpy(message, e.what(), sizeof(message)-1); return -1; }
        catch (...) { std::strncpy(message, "throw 1", sizeof(message)-1); return -1; }
        return lists<TF>().nghost;
    }

    template<typename T> void put(const std::vector<T>& v, T* out) { std::copy(v.begin(), v.end(), out); }

    template<typename TF>
    void get(int** ints, TF** reals)
    {
        const Ghost_cells<TF>& g = lists<TF>();
        put(g.i, ints[0]); put(g.j, ints[1]); put(g.k, ints[2]); put(g.ip_i, ints[3]); put(g.ip_j, ints[4]); put(g.ip_k, ints[5]);
        put(g.xb, reals[0]); put(g.yb, reals[1]); put(g.zb, reals[2]); put(g.xi, reals[3]); put(g.yi, reals[4]); put(g.zi, reals[5]);
        put(g.di, reals[6]); put(g.ip_d, reals[7]); put(g.c_idw, reals[8]); put(g.c_idw_sum, reals[9]);
    }

    template<typename TF>
    int interp(const Dims& d, int n, const TF* xp, const TF* yp, const TF* x, const TF* y, const TF* plane, double dx, double dy, int offx, int offy, TF* out)
    {
        const int jcells = d.ijcells / d.icells;
        const std::vector<TF> vp(plane, plane + d.ijcells), vx(x, x + d.icells), vy(y, y + jcells);
        message[0] = 0;
        try
        {
            for (int m=0; m<n; ++m)
                out[m] = interp2_dem<TF>(xp[m], yp[m], vx, vy, vp, TF(dx), TF(dy), d.icells, jcells, offx, offy);
        }
        catch (const std::exception& e) { std::strncpy(message, e.what(), sizeof(message)-1); return -1; }
        return 0;
    }
}

#define F64(x) static_cast<double*>(x)
#define F32(x) static_cast<float*>(x)
#define C64(x) static_cast<const double*>(x)
#define C32(x) static_cast<const float*>(x)

REF_API const char* ref_ib_message() { return message; }

REF_API int ref_ib_ghost(int dtype, const Dims* d, const void* dem, const void* x, const void* y, const void* z, const void* dz, int bc,
                         double dx, double dy, int n_idw, int offx, int offy)
{
    if (dtype == 0) return ghost(*d, C64(dem), C64(x), C64(y), C64(z), C64(dz), bc, dx, dy, n_idw, offx, offy);
    return ghost(*d, C32(dem), C32(x), C32(y), C32(z), C32(dz), bc, dx, dy, n_idw, offx, offy);
}
// ints: i, j, k, ip_i, ip_j, ip_k; reals: xb, yb, zb, xi, yi, zi, di, ip_d, c_idw, c_idw_sum
REF_API void ref_ib_ghost_get(int dtype, int** ints, void** reals)
{
    if (dtype == 0) get<double>(ints, reinterpret_cast<double**>(reals));
    else            get<float>(ints, reinterpret_cast<float**>(reals));
}
REF_API int ref_ib_interp(int dtype, const Dims* d, int n, const void* xp, const void* yp, const void* x, const void* y, const void* plane,
                          double dx, double dy, int offx, int offy, void* out)
{
    if (dtype == 0) return interp(*d, n, C64(xp), C64(yp), C64(x), C64(y), C64(plane), dx, dy, offx, offy, F64(out));
    return interp(*d, n, C32(xp), C32(yp), C32(x), C32(y), C32(plane), dx, dy, offx, offy, F32(out));
}
REF_API void ref_ib_set_ghost_cells(int dtype, const Dims* d, void* fld, const void* bv, const void* c_idw, const void* c_idw_sum, const void* di,
                                    const int* gi, const int* gj, const int* gk, const int* ipi, const int* ipj, const int* ipk,
                                    int bc, double visc, int nghost, int n_idw)
{
    if (dtype == 0) set_ghost_cells<double>(F64(fld), C64(bv), C64(c_idw), C64(c_idw_sum), C64(di), gi, gj, gk, ipi, ipj, ipk, type_of(bc), visc, nghost, n_idw, d->icells, d->ijcells);
    else            set_ghost_cells<float>(F32(fld), C32(bv), C32(c_idw), C32(c_idw_sum), C32(di), gi, gj, gk, ipi, ipj, ipk, type_of(bc), float(visc), nghost, n_idw, d->icells, d->ijcells);
}
REF_API void ref_ib_mask(int dtype, const Dims* d, void* mask, void* maskh, const void* dem, const void* z, const void* zh)
{
    if (dtype == 0) calc_mask<double>(F64(mask), F64(maskh), C64(dem), C64(z), C64(zh), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
    else            calc_mask<float>(F32(mask), F32(maskh), C32(dem), C32(z), C32(zh), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
}
REF_API void ref_ib_k_dem(int dtype, const Dims* d, unsigned int* k_dem, const void* dem, const void* z)
{
    if (dtype == 0) find_k_dem<double>(k_dem, C64(dem), C64(z), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells);
    else            find_k_dem<float>(k_dem, C32(dem), C32(z), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells);
}
// dxi, dyi: gd.dxi, gd.dyi (1./dx narrowed, src/grid.cxx:244)
REF_API void ref_ib_fluxes(int dtype, const Dims* d, void* flux, const unsigned int* k_dem, const void* s, double dx, double dy, const void* dz,
                           double dxi, double dyi, const void* dzhi, double svisc)
{
    if (dtype == 0) calc_fluxes<double>(F64(flux), k_dem, C64(s), dx, dy, C64(dz), dxi, dyi, C64(dzhi), svisc, d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
    else            calc_fluxes<float>(F32(flux), k_dem, C32(s), float(dx), float(dy), C32(dz), float(dxi), float(dyi), C32(dzhi), float(svisc), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
}
