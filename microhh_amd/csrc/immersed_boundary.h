// immersed_boundary.h -- Immersed_boundary<TF> (src/immersed_boundary.cxx, src/immersed_boundary.cu) for sw_immersed_boundary=dem:
// the set-up of Immersed_boundary::create on the HOST (calc_ghost_cells, find_k_dem, interp2_dem; no GPU is touched, both drivers
// call the same code), and on the device the ghost-cell kernel (set_ghost_cells), the ib mask (calc_mask) and the wall flux of a
// scalar (calc_fluxes). Kernels and C-ABI entry points; included from k_stencil.hip.
//
// The device tables are not the reference's. One 32-bit linear cell offset stands for each (i, j, k) triple, and the per-point
// arrays are TRANSPOSED, [q][n] instead of [n][q], so that consecutive lanes read consecutive table entries. The ghost list keeps
// the k-j-i order of calc_ghost_cells, so neighbouring lanes address neighbouring cells; the field reads are an element gather
// that L2 serves (a ghost cell's points lie in the 3 x 3 x 8 box around it). No LDS, no reduction, no atomics.
//
// No ordering between lanes or jobs is needed: a list's interpolation points lie OUTSIDE the wall (z > dem at their own column,
// find_interpolation_points :247) and its ghost cells lie INSIDE (z <= dem, is_ghost_cell :121), so within a field the cells a
// launch reads and the cells it writes are disjoint; different jobs of a launch hold different fields.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace mhh
{
constexpr int IBNJ = MHH_IB_MAX_JOBS;

template<class TF> struct IbJob
{
    TF* fld; const TF* bv; const TF* c_idw; const TF* c_idw_sum; const TF* di; const int* cell; const int* ip;
    TF visc; int bc, nghost;
};
template<class TF> struct IbArgs { IbJob<TF> job[IBNJ]; int n_idw; };

// set_ghost_cells (src/immersed_boundary.cxx:441-485, src/immersed_boundary.cu:33-78): the sum over q in index order from TF(0), the
// Dirichlet boundary term last, ONE division by c_idw_sum[n], then 2*bv - vI, vI - bv*di or vI - (-bv/visc)*di.
template<class TF>
__global__ void __launch_bounds__(256) ib_set_ghost_cells_kernel(const IbArgs<TF> A)
{
    const IbJob<TF>& J = A.job[blockIdx.y];
    const unsigned n = blockIdx.x*256u + threadIdx.x;
    if (n >= (unsigned)J.nghost) return;
    const size_t ng = (size_t)J.nghost;
    const int n_idw = A.n_idw;
    const int n_loc = (J.bc == MHH_IB_DIRICHLET) ? n_idw-1 : n_idw;
    TF* __restrict__ fld = J.fld;
    const TF bv = J.bv[n];
    TF vI = TF(0);
    for (int q=0; q<n_loc; ++q)
        vI += J.c_idw[(size_t)q*ng + n] * fld[J.ip[(size_t)q*ng + n]];
    if (J.bc == MHH_IB_DIRICHLET)
        vI += J.c_idw[(size_t)(n_idw-1)*ng + n] * bv;
    vI /= J.c_idw_sum[n];
    TF out;
    if (J.bc == MHH_IB_DIRICHLET)    out = 2*bv - vI;
    else if (J.bc == MHH_IB_NEUMANN) out = vI - bv * J.di[n];
    else                             { const TF grad = -bv / J.visc; out = vI - grad * J.di[n]; }
    fld[J.cell[n]] = out;
}

// calc_mask (src/immersed_boundary.cxx:489-512): 1 where the level lies above the DEM of the column, interior cells only
template<class TF>
struct IbMaskOp
{
    TF* __restrict__ mask; TF* __restrict__ maskh; const TF* __restrict__ dem; const TF* __restrict__ z; const TF* __restrict__ zh; int icells;
    __device__ void operator()(int i, int j, int k, int ijk) const
    {
        const int ij = i + j*icells;
        const int is_not_ib = z[k] > dem[ij], is_not_ib_h = zh[k] > dem[ij];
        mask[ijk] = static_cast<TF>(is_not_ib);
        maskh[ijk] = static_cast<TF>(is_not_ib_h);
    }
};

// calc_fluxes (src/immersed_boundary.cxx:541-597): one thread per column, serial in k, the reference's operand order: the vertical
// flux, then west, east, south, north through the faces shared with a neighbour whose first level above the DEM is higher, then
// / (dx*dy). k_dem is held inside [kstart, kend] (what find_k_dem writes), so that a foreign plane cannot index outside the field.
template<class TF>
struct IbFluxbotOp
{
    TF* __restrict__ flux; const unsigned int* __restrict__ k_dem; const TF* __restrict__ s;
    TF dx, dy; const TF* __restrict__ dz; TF dxi, dyi; const TF* __restrict__ dzhi; TF svisc;
    int kstart, kend, icells, ijcells;
    __device__ void operator()(int, int, int, int ij) const
    {
        const int ii = 1, jj = icells;
        const size_t kk = ijcells;
        auto kd = [&](int c) { const int v = (int)k_dem[c]; return v < kstart ? kstart : (v > kend ? kend : v); };
        const int k0 = kd(ij);
        const size_t col = (size_t)ij;
        TF f;
        {
            const size_t ijk = col + k0*kk;
            f = -svisc*(s[ijk]-s[ijk-kk])*dzhi[k0] * dx*dy;
        }
        for (int k=k0; k<kd(ij-ii); ++k) { const size_t ijk = col + k*kk; f += -svisc*(s[ijk]-s[ijk-ii])*dxi * dy*dz[k]; }
        for (int k=k0; k<kd(ij+ii); ++k) { const size_t ijk = col + k*kk; f +=  svisc*(s[ijk+ii]-s[ijk])*dxi * dy*dz[k]; }
        for (int k=k0; k<kd(ij-jj); ++k) { const size_t ijk = col + k*kk; f += -svisc*(s[ijk]-s[ijk-jj])*dyi * dx*dz[k]; }
        for (int k=k0; k<kd(ij+jj); ++k) { const size_t ijk = col + k*kk; f +=  svisc*(s[ijk+jj]-s[ijk])*dyi * dx*dz[k]; }
        f /= dx*dy;
        flux[ij] = f;
    }
};

// ---- host side: the set-up of Immersed_boundary::create ----------------------------------------------------------------------
// What the reference throws (std::runtime_error, `throw 1`) is thrown here as well and becomes the error string at the entry point.
struct IbGrid { int icells, jcells, kcells, istart, iend, jstart, jend, kstart, kend, offx, offy; };

// std::pow(sum, TF(0.5)) (:44): powf for float; not sqrt
template<class TF> inline TF ib_distance(TF x1, TF y1, TF z1, TF x2, TF y2, TF z2)
{
    const TF ax = x2-x1, ay = y2-y1, az = z2-z1;
    return std::pow(ax*ax + ay*ay + az*az, TF(0.5));
}

// interp2_dem (:65-103): the bilinear value of the plane at (xg, yg). What decides the bits is kept: the cell index is a TF quotient
// plus the rank's offset AS TF, truncated; the last cell of a row or column steps back one BEFORE the bounds are checked; the
// weights are quotients by dx and dy; the two rows are blended in x first, then in y.
template<class TF>
inline TF ib_interp2(TF xg, TF yg, const TF* x, const TF* y, const TF* dem, TF dx, TF dy, const IbGrid& G)
{
    const TF half = TF(0.5);
    int ic = static_cast<int>((xg - half*dx) / dx + TF(G.offx));
    int jc = static_cast<int>((yg - half*dy) / dy + TF(G.offy));
    ic -= (ic == G.icells-1);
    jc -= (jc == G.jcells-1);
    if (ic < 0 || jc < 0 || ic >= G.icells-1 || jc >= G.jcells-1)
        throw std::runtime_error("IB dem interpolation out of bounds!");
    const TF wx = (xg - x[ic]) / dx, wy = (yg - y[jc]) / dy;
    const TF* south = dem + (size_t)jc*G.icells + ic;
    const TF* north = south + G.icells;
    return (TF(1) - wy) * ((TF(1) - wx) * south[0] + wx * south[1]) + wy * ((TF(1) - wx) * north[0] + wx * north[1]);
}

// is_ghost_cell (:107-185), the 3 x 3 x 3 "new method"
template<class TF>
inline bool ib_is_ghost(const TF* dem, const TF* x, const TF* y, const TF* z, TF dx, TF dy, int i, int j, int k, const IbGrid& G)
{
    const TF zdem = ib_interp2(x[i], y[j], x, y, dem, dx, dy, G);
    if (z[k] <= zdem)
        for (int dj=-1; dj<=1; ++dj)
            for (int di=-1; di<=1; ++di)
            {
                const TF zd = ib_interp2(x[i+di], y[j+dj], x, y, dem, dx, dy, G);
                for (int dk=-1; dk<=1; ++dk)
                    if (z[k+dk] > zd) return true;
            }
    return false;
}

template<class TF> struct IbNeighbour { int i, j, k; TF distance; };
template<class TF> inline bool ib_compare(const IbNeighbour<TF>& a, const IbNeighbour<TF>& b) { return a.distance < b.distance; }

template<class TF> struct IbLists
{
    std::vector<int> i, j, k, ip_i, ip_j, ip_k;
    std::vector<TF> xb, yb, zb, xi, yi, zi, di, ip_d, c_idw, c_idw_sum;
    bool scanned = false;          // i, j, k are there already: step 1 is not repeated
};

// What the counting call found, kept for the filling call that follows it: the scan visits every cell, and the two-call shape
// would otherwise pay for it twice. The filling call takes the list only if it is handed the same grid and the same values.
template<class TF> struct IbScan
{
    bool valid = false; IbGrid G{}; TF dx = 0, dy = 0; std::vector<TF> dem, x, y, z; std::vector<int> i, j, k;
    bool matches(const IbGrid& g, TF ddx, TF ddy, const TF* d, const TF* xx, const TF* yy, const TF* zz) const
    {
        auto same = [](const std::vector<TF>& v, const TF* p) { return !memcmp(v.data(), p, v.size()*sizeof(TF)); };
        return valid && !memcmp(&G, &g, sizeof(IbGrid)) && dx == ddx && dy == ddy && same(dem, d) && same(x, xx) && same(y, yy) && same(z, zz);
    }
};
template<class TF> inline IbScan<TF>& ib_scan() { static thread_local IbScan<TF> s; return s; }

// calc_ghost_cells (:334-426), steps 1 (count_only stops there) to 4
template<class TF>
static void ib_ghost_cells(IbLists<TF>& L, bool count_only, const TF* dem, const TF* x, const TF* y, const TF* z, const TF* dz,
                           int bc, TF dx, TF dy, int n_idw, const IbGrid& G)
{
    for (int k=G.kstart; k<G.kend && !L.scanned; ++k)
        for (int j=G.jstart; j<G.jend; ++j)
            for (int i=G.istart; i<G.iend; ++i)
                if (ib_is_ghost(dem, x, y, z, dx, dy, i, j, k, G))
                {
                    // find_interpolation_points reads z[k+dk] up to dk = 5 (:240-247): the reference reads past its arrays here
                    if (k+5 >= G.kcells)
                        throw std::runtime_error("IB ghost cell at i=" + std::to_string(i) + ", j=" + std::to_string(j) + ", k=" + std::to_string(k) +
                                                 " is too close to the top: the interpolation stencil reads level k+5 of " + std::to_string(G.kcells));
                    L.i.push_back(i); L.j.push_back(j); L.k.push_back(k);
                }
    if (count_only) return;
    const int nghost = (int)L.i.size();
    for (auto* v : {&L.xb, &L.yb, &L.zb, &L.xi, &L.yi, &L.zi, &L.di, &L.c_idw_sum}) v->assign(nghost, TF(0));
    // 2. find_nearest_location_wall (:188-220), the image point and its distance (:385-390)
    for (int n=0; n<nghost; ++n)
    {
        const TF x0 = x[L.i[n]], y0 = y[L.j[n]], z0 = z[L.k[n]];
        // the 41 x 41 points within one cell of the ghost cell, x outer and y inner; the FIRST of equal distances is kept. The offset
        // is a double fraction times the spacing, added to the coordinate in double and narrowed.
        constexpr int HALF = 20, SIDE = 2*HALF + 1;
        TF d_min = TF(1e12), x_min = 0, y_min = 0, z_min = 0;
        for (int m=0; m<SIDE*SIDE; ++m)
        {
            const double fx = double(2*(m/SIDE - HALF)) / double(2*HALF), fy = double(2*(m%SIDE - HALF)) / double(2*HALF);
            const TF xc = TF(double(x0) + fx*double(dx)), yc = TF(double(y0) + fy*double(dy));
            const TF zc = ib_interp2(xc, yc, x, y, dem, dx, dy, G);
            const TF d = ib_distance(x0, y0, z0, xc, yc, zc);
            if (d < d_min) { d_min = d; x_min = xc; y_min = yc; z_min = zc; }
        }
        L.xb[n] = x_min; L.yb[n] = y_min; L.zb[n] = z_min;
        L.xi[n] = 2*L.xb[n] - x0;
        L.yi[n] = 2*L.yb[n] - y0;
        L.zi[n] = 2*L.zb[n] - z0;
        L.di[n] = ib_distance(L.xi[n], L.yi[n], L.zi[n], x0, y0, z0);
    }
    // 3. find_interpolation_points (:223-285): candidates in the loop order dk, dj, di; std::sort on the distance alone
    const size_t np = (size_t)nghost*n_idw;
    L.ip_i.assign(np, 0); L.ip_j.assign(np, 0); L.ip_k.assign(np, 0); L.ip_d.assign(np, TF(0)); L.c_idw.assign(np, TF(0));
    std::vector<IbNeighbour<TF>> neighbours;
    for (int n=0; n<nghost; ++n)
    {
        const int i = L.i[n], j = L.j[n], k = L.k[n];
        neighbours.clear();
        const int dk0 = std::max(-2, G.kstart-k);
        for (int dk=dk0; dk<6; ++dk)
            for (int dj=-1; dj<2; ++dj)
                for (int di=-1; di<2; ++di)
                {
                    const TF zd = ib_interp2(x[i+di], y[j+dj], x, y, dem, dx, dy, G);
                    if (z[k+dk] > zd)
                    {
                        const TF distance = ib_distance(x[i], y[j], z[k], x[i+di], y[j+dj], z[k+dk]);
                        neighbours.push_back(IbNeighbour<TF>{i+di, j+dj, k+dk, distance});
                    }
                }
        std::sort(neighbours.begin(), neighbours.end(), ib_compare<TF>);
        if ((int)neighbours.size() < n_idw)
            throw std::runtime_error("only found " + std::to_string(neighbours.size()) + " interpolation points @ i=" + std::to_string(i) +
                                     ", j=" + std::to_string(j) + ", k=" + std::to_string(k));
        for (int q=0; q<n_idw; ++q)
        {
            const size_t in = q + (size_t)n*n_idw;
            L.ip_i[in] = neighbours[q].i; L.ip_j[in] = neighbours[q].j; L.ip_k[in] = neighbours[q].k; L.ip_d[in] = neighbours[q].distance;
        }
    }
    // 4. precalculate_idw (:288-331): Dirichlet uses n_idw-1 points plus the wall distance, held above 1e-9
    std::vector<TF> tmp(n_idw);
    for (int n=0; n<nghost; ++n)
    {
        const int nq = (bc == MHH_IB_DIRICHLET) ? n_idw-1 : n_idw;
        TF dist_max = TF(0);
        for (int q=0; q<nq; ++q)
        {
            const size_t qq = q + (size_t)n*n_idw;
            tmp[q] = ib_distance(L.xi[n], L.yi[n], L.zi[n], x[L.ip_i[qq]], y[L.ip_j[qq]], z[L.ip_k[qq]]);
            dist_max = std::max(dist_max, tmp[q]);
        }
        if (bc == MHH_IB_DIRICHLET)
        {
            tmp[n_idw-1] = std::max(ib_distance(L.xi[n], L.yi[n], L.zi[n], L.xb[n], L.yb[n], L.zb[n]), TF(1e-9));
            dist_max = std::max(dist_max, tmp[n_idw-1]);
        }
        for (int q=0; q<n_idw; ++q)
        {
            const size_t qq = q + (size_t)n*n_idw;
            L.c_idw[qq] = std::pow((dist_max - tmp[q]) / (dist_max * tmp[q]), 0.5) + TF(1e-9);     // a double exponent: pow in double
            L.c_idw_sum[n] += L.c_idw[qq];
        }
    }
}

inline int ib_check_setup(const mhh_grid* g, const char* who)
{
    if (int e = check_grid(g)) return e;
    if (g->ncells > 2147483647LL || (long long)g->ijcells*(long long)g->kcells > 2147483647LL)
    { set_error("%s: a grid of more than 2^31-1 cells: the tables hold 32-bit cell offsets", who); return MHH_EINVAL; }
    if (g->igc < 2 || g->jgc < 2)
    { set_error("%s: the immersed boundary needs at least two horizontal ghost cells (src/immersed_boundary.cxx:622), the grid has igc = %d, jgc = %d", who, g->igc, g->jgc); return MHH_EINVAL; }
    return MHH_OK;
}
inline IbGrid ib_grid(const mhh_grid* g, int offx, int offy)
{
    return IbGrid{g->icells, g->jcells, g->kcells, g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, offx, offy};
}

template<class TF>
static int ib_ghost_cells_entry(const mhh_grid* g, const void* dem, const void* x, const void* y, const void* z, const void* dz, int n_idw, int bc,
                                int offx, int offy, int* nghost, mhh_ib_ghost_lists* out)
{
    IbLists<TF> L;
    const IbGrid G = ib_grid(g, offx, offy);
    IbScan<TF>& scan = ib_scan<TF>();
    if (out && scan.matches(G, TF(g->dx), TF(g->dy), cp<TF>(dem), cp<TF>(x), cp<TF>(y), cp<TF>(z)))
    { L.i.swap(scan.i); L.j.swap(scan.j); L.k.swap(scan.k); L.scanned = true; }
    scan = IbScan<TF>();
    try { ib_ghost_cells<TF>(L, out == nullptr, cp<TF>(dem), cp<TF>(x), cp<TF>(y), cp<TF>(z), cp<TF>(dz), bc, TF(g->dx), TF(g->dy), n_idw, ib_grid(g, offx, offy)); }
    catch (const std::exception& e) { set_error("mhh_ib_ghost_cells_host: %s", e.what()); return MHH_EINVAL; }
    const int n = (int)L.i.size();
    if (!out)
    {
        scan.G = G; scan.dx = TF(g->dx); scan.dy = TF(g->dy); scan.i = L.i; scan.j = L.j; scan.k = L.k; scan.valid = true;
        scan.dem.assign(cp<TF>(dem), cp<TF>(dem) + g->ijcells); scan.x.assign(cp<TF>(x), cp<TF>(x) + g->icells);
        scan.y.assign(cp<TF>(y), cp<TF>(y) + g->jcells); scan.z.assign(cp<TF>(z), cp<TF>(z) + g->kcells);
        *nghost = n;
        return MHH_OK;
    }
    if (*nghost != n) { set_error("mhh_ib_ghost_cells_host: room for %d ghost cells, the search finds %d (count first: out = NULL)", *nghost, n); return MHH_EINVAL; }
    if (n == 0) return MHH_OK;
    const bool all = out->i && out->j && out->k && out->xb && out->yb && out->zb && out->xi && out->yi && out->zi && out->di &&
                     out->ip_i && out->ip_j && out->ip_k && out->ip_d && out->c_idw && out->c_idw_sum;
    if (!all) { set_error("mhh_ib_ghost_cells_host: null pointer in the lists"); return MHH_EINVAL; }
    std::copy(L.i.begin(), L.i.end(), out->i); std::copy(L.j.begin(), L.j.end(), out->j); std::copy(L.k.begin(), L.k.end(), out->k);
    std::copy(L.ip_i.begin(), L.ip_i.end(), out->ip_i); std::copy(L.ip_j.begin(), L.ip_j.end(), out->ip_j); std::copy(L.ip_k.begin(), L.ip_k.end(), out->ip_k);
    auto put = [](const std::vector<TF>& v, void* p) { std::copy(v.begin(), v.end(), mp<TF>(p)); };
    put(L.xb, out->xb); put(L.yb, out->yb); put(L.zb, out->zb); put(L.xi, out->xi); put(L.yi, out->yi); put(L.zi, out->zi); put(L.di, out->di);
    put(L.ip_d, out->ip_d); put(L.c_idw, out->c_idw); put(L.c_idw_sum, out->c_idw_sum);
    return MHH_OK;
}

// find_k_dem (:516-537): the first level of the column above the DEM (kend where there is none), interior columns
template<class TF>
static void ib_k_dem(const mhh_grid* g, const TF* dem, const TF* z, unsigned int* k_dem)
{
    for (int j=g->jstart; j<g->jend; ++j)
        for (int i=g->istart; i<g->iend; ++i)
        {
            const int ij = i + j*g->icells;
            int k;
            for (k=g->kstart; k<g->kend; ++k)
                if (z[k] > dem[ij]) break;
            k_dem[ij] = k;
        }
}

template<class TF>
static int ib_interp_entry(const mhh_grid* g, const void* plane, const void* x, const void* y, const void* xp, const void* yp, int n, int offx, int offy, void* out)
{
    try
    {
        const IbGrid G = ib_grid(g, offx, offy);
        for (int m=0; m<n; ++m)
            mp<TF>(out)[m] = ib_interp2<TF>(cp<TF>(xp)[m], cp<TF>(yp)[m], cp<TF>(x), cp<TF>(y), cp<TF>(plane), TF(g->dx), TF(g->dy), G);
    }
    catch (const std::exception& e) { set_error("mhh_ib_interp_dem_host: %s", e.what()); return MHH_EINVAL; }
    return MHH_OK;
}

template<class TF>
static int ib_launch(int n_idw, const mhh_ib_job* jobs, int njobs, hipStream_t st)
{
    for (int b=0; b<njobs; b+=IBNJ)      // a batch of IBNJ jobs travels by value with its launch
    {
        const int nb = std::min(IBNJ, njobs - b);
        IbArgs<TF> A{};
        A.n_idw = n_idw;
        int most = 0;
        for (int n=0; n<nb; ++n)
        {
            const mhh_ib_job& j = jobs[b + n];
            A.job[n] = IbJob<TF>{mp<TF>(j.fld), cp<TF>(j.boundary_value), cp<TF>(j.c_idw), cp<TF>(j.c_idw_sum), cp<TF>(j.di), j.cell, j.ip,
                                 TF(j.visc), j.bc, j.nghost};
            most = std::max(most, j.nghost);
        }
        if (!most) continue;             // terrain below the first level everywhere: nothing to set
        const dim3 grid((most + 255)/256, nb), block(256);
        hipLaunchKernelGGL(ib_set_ghost_cells_kernel<TF>, grid, block, 0, st, A);
        MHH_LAUNCH_CHECK();
    }
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

// calc_ghost_cells (src/immersed_boundary.cxx:334-426) of Immersed_boundary::create (:805-866) for ONE staggered location
MHH_API int mhh_ib_ghost_cells_host(const mhh_grid* g, const void* dem, const void* x, const void* y, const void* z, const void* dz, int n_idw, int bc,
                                    int mpi_offset_x, int mpi_offset_y, int* nghost, mhh_ib_ghost_lists* out)
{
    if (int e = ib_check_setup(g, "mhh_ib_ghost_cells_host")) return e;
    MHH_REQUIRE(dem && x && y && z && dz && nghost, "null pointer");
    MHH_REQUIRE(n_idw >= 1, "n_idw_points must be at least 1");
    if (bc != MHH_IB_DIRICHLET && bc != MHH_IB_NEUMANN && bc != MHH_IB_FLUX)
    { set_error("mhh_ib_ghost_cells_host: unknown boundary type %d (MHH_IB_DIRICHLET | NEUMANN | FLUX)", bc); return MHH_EINVAL; }
#define CALL(TF) ib_ghost_cells_entry<TF>(g, dem, x, y, z, dz, n_idw, bc, mpi_offset_x, mpi_offset_y, nghost, out)
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// find_k_dem (src/immersed_boundary.cxx:516-537, called at :909-914)
MHH_API int mhh_ib_k_dem_host(const mhh_grid* g, const void* dem, const void* z, unsigned int* k_dem)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(dem && z && k_dem, "null pointer");
    if (g->dtype == MHH_F64) ib_k_dem<double>(g, cp<double>(dem), cp<double>(z), k_dem); else ib_k_dem<float>(g, cp<float>(dem), cp<float>(z), k_dem);
    return MHH_OK;
}

// interp2_dem (src/immersed_boundary.cxx:65-103) of a plane at n points: the sbot_spatial values at (xb, yb) (:891-897)
MHH_API int mhh_ib_interp_dem_host(const mhh_grid* g, const void* plane, const void* x, const void* y, const void* xp, const void* yp, int n,
                                   int mpi_offset_x, int mpi_offset_y, void* out)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(n >= 0 && plane && x && y && (n == 0 || (xp && yp && out)), "null pointer");
#define CALL(TF) ib_interp_entry<TF>(g, plane, x, y, xp, yp, n, mpi_offset_x, mpi_offset_y, out)
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// set_ghost_cells (src/immersed_boundary.cxx:441-485; set_ghost_cells_g, src/immersed_boundary.cu:33-78) of exec_momentum (:640-674,
// .cu:108-137) and exec_scalars (:677-696, .cu:140-168): every job of the table in one launch
MHH_API int mhh_ib_set_ghost_cells(const mhh_grid* g, int n_idw, const mhh_ib_job* jobs, int njobs, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(n_idw >= 1, "n_idw_points must be at least 1");
    MHH_REQUIRE(jobs && njobs >= 1, "at least one job");
    for (int n=0; n<njobs; ++n)
    {
        const mhh_ib_job& j = jobs[n];
        if (j.bc != MHH_IB_DIRICHLET && j.bc != MHH_IB_NEUMANN && j.bc != MHH_IB_FLUX)
        { set_error("mhh_ib_set_ghost_cells: job %d: unknown boundary type %d (MHH_IB_DIRICHLET | NEUMANN | FLUX)", n, j.bc); return MHH_EINVAL; }
        if (j.nghost < 0) { set_error("mhh_ib_set_ghost_cells: job %d: nghost = %d", n, j.nghost); return MHH_EINVAL; }
        if (j.nghost > 0 && !(j.fld && j.boundary_value && j.c_idw && j.c_idw_sum && j.di && j.cell && j.ip))
        { set_error("mhh_ib_set_ghost_cells: job %d: null pointer", n); return MHH_EINVAL; }
    }
#define CALL(TF) ib_launch<TF>(n_idw, jobs, njobs, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_mask (src/immersed_boundary.cxx:489-512) of Immersed_boundary::get_mask (:930-946)
MHH_API int mhh_ib_mask(const mhh_grid* g, const void* dem, void* mask, void* maskh, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(dem && mask && maskh && g->z && g->zh, "null pointer");
#define CALL(TF) launch_interior(as_stream(stream), make_grid<TF>(g), g->kstart, g->kend, \
                                 IbMaskOp<TF>{mp<TF>(mask), mp<TF>(maskh), cp<TF>(dem), cp<TF>(g->z), cp<TF>(g->zh), g->icells})
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// calc_fluxes (src/immersed_boundary.cxx:541-597) of Immersed_boundary::exec_cross (:950-985): flux [ijcells], interior columns
MHH_API int mhh_ib_fluxbot(const mhh_grid* g, void* flux, const unsigned int* k_dem, const void* s, double svisc, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(flux && k_dem && s && g->dz && g->dzhi, "null pointer");
    MHH_REQUIRE(g->igc >= 1 && g->jgc >= 1 && g->kgc >= 1, "calc_fluxes reads one ghost cell in every direction");
    // gd.dxi = 1./gd.dx (src/grid.cxx:244): a double quotient of the narrowed spacing, narrowed
#define CALL(TF) launch_columns(as_stream(stream), make_grid<TF>(g), 1, IbFluxbotOp<TF>{mp<TF>(flux), k_dem, cp<TF>(s), TF(g->dx), TF(g->dy), cp<TF>(g->dz), \
                                TF(1./TF(g->dx)), TF(1./TF(g->dy)), cp<TF>(g->dzhi), TF(svisc), g->kstart, g->kend, g->icells, g->ijcells})
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
