// integration/adaptor_immersed_boundary.cxx -- replaces src/immersed_boundary.cu: the USECUDA members exec_momentum (:83-137),
// exec_scalars (:140-169), prepare_device (:173-250) and clear_device (:253-283) of Immersed_boundary<TF>. Everything else of the
// class stays the reference's host code (src/immersed_boundary.cxx): init, create -- whose calc_ghost_cells, find_k_dem and
// interp2_dem the library restates bit for bit as mhh_ib_ghost_cells_host, mhh_ib_k_dem_host and mhh_ib_interp_dem_host, for
// drivers that have no such class --, get_mask and exec_cross, which run on the host there.
//
// The device tables are the library's, not the reference's: of the sixteen device arrays of Ghost_cells<TF> five are used, with
// another content. i_g holds ONE linear cell offset per ghost cell, ip_i_g the offsets of the interpolation points TRANSPOSED
// ([n_idw][nghost]), c_idw_g the weights transposed; c_idw_sum_g and di_g are as there; j_g, k_g, ip_j_g, ip_k_g and the
// coordinate arrays are not used: the reference declares them without initialisers, and prepare_device sets them to null. u, v
// and w are set in one launch and all scalars in one; the reference launches once per field.
#include <stdexcept>
#include <string>
#include <vector>
#include "master.h"
#include "grid.h"
#include "fields.h"
#include "immersed_boundary.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 1 = host to device

namespace
{
    template<typename T>
    T* mhh_put(const std::vector<T>& v)
    {
        void* d = nullptr;
        if (hipMalloc(&d, (v.empty() ? 1 : v.size())*sizeof(T)) != 0) throw std::runtime_error("hipMalloc");
        if (!v.empty() && hipMemcpy(d, v.data(), v.size()*sizeof(T), 1) != 0) throw std::runtime_error("hipMemcpy");
        return static_cast<T*>(d);
    }

    // clear_device frees what prepare_device made and nothing else: before it has run the pointers of Ghost_cells<TF> hold
    // whatever the reference's declaration left in them
    bool mhh_prepared = false;

    template<typename T> void mhh_drop(T*& p) { if (p) hipFree(p); p = nullptr; }

    template<typename TF>
    mhh_ib_job mhh_job(TF* fld, const TF* bv, Boundary_type bc, TF visc, const Ghost_cells<TF>& gh)
    {
        mhh_ib_job j{};
        j.fld = fld; j.boundary_value = bv; j.nghost = gh.nghost; j.visc = visc;
        j.bc = (bc == Boundary_type::Dirichlet_type) ? MHH_IB_DIRICHLET : (bc == Boundary_type::Neumann_type) ? MHH_IB_NEUMANN : MHH_IB_FLUX;
        j.cell = gh.i_g; j.ip = gh.ip_i_g; j.c_idw = gh.c_idw_g; j.c_idw_sum = gh.c_idw_sum_g; j.di = gh.di_g;
        return j;
    }
}

template<typename TF>
void Immersed_boundary<TF>::exec_momentum()
{
    if (sw_ib == IB_type::Disabled)
        return;

    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());

    mhh_ib_job jobs[3];
    int n = 0;
    for (const char* name : {"u", "v", "w"})
        jobs[n++] = mhh_job<TF>(fields.mp.at(name)->fld_g, ghost.at(name).mbot_g, Boundary_type::Dirichlet_type, fields.visc, ghost.at(name));
    mhh_check(mhh_ib_set_ghost_cells(&g, n_idw_points, jobs, 3, nullptr));

    boundary_cyclic.exec_g(fields.mp.at("u")->fld_g);
    boundary_cyclic.exec_g(fields.mp.at("v")->fld_g);
    boundary_cyclic.exec_g(fields.mp.at("w")->fld_g);
    mhh_check(mhh_synchronize(nullptr));
}

template<typename TF>
void Immersed_boundary<TF>::exec_scalars()
{
    if (sw_ib == IB_type::Disabled || fields.sp.empty())
        return;

    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());

    std::vector<mhh_ib_job> jobs;
    for (auto& it : fields.sp)
        jobs.push_back(mhh_job<TF>(it.second->fld_g, ghost.at("s").sbot_g.at(it.first), sbcbot, it.second->visc, ghost.at("s")));
    mhh_check(mhh_ib_set_ghost_cells(&g, n_idw_points, jobs.data(), (int)jobs.size(), nullptr));

    for (auto& it : fields.sp)
        boundary_cyclic.exec_g(it.second->fld_g);
    mhh_check(mhh_synchronize(nullptr));
}

template<typename TF>
void Immersed_boundary<TF>::prepare_device()
{
    if (sw_ib == IB_type::Disabled)
        return;

    auto& gd = grid.get_grid_data();
    if ((long long)gd.ijcells*gd.kcells > 2147483647LL)
        throw std::runtime_error("Immersed_boundary: a grid of more than 2^31-1 cells: the tables hold 32-bit cell offsets");
    const int nq = n_idw_points;

    for (auto& it : ghost)
    {
        Ghost_cells<TF>& gh = it.second;
        const size_t n = gh.nghost;
        std::vector<int> cell(n), ip(n*nq);
        std::vector<TF> c(n*nq);
        for (size_t m=0; m<n; ++m)
        {
            cell[m] = gh.i[m] + gh.j[m]*gd.icells + gh.k[m]*gd.ijcells;
            for (int q=0; q<nq; ++q)
            {
                ip[q*n + m] = gh.ip_i[m*nq + q] + gh.ip_j[m*nq + q]*gd.icells + gh.ip_k[m*nq + q]*gd.ijcells;
                c [q*n + m] = gh.c_idw[m*nq + q];
            }
        }
        gh.j_g = gh.k_g = gh.ip_j_g = gh.ip_k_g = nullptr;
        gh.xb_g = gh.yb_g = gh.zb_g = gh.xi_g = gh.yi_g = gh.zi_g = gh.ip_d_g = nullptr;
        gh.mbot_g = nullptr;
        gh.i_g = mhh_put(cell);
        gh.ip_i_g = mhh_put(ip);
        gh.c_idw_g = mhh_put(c);
        gh.c_idw_sum_g = mhh_put(gh.c_idw_sum);
        gh.di_g = mhh_put(gh.di);
        if (it.first == "u" || it.first == "v" || it.first == "w")
            gh.mbot_g = mhh_put(gh.mbot);
        else
            for (auto& sb : gh.sbot)
                gh.sbot_g[sb.first] = mhh_put(sb.second);
    }
    mhh_prepared = true;
}

template<typename TF>
void Immersed_boundary<TF>::clear_device()
{
    if (sw_ib == IB_type::Disabled || !mhh_prepared)
        return;
    mhh_prepared = false;

    for (auto& it : ghost)
    {
        Ghost_cells<TF>& gh = it.second;
        mhh_drop(gh.i_g); mhh_drop(gh.ip_i_g); mhh_drop(gh.c_idw_g); mhh_drop(gh.c_idw_sum_g); mhh_drop(gh.di_g);
        if (it.first == "u" || it.first == "v" || it.first == "w")
            mhh_drop(gh.mbot_g);
        for (auto& sb : gh.sbot_g)
            mhh_drop(sb.second);
    }
}

template class Immersed_boundary<double>;
template class Immersed_boundary<float>;
#endif
