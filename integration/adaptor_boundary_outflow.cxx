// integration/adaptor_boundary_outflow.cxx -- replaces the USECUDA half of the reference's Boundary_outflow
// (src/boundary_outflow.cu:145-292): exec. The parity target is the CPU path, src/boundary_outflow.cxx:236-343, which the .cu mirrors
// (gd.kgc in the place of jgc included). One call fills one scalar, as Boundary::set_prognostic_outflow_bcs issues them
// (src/boundary.cu); the four edges of that scalar go in two launches instead of four. A port of Boundary itself would hand all
// scalars of scalar_outflow to one mhh_boundary_outflow_exec, and could drop the throw on swtimedep_outflow (src/boundary.cxx:431):
// the inflow profile is a device table that Boundary::update_time_dependent may overwrite between steps.
#include <map>
#include "input.h"
#include "master.h"
#include "grid.h"
#include "boundary_outflow.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
template<typename TF>
void Boundary_outflow<TF>::exec(
        TF* const restrict data,
        const TF* const restrict inflow_prof)
{
    auto& gd = grid.get_grid_data();
    auto& md = master.get_MPI_data();

    const int order = grid.get_spatial_order() == Grid_order::Fourth ? 4 : 2;
    int dirs[4] = {MHH_OUTFLOW_OUTFLOW, MHH_OUTFLOW_OUTFLOW, MHH_OUTFLOW_OUTFLOW, MHH_OUTFLOW_OUTFLOW};
    if (order == 2)
    {
        const Edge_location edges[4] = {Edge_location::West, Edge_location::East, Edge_location::South, Edge_location::North};
        for (int e=0; e<4; ++e)
            dirs[e] = flow_direction.at(edges[e]) == Flow_direction::Inflow ? MHH_OUTFLOW_INFLOW : MHH_OUTFLOW_OUTFLOW;
    }
    const int mask = (md.mpicoordx == 0        ? MHH_OUTFLOW_WEST  : 0) | (md.mpicoordx == md.npx-1 ? MHH_OUTFLOW_EAST  : 0)
                   | (md.mpicoordy == 0        ? MHH_OUTFLOW_SOUTH : 0) | (md.mpicoordy == md.npy-1 ? MHH_OUTFLOW_NORTH : 0);

    void* fields[1] = {data};
    const void* profiles[1] = {inflow_prof};
    mhh_grid g = mhh_make_grid(gd, md);
    mhh_check(mhh_boundary_outflow_exec(&g, order, fields, 1, profiles, dirs, mask, nullptr));
}

template void Boundary_outflow<double>::exec(double* const restrict, const double* const restrict);
template void Boundary_outflow<float>::exec(float* const restrict, const float* const restrict);
#endif
