// ref_outflow_shim.cpp -- TEST infrastructure: the reference's own Boundary_outflow loops behind a C interface.
//
// Compiled by tests/outflow_ref.py into a temporary directory with the reference's src and include directories and
// tests/stubs_syntax_only on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections
// collected at link time); nothing compiled from it is kept. The translation unit is included in place and unmodified, so that the
// functions of its anonymous namespace (compute_inoutflow_2nd, compute_inflow_4th, compute_outflow_4th) are visible here. What is
// written here is the calls only, in the order and with the arguments of Boundary_outflow<TF>::exec (src/boundary_outflow.cxx:
// 236-343) -- gd.kgc in the place of jgc, as there. The class itself is never constructed: its members read Master, Grid and Input,
// and the mpicoordx / mpicoordy tests of exec become the bits of `mask`.
#include "boundary_outflow.cxx"
#include "ref_shim.h"

namespace
{
    struct ODims { int istart, iend, igc, jstart, jend, jgc, kgc, icells, jcells, kcells, ijcells; };
    enum { WEST = 1, EAST = 2, SOUTH = 4, NORTH = 8 };

    template<class TF, Edge_location edge>
    void edge_2nd(TF* a, const TF* prof, const ODims& d, bool inflow)
    {
        if (inflow)
            compute_inoutflow_2nd<TF, edge, Flow_direction::Inflow>(
                    a, prof,
                    d.istart, d.iend, d.igc,
                    d.jstart, d.jend, d.kgc,
                    d.icells, d.jcells, d.kcells,
                    d.ijcells);
        else
            compute_inoutflow_2nd<TF, edge, Flow_direction::Outflow>(
                    a, prof,
                    d.istart, d.iend, d.igc,
                    d.jstart, d.jend, d.kgc,
                    d.icells, d.jcells, d.kcells,
                    d.ijcells);
    }

    template<class TF>
    void exec(int order, const ODims& d, void* data, const void* profile, const int* inflow, int mask)
    {
        TF* a = static_cast<TF*>(data);
        const TF* prof = static_cast<const TF*>(profile);
        if (order == 4)
        {
            if (mask & WEST) compute_inflow_4th<TF>(a, TF(0.), d.istart, d.icells, d.jcells, d.kcells, d.ijcells);
            if (mask & EAST) compute_outflow_4th<TF>(a, d.iend, d.icells, d.jcells, d.kcells, d.ijcells);
            return;
        }
        if (mask & WEST)  edge_2nd<TF, Edge_location::West >(a, prof, d, inflow[0] != 0);
        if (mask & EAST)  edge_2nd<TF, Edge_location::East >(a, prof, d, inflow[1] != 0);
        if (mask & SOUTH) edge_2nd<TF, Edge_location::South>(a, prof, d, inflow[2] != 0);
        if (mask & NORTH) edge_2nd<TF, Edge_location::North>(a, prof, d, inflow[3] != 0);
    }
}

// Boundary_outflow<TF>::exec(data, inflow_prof) on a rank that owns the edges of `mask`; inflow[4]: West, East, South, North
REF_API void ref_outflow_exec(int dtype, int order, const ODims* d, void* data, const void* profile, const int* inflow, int mask)
{
    if (dtype == 0) exec<double>(order, *d, data, profile, inflow, mask); else exec<float>(order, *d, data, profile, inflow, mask);
}
