// boundary_outflow.h -- Boundary_outflow<TF>::exec (src/boundary_outflow.cxx:236-343, src/boundary_outflow.cu:147-291): open lateral
// boundaries for scalars. Kernels and C-ABI entry points; included from k_stencil.hip.
//
// A ghost-cell fill: it moves a few surfaces of the fields, not their volume. The reference launches once per scalar and edge; here
// all scalars go in TWO launches, West + East first and South + North behind them, which is the reference's order (West, East, South,
// North): the South / North rule runs over the ghost columns the West / East rule has just written, so the corners have its bits.
//   West / East: a lane owns one ghost cell. Lanes map over (row, side, ghost index), i.e. the 2*igc ghost cells of a row are
//     consecutive lanes and no lane idles, whatever igc is; a row is a (j, k) line of ALL jcells x kcells, as in the reference.
//   South / North: lanes run along i over ALL icells, so a wave reads and writes whole rows; a lane walks the ghost rows of both
//     sides at its level. The reference hands gd.kgc to the loops where they expect jgc (src/boundary_outflow.cxx:311, :333 and the
//     .cu alike), so kgc ghost rows are set and the rows beyond keep their cyclic values. That is reproduced: nrows_y = kgc.
//   Fourth order: compute_inflow_4th with value 0 at West and compute_outflow_4th at East in one launch, a lane per (row, side).
// No LDS, no DMA. The arithmetic is the reference's, operation for operation; this translation unit is built with contraction off.
#pragma once
#include "k_common.h"

namespace mhh
{
constexpr int OUTFLOW_WEST = MHH_OUTFLOW_WEST, OUTFLOW_EAST = MHH_OUTFLOW_EAST, OUTFLOW_SOUTH = MHH_OUTFLOW_SOUTH, OUTFLOW_NORTH = MHH_OUTFLOW_NORTH;

template<class TF> struct OutflowArgs
{
    TF* a[MHH_MAX_SCALARS]; const TF* prof[MHH_MAX_SCALARS];
    int inflow[4];                     // West, East, South, North: 1 = Flow_direction::Inflow
    int mask;
    int istart, iend, igc, jstart, jend, nrows_y, icells, jcells, kcells, ijcells;
};

// compute_inoutflow_2nd, the West / East branch (src/boundary_outflow.cxx:99-123). width = igc * (sides active), side0 = the first
// active side (0 West, 1 East). nrows * width <= the cells of a field, which check_grid keeps below 2^31.
template<class TF>
__global__ void __launch_bounds__(256) outflow_we_kernel(const OutflowArgs<TF> A, unsigned nrows, unsigned width, int side0)
{
    const unsigned t = blockIdx.x*256u + threadIdx.x;
    const unsigned row = t / width;
    if (row >= nrows) return;
    const int c = (int)(t - row*width);
    const int side = side0 + c / A.igc, n = c % A.igc;
    const int k = (int)(row / (unsigned)A.jcells);
    TF* __restrict__ a = A.a[blockIdx.y] + (size_t)row*A.icells;
    const int d   = side == 0 ? A.istart       : A.iend - 1;
    const int src = side == 0 ? A.istart + n   : A.iend - 1 - n;
    const int gc  = side == 0 ? A.istart - 1 - n : A.iend + n;
    if (A.inflow[side])
    {
        const TF ad = a[d];
        a[gc] = ad - (n+1)*TF(2)*(ad - A.prof[blockIdx.y][k]);
    }
    else
        a[gc] = a[src];
}

// compute_inoutflow_2nd, the South / North branch (:124-148) over all icells, the ghost columns included
template<class TF>
__global__ void __launch_bounds__(256) outflow_sn_kernel(const OutflowArgs<TF> A)
{
    const int i = (int)(blockIdx.x*256u + threadIdx.x);
    const int k = (int)blockIdx.y;
    if (i >= A.icells) return;
    TF* __restrict__ a = A.a[blockIdx.z] + (size_t)k*A.ijcells + i;
    // the table is read on an active inflow edge only: without one the caller may pass no profiles (the pointer is then null)
    const bool in_s = (A.mask & OUTFLOW_SOUTH) && A.inflow[2], in_n = (A.mask & OUTFLOW_NORTH) && A.inflow[3];
    const TF p = (in_s || in_n) ? A.prof[blockIdx.z][k] : TF(0);
    if (A.mask & OUTFLOW_SOUTH)
    {
        const TF ad = a[(size_t)A.jstart*A.icells];
        for (int j=0; j<A.nrows_y; ++j)
        {
            const size_t gc = (size_t)(A.jstart-1-j)*A.icells;
            if (A.inflow[2]) a[gc] = ad - (j+1)*TF(2)*(ad - p);
            else             a[gc] = a[(size_t)(A.jstart+j)*A.icells];
        }
    }
    if (A.mask & OUTFLOW_NORTH)
    {
        const TF ad = a[(size_t)(A.jend-1)*A.icells];
        for (int j=0; j<A.nrows_y; ++j)
        {
            const size_t gc = (size_t)(A.jend+j)*A.icells;
            if (A.inflow[3]) a[gc] = ad - (j+1)*TF(2)*(ad - p);
            else             a[gc] = a[(size_t)(A.jend-1-j)*A.icells];
        }
    }
}

// compute_inflow_4th with value = 0 (:173-193) and compute_outflow_4th (:151-171): three ghost columns from the three interior cells
// next to the edge, which the fill does not write (itot >= 3)
template<class TF>
__global__ void __launch_bounds__(256) outflow_4th_kernel(const OutflowArgs<TF> A, unsigned nrows, unsigned nsides, int side0)
{
    const unsigned t = blockIdx.x*256u + threadIdx.x;
    const unsigned row = t / nsides;
    if (row >= nrows) return;
    const int side = side0 + (int)(t - row*nsides);
    TF* __restrict__ a = A.a[blockIdx.y] + (size_t)row*A.icells;
    if (side == 0)
    {
        const int ijk = A.istart;
        const TF value = TF(0.);
        const TF a0 = a[ijk], a1 = a[ijk+1], a2 = a[ijk+2];
        a[ijk-1] = value + TF( 9./8.)*a0 - TF( 14./8.)*a1 + TF( 5./8.)*a2;
        a[ijk-2] = value + TF(33./8.)*a0 - TF( 54./8.)*a1 + TF(21./8.)*a2;
        a[ijk-3] = value + TF(65./8.)*a0 - TF(110./8.)*a1 + TF(45./8.)*a2;
    }
    else
    {
        const int ijk = A.iend-1;
        const TF a0 = a[ijk], a1 = a[ijk-1], a2 = a[ijk-2];
        a[ijk+1] = TF(2.)*a0 - TF( 3./2.)*a1 + TF(1./2.)*a2;
        a[ijk+2] = TF(3.)*a0 - TF( 7./2.)*a1 + TF(3./2.)*a2;
        a[ijk+3] = TF(5.)*a0 - TF(15./2.)*a1 + TF(7./2.)*a2;
    }
}

static thread_local int g_outflow_launches = 0;       // launches of this thread's last mhh_boundary_outflow_exec

template<class TF>
static int outflow_launch(const mhh_grid* g, int order, void* const* fields, int nf, const void* const* profiles, const int* dirs, int mask,
                          hipStream_t st)
{
    OutflowArgs<TF> A{};
    for (int n=0; n<MHH_MAX_SCALARS; ++n)
    {
        A.a[n] = mp<TF>(fields[n < nf ? n : 0]);
        A.prof[n] = profiles ? cp<TF>(profiles[n < nf ? n : 0]) : nullptr;
    }
    for (int e=0; e<4; ++e) A.inflow[e] = (order == 2 && dirs[e] == MHH_OUTFLOW_INFLOW);
    A.mask = mask;
    A.istart = g->istart; A.iend = g->iend; A.igc = g->igc; A.jstart = g->jstart; A.jend = g->jend; A.nrows_y = g->kgc;
    A.icells = g->icells; A.jcells = g->jcells; A.kcells = g->kcells; A.ijcells = g->ijcells;
    const unsigned nrows = (unsigned)g->jcells * (unsigned)g->kcells;
    const int nwe = ((mask & OUTFLOW_WEST) != 0) + ((mask & OUTFLOW_EAST) != 0), side0 = (mask & OUTFLOW_WEST) ? 0 : 1;
    if (order == 4)
    {
        if (nwe)
        {
            hipLaunchKernelGGL(outflow_4th_kernel<TF>, dim3((nrows*nwe + 255u)/256u, nf), dim3(256), 0, st, A, nrows, (unsigned)nwe, side0);
            MHH_LAUNCH_CHECK();
            ++g_outflow_launches;
        }
        return MHH_OK;
    }
    if (nwe)
    {
        const unsigned width = (unsigned)(nwe*g->igc);
        hipLaunchKernelGGL(outflow_we_kernel<TF>, dim3((nrows*width + 255u)/256u, nf), dim3(256), 0, st, A, nrows, width, side0);
        MHH_LAUNCH_CHECK();
        ++g_outflow_launches;
    }
    if (mask & (OUTFLOW_SOUTH | OUTFLOW_NORTH))
    {
        hipLaunchKernelGGL(outflow_sn_kernel<TF>, dim3((g->icells + 255)/256, g->kcells, nf), dim3(256), 0, st, A);
        MHH_LAUNCH_CHECK();
        ++g_outflow_launches;
    }
    return MHH_OK;
}
} // namespace mhh
using namespace mhh;

// Boundary::process_time_dependent_outflow's table (src/boundary.cxx:411-426): the ktot values at kstart .. kend-1 of a zeroed
// kcells vector. Host memory both; the inflow rule reads the zeros on the ghost levels.
MHH_API int mhh_boundary_outflow_profile_host(const mhh_grid* g, const void* prof_ktot, void* table_kcells)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(prof_ktot && table_kcells, "null pointer");
    const size_t w = g->dtype == MHH_F64 ? sizeof(double) : sizeof(float);
    memset(table_kcells, 0, (size_t)g->kcells*w);
    memcpy(static_cast<char*>(table_kcells) + (size_t)g->kstart*w, prof_ktot, (size_t)g->kmax*w);
    return MHH_OK;
}

// Boundary_outflow<TF>::exec (src/boundary_outflow.cxx:236-343; GPU src/boundary_outflow.cu:147-291) for all fields of
// Boundary::set_prognostic_outflow_bcs (src/boundary.cxx:464-469) in at most two launches. Only enqueues.
MHH_API int mhh_boundary_outflow_exec(const mhh_grid* g, int order, void* const* fields, int nfields, const void* const* profiles, const int* dirs,
                                      int edges_mask, void* stream)
{
    g_outflow_launches = 0;
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(order == 2 || order == 4, "order is 2 or 4 (Grid_order::Second, Grid_order::Fourth)");
    MHH_REQUIRE(nfields >= 0 && nfields <= MHH_MAX_SCALARS, "0..MHH_MAX_SCALARS fields per call");
    MHH_REQUIRE(edges_mask >= 0 && edges_mask < 16, "edges_mask is a combination of MHH_OUTFLOW_WEST, _EAST, _SOUTH, _NORTH");
    MHH_REQUIRE(nfields == 0 || fields, "null field list");
    for (int n=0; n<nfields; ++n) MHH_REQUIRE(fields[n] != nullptr, "null field");
    // the mirror of West reads istart .. istart+igc-1 and that of East iend-igc .. iend-1: with itot < igc these run into the other
    // side's ghost columns, which the fill itself writes (and, at West of a narrow grid, beyond the row)
    MHH_REQUIRE(g->imax >= g->igc, "itot < igc: the mirror would read ghost columns that the fill writes");
    if (order == 4)
    {
        MHH_REQUIRE(g->igc >= 3 && g->imax >= 3, "the fourth-order extrapolations write three ghost columns from three interior cells");
        edges_mask &= OUTFLOW_WEST | OUTFLOW_EAST;          // north and south stay cyclic
    }
    else
    {
        MHH_REQUIRE(dirs, "null dirs");
        for (int e=0; e<4; ++e)
            MHH_REQUIRE(dirs[e] == MHH_OUTFLOW_OUTFLOW || dirs[e] == MHH_OUTFLOW_INFLOW, "a direction is MHH_OUTFLOW_OUTFLOW or MHH_OUTFLOW_INFLOW");
        // South and North set kgc rows (the reference hands gd.kgc to the loops): rows jstart-1-j, jend+j for j < kgc lie outside the
        // field when kgc > jgc
        MHH_REQUIRE(g->kgc <= g->jgc, "kgc > jgc: the reference's South / North loops would index outside the field");
        // ... and their mirror reads rows jstart .. jstart+kgc-1 and jend-kgc .. jend-1, which must be interior rows
        if (edges_mask & (OUTFLOW_SOUTH | OUTFLOW_NORTH))
            MHH_REQUIRE(g->jmax >= g->kgc, "jmax < kgc: the mirror would read ghost rows that the fill writes");
        bool need_prof = false;
        for (int e=0; e<4; ++e) need_prof = need_prof || ((edges_mask >> e & 1) && dirs[e] == MHH_OUTFLOW_INFLOW);
        if (need_prof && nfields)
        {
            MHH_REQUIRE(profiles, "an inflow edge needs the profiles");
            for (int n=0; n<nfields; ++n) MHH_REQUIRE(profiles[n] != nullptr, "an inflow edge needs a profile per field");
        }
    }
    if (!nfields || !edges_mask) return MHH_OK;
#define CALL(TF) outflow_launch<TF>(g, order, fields, nfields, profiles, dirs, edges_mask, as_stream(stream))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}

// launches the calling thread's last mhh_boundary_outflow_exec made: at most two, whatever the number of fields and edges
MHH_API int mhh_boundary_outflow_last_launches(void) { return g_outflow_launches; }
