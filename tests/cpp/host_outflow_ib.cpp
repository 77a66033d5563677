// tests/cpp/host_outflow_ib.cpp -- the head of Model::exec with an immersed boundary and open lateral boundaries, through the C++ host
// classes of microhh_amd/host/mhh_host.h and mhh_host_rccl.h: both calls of boundary->set_prognostic_outflow_bcs, the one after the
// cyclic fills (src/model.cxx:346-347) and the one after ib->exec_scalars (:380-383). Built and run by
// tests/test_cpp_host_outflow.py, which compares th, bit for bit, with what the Python driver leaves after the same four calls.
//   host_outflow_ib IN OUT itot jtot ktot n_idw sbot visc slab
// IN: u v w th [ncells each], dem [ijcells, halos filled], z zh dz dzh dzi dzhi [kcells each], the inflow profile of th [ktot]
// OUT: th after the first pair of calls, th after the second pair [ncells each]
// slab = 1: the first pair is Substep_slab::cyclic_outflow on a ONE-rank RCCL communicator (the exchange to self, then exec_all with
// the rank's edge mask, which on one rank holds all four edges), and can_overlap turns false once set_outflow has been called.
// gc = (3, 3, 1), second order, double, the domain of drycblles; West inflow, the other edges outflow; sbcbot = flux.
#include "host_prog.h"
#include "../../microhh_amd/host/mhh_host_rccl.h"

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 10, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 3200., 3200., 1200.);
        const int n_idw = std::atoi(argv[6]);
        const TF sbot = std::atof(argv[7]), visc = std::atof(argv[8]);
        const bool slab = std::atoi(argv[9]) != 0;
        const size_t n3 = gd.ncells, n2 = gd.ijcells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        fields.visc = visc;
        for (const char* n : {"u", "v", "w"}) { fields.mp[n] = std::make_shared<Field3d<TF>>(); fields.mp[n]->fld_g = up(rd(n3)); }
        fields.sp["th"] = std::make_shared<Field3d<TF>>(); fields.sp["th"]->fld_g = up(rd(n3)); fields.sp["th"]->visc = visc;
        std::vector<TF> dem = rd(n2);
        read_metrics(grid, rd);
        const std::vector<TF> prof = rd(gd.ktot);
        rd.close();

        Immersed_boundary<TF> ib(grid, fields);
        ib.sbcbot = MHH_IB_FLUX; ib.sbc["th"] = sbot; ib.dem = dem; ib.n_idw_points = n_idw;
        ib.alloc = [](size_t bytes) { void* d; HIPCHK(hipMalloc(&d, bytes)); return d; };
        ib.upload = [](void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); };
        ib.release = [](void* d) { HIPCHK(hipFree(d)); };
        ib.create();
        ib.prepare_device();

        Boundary_cyclic<TF> boundary_cyclic(grid);
        Boundary_outflow<TF> boundary_outflow(grid, {{Edge_location::West, Flow_direction::Inflow}, {Edge_location::East, Flow_direction::Outflow},
                                                     {Edge_location::South, Flow_direction::Outflow}, {Edge_location::North, Flow_direction::Outflow}},
                                              {"th"});
        std::map<std::string, TF*> inflow_profiles{{"th", up(boundary_outflow.inflow_profile(prof))}};
        TF* first = dev<TF>(n3);
        if (!slab)
        {
            for (auto& it : fields.mp) boundary_cyclic.exec_g(it.second->fld_g);      // :346
            for (auto& it : fields.sp) boundary_cyclic.exec_g(it.second->fld_g);
            boundary_outflow.exec_all(fields, inflow_profiles);                       // :347
            HIPCHK(hipMemcpy(first, fields.sp["th"]->fld_g, n3*sizeof(TF), hipMemcpyDeviceToDevice));
            ib.exec_scalars();                                                        // :380
            boundary_outflow.exec_all(fields, inflow_profiles);                       // :383
        }
        else
        {
            Master_rccl master;
            master.init(1, 0, Master_rccl::unique_id(), nullptr);
            Boundary_cyclic_slab<TF> halo(master, grid);
            Boundary<TF> boundary;
            auto advec = Advec<TF>::factory(grid, fields, "2i5");
            auto diff = Diff<TF>::factory(grid, fields, boundary, "smag2");
            Substep_slab<TF> sub(master, grid, fields, halo);
            if (!sub.can_overlap(*advec, *diff)) return 6;                           // the scheme pair and the slab allow the overlap ...
            sub.set_outflow(&boundary_outflow, inflow_profiles);
            if (sub.can_overlap(*advec, *diff)) return 7;                            // ... and open boundaries forbid it
            if (boundary_outflow.edges() != (MHH_OUTFLOW_WEST | MHH_OUTFLOW_EAST | MHH_OUTFLOW_SOUTH | MHH_OUTFLOW_NORTH)) return 8;
            sub.cyclic_outflow();                                                     // :346-347
            HIPCHK(hipStreamSynchronize(master.stream));
            HIPCHK(hipMemcpy(first, fields.sp["th"]->fld_g, n3*sizeof(TF), hipMemcpyDeviceToDevice));
            ib.cyclic = [&](const std::vector<TF*>& f, void*) { halo.exec_g(f); };
            ib.exec_scalars(master.stream);                                           // :380
            boundary_outflow.exec_all(fields, inflow_profiles, master.stream);        // :383
            HIPCHK(hipStreamSynchronize(master.stream));
        }
        HIPCHK(hipDeviceSynchronize());
        Writer wr(argv[2]);
        wr(first, n3);
        wr(fields.sp["th"]->fld_g, n3);
        wr.close();
        ib.clear_device();
        std::printf("host_outflow_ib ok\n");
        return 0;
    });
}
