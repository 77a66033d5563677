// tests/cpp/host_moist.cpp -- Thermo_moist through the C++ host class of microhh_amd/host/mhh_host.h. Built and run by
// tests/test_cpp_host_moist.py, which hands the inputs over in a file of doubles and compares what this program writes back, bit for
// bit, with the same calls made through the Python binding.
//   host_moist IN OUT itot jtot ktot pbot
// IN: thl qt wt [ncells each], then thl0 qt0 [ktot each]. create_basestate, the means of thl and qt, exec (base state on the device
// and the buoyancy tendency), get_thermo_field("ql"). OUT: wt ql [ncells each], then the eight tables [kcells each].
// gc = (3, 3, 1), second order, double, a uniform grid of 6400 x 6400 x 3000 m.
#include "host_prog.h"
#include <cstring>

using namespace mhh_host;
typedef double TF;

int main(int argc, char** argv)
{
    return run_main(argc, argv, 7, [&]() -> int
    {
        Grid<TF> grid; auto& gd = grid.gd;
        make_grid(grid, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), 3, 3, 1, 6400., 6400., 3000.);
        const size_t nk = gd.kcells, n3 = gd.ncells;
        Reader rd(argv[1]);
        Fields<TF> fields;
        auto mk = [&]() { auto f = std::make_shared<Field3d<TF>>(); f->fld_g = up(rd(n3)); f->fld_mean_g = dev<TF>(nk); return f; };
        fields.sp["thl"] = mk(); fields.sp["qt"] = mk(); fields.mt["w"] = mk();
        const std::vector<TF> thl0 = rd(gd.ktot), qt0 = rd(gd.ktot);
        read_metrics(grid, rd);
        rd.close();

        Thermo_moist<TF> thermo(grid, fields);
        thermo.pbot = std::atof(argv[6]);
        TF** tabs[8] = {&thermo.pref_g, &thermo.prefh_g, &thermo.rhoref_g, &thermo.rhorefh_g, &thermo.thvref_g, &thermo.thvrefh_g, &thermo.exnref_g, &thermo.exnrefh_g};
        for (TF** t : tabs) *t = dev<TF>(nk);
        thermo.nonconv_g = dev<int>(1);
        auto upload = [](void* d, const void* s, size_t n) { HIPCHK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); };
        thermo.create_basestate(thl0, qt0, upload);
        if (fields.rhoref.size() != nk || fields.rhoref[gd.kstart] != thermo.rhoref[gd.kstart]) return 6;

        // fields->exec: the means of thl and qt
        mhh_grid g = grid.abi();
        const void* flds[2] = {fields.sp["thl"]->fld_g, fields.sp["qt"]->fld_g};
        void* profs[2] = {fields.sp["thl"]->fld_mean_g, fields.sp["qt"]->fld_mean_g};
        double* scratch = dev<double>(mhh_field_mean_scratch_elems(&g, 2));
        mhh_check(mhh_field_mean_profile(&g, flds, 2, profs, scratch, nullptr));
        thermo.exec();
        TF* ql = dev<TF>(n3);
        thermo.get_thermo_field(ql, "ql");
        bool refused = false;
        try { thermo.get_thermo_field(ql, "thv"); } catch (const std::runtime_error&) { refused = true; }
        if (!refused || thermo.get_basestate_vector("thvrefh") != thermo.thvrefh_g) return 7;
        HIPCHK(hipDeviceSynchronize());
        int nonconv = 0; HIPCHK(hipMemcpy(&nonconv, thermo.nonconv_g, sizeof(int), hipMemcpyDeviceToHost));
        if (nonconv) return 8;
        Writer wr(argv[2]);
        wr(fields.mt["w"]->fld_g, n3); wr(ql, n3);
        for (TF** t : tabs) wr(*t, nk);
        wr.close();
        std::printf("host_moist ok\n");
        return 0;
    });
}
