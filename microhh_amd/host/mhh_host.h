// mhh_host.h -- C++ host side of the drop-in: the reference's operator interfaces for the hot path, implemented by
// forwarding to the C ABI (include/mhh_hip.h).
//
// MicroHH selects its GPU backend at compile time: every operator's exec()/get_cfl()/... is defined once in the
// .cxx under `#ifndef USECUDA` and once in the .cu under `#ifdef USECUDA` (src/advec_2.cxx:265 <-> src/advec_2.cu:140,
// src/diff_smag2.cxx:882,902,937 <-> src/diff_smag2.cu:519,551,703,792,833, src/pres_2.cxx:64,97,389 <->
// src/pres_2.cu:215). This header provides those member functions -- same names, arguments and error behaviour
// (std::runtime_error on failure) -- over containers that mirror the slice of Grid_data / Field3d / Fields /
// Boundary / Thermo the operators touch. INTEGRATION.md shows the same bodies written against the reference's
// real classes (the adaptor translation units a MicroHH maintainer would add in place of the .cu files).
//
// Header-only, C++17, no HIP or torch types: device memory is owned by the caller (Field3d::init_device,
// src/field3d.cu:32-47) and travels as raw pointers.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/mhh_hip.h"

namespace mhh_host
{
template<typename TF> constexpr int mhh_dtype();
template<> constexpr int mhh_dtype<double>() { return MHH_F64; }
template<> constexpr int mhh_dtype<float>()  { return MHH_F32; }

inline void mhh_check(int rc) { if (rc != MHH_OK) throw std::runtime_error(std::string("mhh: ") + mhh_last_error()); }

// ---- containers (subset of include/grid.h:49-135, include/field3d.h:33-81, include/fields.h:132-161) ----------
template<typename TF>
struct Grid_data
{
    int itot, jtot, ktot, imax, jmax, kmax, igc, jgc, kgc;
    int icells, jcells, ijcells, kcells, ncells;
    int istart, jstart, kstart, iend, jend, kend;
    TF xsize, ysize, zsize, dx, dy;
    std::vector<TF> z, zh, dz, dzh, dzi, dzhi, dzi4, dzhi4;                    // host metrics [kcells]
    TF* z_g = nullptr; TF* zh_g = nullptr; TF* dz_g = nullptr; TF* dzh_g = nullptr;
    TF* dzi_g = nullptr; TF* dzhi_g = nullptr; TF* dzi4_g = nullptr; TF* dzhi4_g = nullptr;   // device copies (Grid::prepare_device)
    int npy = 1, mpicoordy = 0;                                                // slab decomposition (npx == 1)
    TF lat = 0, lon = 0;                                                       // [grid] lat, lon in degrees: Radiation_gcss's zenith angle
};

template<typename TF>
struct Field3d
{
    TF* fld_g = nullptr;
    TF* fld_mean_g = nullptr;          // [kcells] horizontal mean profile (Field3d::fld_mean_g, include/field3d.h:72)
    TF* flux_bot_g = nullptr; TF* flux_top_g = nullptr;
    TF visc = 0;
    TF* fld_bot_g = nullptr; TF* grad_bot_g = nullptr;    // [ijcells] surface value and gradient (Field3d::fld_bot_g, grad_bot_g): Boundary_surface
};

template<typename TF>
struct Fields
{
    using Map = std::map<std::string, std::shared_ptr<Field3d<TF>>>;
    Map mp, mt, sp, st, sd;            // momentum / tendencies / scalars / scalar tendencies / diagnostic (evisc, p)
    TF* rhoref_g = nullptr; TF* rhorefh_g = nullptr;
    std::vector<TF> rhoref, rhorefh;   // host copies (Pres::set_values runs on the host)
    TF visc = 0;
};

template<typename TF>
struct Grid
{
    Grid_data<TF> gd;
    const Grid_data<TF>& get_grid_data() const { return gd; }
    // C-ABI descriptor with device (default) or host metric pointers
    mhh_grid abi(bool host = false) const
    {
        mhh_grid g{};
        g.itot = gd.itot; g.jtot = gd.jtot; g.ktot = gd.ktot; g.imax = gd.imax; g.jmax = gd.jmax; g.kmax = gd.kmax;
        g.igc = gd.igc; g.jgc = gd.jgc; g.kgc = gd.kgc; g.icells = gd.icells; g.jcells = gd.jcells; g.ijcells = gd.ijcells; g.kcells = gd.kcells;
        g.istart = gd.istart; g.jstart = gd.jstart; g.kstart = gd.kstart; g.iend = gd.iend; g.jend = gd.jend; g.kend = gd.kend;
        g.dtype = mhh_dtype<TF>(); g.npx = 1; g.npy = gd.npy; g.mpicoordx = 0; g.mpicoordy = gd.mpicoordy;
        g.ncells = (long long)gd.ijcells * gd.kcells;
        g.xsize = gd.xsize; g.ysize = gd.ysize; g.zsize = gd.zsize; g.dx = gd.dx; g.dy = gd.dy;
        if (host) { g.z = gd.z.data(); g.zh = gd.zh.data(); g.dz = gd.dz.data(); g.dzh = gd.dzh.data(); g.dzi = gd.dzi.data(); g.dzhi = gd.dzhi.data(); g.dzi4 = gd.dzi4.data(); g.dzhi4 = gd.dzhi4.data(); }
        else      { g.z = gd.z_g; g.zh = gd.zh_g; g.dz = gd.dz_g; g.dzh = gd.dzh_g; g.dzi = gd.dzi_g; g.dzhi = gd.dzhi_g; g.dzi4 = gd.dzi4_g; g.dzhi4 = gd.dzhi4_g; }
        return g;
    }
};

// What Diff_smag2 reads from Boundary / Thermo (src/diff_smag2.cxx:1050-1180)
template<typename TF>
struct Boundary
{
    std::string swboundary = "default";
    TF* z0m_g = nullptr; TF* dudz_g = nullptr; TF* dvdz_g = nullptr; TF* dbdz_g = nullptr;
    std::string get_switch() const { return swboundary; }
};
template<typename TF>
struct Thermo
{
    std::string swthermo = "0";
    TF* N2_g = nullptr;            // get_thermo_field("N2") result, or null to have it evaluated from scalar `th`
    std::string th = "th"; TF* thref_g = nullptr; TF* threfh_g = nullptr; TF grav = 9.81;
    int swspatialorder = 2;        // grid.swspatialorder: calc_buoyancy_tend_2nd / _4th (src/thermo_dry.cxx:557-562)
    // swthermo == "buoy" (Thermo_buoy, src/thermo_buoy.cxx:303-325): the buoyancy scalar, [thermo] alpha and N2 (bs.alpha, bs.n2),
    // grid.utrans. alpha == 0 and n2 == 0: the flat form (wt only), otherwise the slope / stratified form (ut, wt, bt)
    std::string b = "b"; TF alpha = 0, n2 = 0, utrans = 0;
    std::string get_switch() const { return swthermo; }
    // Thermo_dry::exec (src/thermo_dry.cxx:551-565): the buoyancy tendency of w; Thermo_buoy::exec (src/thermo_buoy.cxx:347-395):
    // that of w, or of u, w and b. Defined after Fields/Grid below
    template<class G, class F> void exec(G& grid, F& fields, void* stream = nullptr)
    {
        mhh_grid g = grid.abi();
        if (swthermo == "dry")
            mhh_check(mhh_thermo_dry_buoyancy_tend(&g, swspatialorder, fields.mt.at("w")->fld_g, fields.sp.at(th)->fld_g, threfh_g, grav, stream));
        else if (swthermo == "buoy")
        {
            mhh_fields f = abi_fields(fields);
            mhh_check(mhh_thermo_buoy_tend(&g, swspatialorder, &f, scalar_index(fields, b), alpha, n2, utrans, stream));
        }
    }
    // Thermo_buoy::get_thermo_field_g("N2") (src/thermo_buoy.cxx:402-415, calc_N2 :49-61) into a caller-owned 3-D device field
    template<class G, class F> void get_thermo_field_N2(G& grid, F& fields, TF* N2_out, void* stream = nullptr)
    {
        if (swthermo != "buoy") throw std::runtime_error("get_thermo_field_N2: swthermo=buoy only");
        mhh_grid g = grid.abi();
        mhh_check(mhh_thermo_buoy_N2(&g, N2_out, fields.sp.at(b)->fld_g, n2, stream));
    }
};
struct Stats {};                   // calc_tend is a no-op off sampling steps (src/stats.cxx:1893-1896)

template<typename TF>
inline mhh_fields abi_fields(const Fields<TF>& f, const Boundary<TF>* b = nullptr)
{
    mhh_fields a{};
    a.u = f.mp.at("u")->fld_g; a.v = f.mp.at("v")->fld_g; a.w = f.mp.at("w")->fld_g;
    a.ut = f.mt.at("u")->fld_g; a.vt = f.mt.at("v")->fld_g; a.wt = f.mt.at("w")->fld_g;
    int n = 0;
    for (auto& it : f.sp)
    {
        if (n >= MHH_MAX_SCALARS) throw std::runtime_error("mhh: more than MHH_MAX_SCALARS scalars");
        a.s[n] = it.second->fld_g; a.st[n] = f.st.at(it.first)->fld_g; a.svisc[n] = it.second->visc;
        a.s_fluxbot[n] = it.second->flux_bot_g; a.s_fluxtop[n] = it.second->flux_top_g;
        ++n;
    }
    a.nscalars = n;
    a.evisc = f.sd.count("evisc") ? f.sd.at("evisc")->fld_g : nullptr;
    a.p = f.sd.count("p") ? f.sd.at("p")->fld_g : nullptr;
    a.rhoref = f.rhoref_g; a.rhorefh = f.rhorefh_g; a.visc = f.visc;
    a.u_fluxbot = f.mp.at("u")->flux_bot_g; a.u_fluxtop = f.mp.at("u")->flux_top_g;
    a.v_fluxbot = f.mp.at("v")->flux_bot_g; a.v_fluxtop = f.mp.at("v")->flux_top_g;
    if (b) { a.dudz = b->dudz_g; a.dvdz = b->dvdz_g; a.dbdz = b->dbdz_g; a.z0m = b->z0m_g; }
    return a;
}
template<typename TF>
inline int scalar_index(const Fields<TF>& f, const std::string& name)
{
    int n = 0;
    for (auto& it : f.sp) { if (it.first == name) return n; ++n; }
    return -1;
}

// ---- Field3d_io (include/field3d_io.h; src/field3d_io.cxx:54-230) ---------------------------------------------------
// Restart files in the reference's layout: the interior (kmax x jtot x itot, C order) as a raw TF stream, data + offset.
// Host arrays; a y-slab rank (npy > 1) writes / reads its rows of the shared global file at j offset mpicoordy*jmax.
template<typename TF>
class Field3d_io
{
    public:
        explicit Field3d_io(Grid<TF>& gridin) : grid(gridin) {}
        // tmp1 holds imax*jmax*(kend-kstart) values; tmp2 is unused (the reference's transposed write needs it)
        int save_field3d(const TF* data, TF* tmp1, TF*, const char* filename, TF offset, int kstart, int kend)
        {
            const auto& gd = grid.get_grid_data();
            const int kmax = kend - kstart;
            for (int k=0; k<kmax; ++k)
                for (int j=0; j<gd.jmax; ++j)
                    for (int i=0; i<gd.imax; ++i)
                        tmp1[i + j*gd.imax + k*gd.imax*gd.jmax] = data[i+gd.igc + (j+gd.jgc)*gd.icells + (k+kstart)*gd.ijcells] + offset;
            FILE* f = std::fopen(filename, (gd.npy > 1 && gd.mpicoordy > 0) ? "r+b" : "wb");
            if (!f) return 1;
            int nerror = 0;
            for (int k=0; k<kmax && !nerror; ++k)
            {
                const long long pos = ((long long)k*gd.jtot + (long long)gd.mpicoordy*gd.jmax) * gd.itot * (long long)sizeof(TF);
                if (std::fseek(f, pos, SEEK_SET)) { ++nerror; break; }
                const size_t n = (size_t)gd.imax*gd.jmax;
                if (std::fwrite(tmp1 + (size_t)k*n, sizeof(TF), n, f) != n) ++nerror;
            }
            if (std::fclose(f)) ++nerror;
            return nerror;
        }
        int load_field3d(TF* data, TF* tmp1, TF*, const char* filename, TF offset, int kstart, int kend)
        {
            const auto& gd = grid.get_grid_data();
            const int kmax = kend - kstart;
            FILE* f = std::fopen(filename, "rb");
            if (!f) return 1;
            int nerror = 0;
            for (int k=0; k<kmax && !nerror; ++k)
            {
                const long long pos = ((long long)k*gd.jtot + (long long)gd.mpicoordy*gd.jmax) * gd.itot * (long long)sizeof(TF);
                if (std::fseek(f, pos, SEEK_SET)) { ++nerror; break; }
                const size_t n = (size_t)gd.imax*gd.jmax;
                if (std::fread(tmp1 + (size_t)k*n, sizeof(TF), n, f) != n) ++nerror;
            }
            std::fclose(f);
            if (nerror) return nerror;
            for (int k=0; k<kmax; ++k)
                for (int j=0; j<gd.jmax; ++j)
                    for (int i=0; i<gd.imax; ++i)
                        data[i+gd.igc + (j+gd.jgc)*gd.icells + (k+kstart)*gd.ijcells] = tmp1[i + j*gd.imax + k*gd.imax*gd.jmax] - offset;
            return 0;
        }
    private:
        Grid<TF>& grid;
};

// ---- Boundary_cyclic (include/boundary_cyclic.h:35-70) ----------------------------------------------------------
enum class Edge { East_west_edge, North_south_edge, Both_edges };
template<typename TF>
class Boundary_cyclic
{
    public:
        explicit Boundary_cyclic(Grid<TF>& gridin) : grid(gridin) {}
        void init() {}
        void exec_g(TF* data, void* stream = nullptr)    { mhh_grid g = grid.abi(); mhh_check(mhh_boundary_cyclic(&g, data, MHH_EDGE_BOTH, stream)); }
        void exec_g(TF* data, Edge e, void* stream = nullptr) { mhh_grid g = grid.abi(); mhh_check(mhh_boundary_cyclic(&g, data, static_cast<int>(e), stream)); }
        void exec_2d_g(TF* data, void* stream = nullptr) { mhh_grid g = grid.abi(); mhh_check(mhh_boundary_cyclic_2d(&g, data, stream)); }
        // the unsigned int overloads of include/boundary_cyclic.h:46-47 (index masks)
        void exec_g(unsigned int* data, Edge e = Edge::Both_edges, void* stream = nullptr) { mhh_grid g = grid.abi(); mhh_check(mhh_boundary_cyclic_u32(&g, data, static_cast<int>(e), stream)); }
        void exec_2d_g(unsigned int* data, void* stream = nullptr) { mhh_grid g = grid.abi(); mhh_check(mhh_boundary_cyclic_2d_u32(&g, data, stream)); }
    private:
        Grid<TF>& grid;
};

// ---- Advec (include/advec.h:45-70) ----------------------------------------------------------------------------
template<typename TF>
class Advec
{
    public:
        Advec(Grid<TF>& gridin, Fields<TF>& fieldsin, int schemein, double cflmaxin = 1.0, std::vector<std::string> fluxlimit_listin = {}) :
            fluxlimit_list(std::move(fluxlimit_listin)), grid(gridin), fields(fieldsin), scheme(schemein), cflmax(cflmaxin), cflmin(1.e-5), work(nullptr)
        {
            // src/advec_2i5.cxx:39-45: the limited scalars need a second vertical ghost level
            if (!fluxlimit_list.empty() && scheme != MHH_ADVEC_2I5 && scheme != MHH_ADVEC_2I62) throw std::runtime_error("fluxlimit_list is an option of swadvec=2i5 and 2i62");
            if (!fluxlimit_list.empty() && grid.get_grid_data().kgc < 2) throw std::runtime_error("fluxlimit_list needs kgc >= 2");
        }
        virtual ~Advec() {}
        // swadvec as in src/advec.cxx:55-83
        static std::shared_ptr<Advec> factory(Grid<TF>& g, Fields<TF>& f, const std::string& swadvec, double cflmax = 1.0,
                                              std::vector<std::string> fluxlimit_list = {})
        {
            int s;
            if (swadvec == "0") s = 0;                 // Advec_disabled (src/advec_disabled.cxx)
            else if (swadvec == "2") s = MHH_ADVEC_2; else if (swadvec == "2i5") s = MHH_ADVEC_2I5; else if (swadvec == "4") s = MHH_ADVEC_4;
            else if (swadvec == "2i4") s = MHH_ADVEC_2I4; else if (swadvec == "2i62") s = MHH_ADVEC_2I62; else if (swadvec == "2i53") s = MHH_ADVEC_2I53; else if (swadvec == "4m") s = MHH_ADVEC_4M;
            else throw std::runtime_error("\"" + swadvec + "\" is an illegal value for swadvec");
            return std::make_shared<Advec>(g, f, s, cflmax, std::move(fluxlimit_list));
        }
        void set_reduce_workspace(void* device_scratch) { work = device_scratch; }   // >= mhh_reduce_work_bytes()
        void create(Stats&) {}
        void exec(Stats&, void* stream = nullptr)
        {
            if (scheme == 0) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields); mark_limited(f);
            mhh_check(mhh_advec_exec(&g, scheme, &f, stream));
        }
        // scalars named in advec.fluxlimit_list (src/advec_2i5.cxx:921)
        void mark_limited(mhh_fields& f) const
        {
            for (const std::string& nm : fluxlimit_list)
            {
                const int n = scalar_index(fields, nm);
                if (n < 0) throw std::runtime_error("fluxlimit_list: \"" + nm + "\" is not a prognostic scalar");
                f.s_fluxlimit[n] = 1;
            }
        }
        int get_scheme() const { return scheme; }
        std::vector<std::string> fluxlimit_list;
        double get_cfl(double dt, void* stream = nullptr)
        {
            if (scheme == 0) return cflmin;
            mhh_grid g = grid.abi(); double cfl = 0;
            mhh_check(mhh_advec_cfl(&g, scheme, fields.mp.at("u")->fld_g, fields.mp.at("v")->fld_g, fields.mp.at("w")->fld_g, dt, work, &cfl, stream));
            return cfl;
        }
        unsigned long get_time_limit(unsigned long idt, double dt, void* stream = nullptr)
        {
            if (scheme == 0) return ~0ul;              // Constants::ulhuge
            double cfl = get_cfl(dt, stream);
            cfl = std::max(cflmin, cfl);
            return idt * cflmax / cfl;
        }
    protected:
        Grid<TF>& grid; Fields<TF>& fields; int scheme; double cflmax; const double cflmin; void* work;
};

// ---- Diff (include/diff.h:37-71) -------------------------------------------------------------------------------
template<typename TF>
class Diff
{
    public:
        Diff(Grid<TF>& gridin, Fields<TF>& fieldsin, Boundary<TF>& boundaryin, int schemein, double dnmaxin = 0.4, TF csin = 0.23, TF tPrin = 1./3.) :
            tPr(tPrin), grid(gridin), fields(fieldsin), boundary(boundaryin), scheme(schemein), dnmax(dnmaxin), cs(csin), dnmul(0), mlen0_g(nullptr), work(nullptr), mlen2_g(nullptr), mlen2_neutral(false) {}
        virtual ~Diff() {}
        static std::shared_ptr<Diff> factory(Grid<TF>& g, Fields<TF>& f, Boundary<TF>& b, const std::string& swdiff, double dnmax = 0.4, TF cs = 0.23, TF tPr = 1./3.)
        {
            int s;
            if (swdiff == "0") s = 0;                  // Diff_disabled (src/diff_disabled.cxx)
            else if (swdiff == "2") s = MHH_DIFF_2; else if (swdiff == "4") s = MHH_DIFF_4; else if (swdiff == "smag2") s = MHH_DIFF_SMAG2;
            else throw std::runtime_error("\"" + swdiff + "\" is an illegal value for swdiff");
            return std::make_shared<Diff>(g, f, b, s, dnmax, cs, tPr);
        }
        void init() {}
        void set_reduce_workspace(void* device_scratch) { work = device_scratch; }
        // Diff_2/4::create: constant dnmul (src/diff_2.cxx:120-135); Diff_smag2 computes it per call
        void create(Stats&)
        {
            auto& gd = grid.get_grid_data();
            TF viscmax = fields.visc;
            for (auto& it : fields.sp) viscmax = std::max(it.second->visc, viscmax);
            dnmul = 0;
            for (int k=gd.kstart; k<gd.kend; ++k)
                dnmul = std::max(dnmul, std::abs(viscmax * (1./(gd.dx*gd.dx) + 1./(gd.dy*gd.dy) + 1./(gd.dz[k]*gd.dz[k]))));
        }
        // Diff_smag2::prepare_device (src/diff_smag2.cu:521-542): mlen0_device = caller-owned [kcells] device buffer that
        // receives the per-level mixing length; upload(dst_device, src_host, bytes) is the caller's H2D copy
        template<class Upload> void prepare_device(Boundary<TF>&, TF* mlen0_device, Upload upload)
        {
            if (scheme != MHH_DIFF_SMAG2) return;
            auto& gd = grid.get_grid_data();
            std::vector<TF> ml(gd.kcells);
            mhh_grid gh = grid.abi(true);
            mhh_check(mhh_smag2_mlen0_host(&gh, cs, ml.data()));
            upload(mlen0_device, ml.data(), ml.size()*sizeof(TF));
            mlen0_g = mlen0_device;
        }
        // Optional second table for a horizontally UNIFORM roughness length (swconstantz0-like set-ups): the squared mixing
        // length of calc_evisc per level (mhh_smag2_mlen2_host, same bits as the per-cell evaluation). Call after
        // prepare_device with the thermo switch known; mlen2_device = caller-owned [kcells] device buffer. Drop it
        // (clear_uniform_z0m) as soon as z0m may vary in the horizontal.
        template<class Upload> void set_uniform_z0m(TF z0m, bool neutral, TF* mlen2_device, Upload upload)
        {
            if (scheme != MHH_DIFF_SMAG2) return;
            auto& gd = grid.get_grid_data();
            std::vector<TF> ml(gd.kcells), m2(gd.kcells);
            mhh_grid gh = grid.abi(true);
            mhh_check(mhh_smag2_mlen0_host(&gh, cs, ml.data()));
            mhh_check(mhh_smag2_mlen2_host(&gh, boundary.get_switch() != "default", neutral ? 1 : 0, ml.data(), (double)z0m, m2.data()));
            upload(mlen2_device, m2.data(), m2.size()*sizeof(TF));
            mlen2_g = mlen2_device; mlen2_neutral = neutral;
        }
        void clear_uniform_z0m() { mlen2_g = nullptr; }
        void clear_device() { mlen0_g = nullptr; mlen2_g = nullptr; }
        void exec_viscosity(Thermo<TF>& thermo, void* stream = nullptr)
        {
            if (scheme != MHH_DIFF_SMAG2) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, &boundary); mhh_diff_params p = params(&thermo);
            mhh_check(mhh_diff_exec_viscosity(&g, scheme, &f, &p, stream));
        }
        // rows [j0, j1) (and, if j2 >= 0, [j2, j3) in the same launch) of exec_viscosity on a y-slab whose evisc ghost rows jstart-1
        // and jend are evaluated locally from the velocity halos instead of being exchanged (mhh_host_rccl.h, Substep_slab)
        void exec_viscosity_rows(Thermo<TF>& thermo, int j0, int j1, int j2 = -1, int j3 = -1, void* stream = nullptr)
        {
            if (scheme != MHH_DIFF_SMAG2) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, &boundary); mhh_diff_params p = params(&thermo);
            p.evisc_ghost_rows = 1;
            if (j2 < 0) mhh_check(mhh_diff_exec_viscosity_rows(&g, scheme, &f, &p, j0, j1, stream));
            else        mhh_check(mhh_diff_exec_viscosity_rows2(&g, scheme, &f, &p, j0, j1, j2, j3, stream));
        }
        // advec->exec + diff->exec on the rows [j0, j1) (and [j2, j3)): (advec_2i5, diff_smag2) only
        void exec_with_advec_rows(Advec<TF>& advec, int j0, int j1, int j2 = -1, int j3 = -1, void* stream = nullptr)
        {
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, &boundary); mhh_diff_params p = params(nullptr);
            if (j2 < 0) mhh_check(mhh_rhs_exec_rows(&g, advec.get_scheme(), scheme, &f, &p, j0, j1, stream));
            else        mhh_check(mhh_rhs_exec_rows2(&g, advec.get_scheme(), scheme, &f, &p, j0, j1, j2, j3, stream));
        }
        void exec(Stats&, void* stream = nullptr)
        {
            if (scheme == 0) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, &boundary); mhh_diff_params p = params(nullptr);
            mhh_check(mhh_diff_exec(&g, scheme, &f, &p, stream));
        }
        int get_scheme() const { return scheme; }
        // advec->exec + diff->exec of Model::exec (src/model.cxx:388-392) as ONE pass over the fields where the library
        // has a fused kernel for the scheme pair: (2,2), (2i5,smag2). The 4th-order pair stays two calls because the
        // reference switches the w ghost cells between them (Boundary_w_type, src/model.cxx:387,389).
        // fold_buoyancy: also add Thermo_dry's buoyancy tendency (the caller then skips thermo->exec; nothing between it and
        // advec->exec touches wt, src/model.cxx:365-388)
        void exec_with_advec(Advec<TF>& advec, Stats& stats, void* stream = nullptr, Thermo<TF>* fold_buoyancy = nullptr)
        {
            const int a = advec.get_scheme();
            if (!((a == MHH_ADVEC_2 && scheme == MHH_DIFF_2) || (a == MHH_ADVEC_2I5 && scheme == MHH_DIFF_SMAG2)))
            {
                if (fold_buoyancy) fold_buoyancy->exec(grid, fields, stream);
                advec.exec(stats, stream); exec(stats, stream);
                return;
            }
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, &boundary); mhh_diff_params p = params(nullptr);
            if (fold_buoyancy && fold_buoyancy->get_switch() == "dry")
            {
                p.buoyancy = fold_buoyancy->swspatialorder; p.th_for_N2 = scalar_index(fields, fold_buoyancy->th);
                p.threfh = fold_buoyancy->threfh_g; p.grav = fold_buoyancy->grav;
            }
            else if (fold_buoyancy && fold_buoyancy->get_switch() == "buoy")
            {   // the flat form is folded into the pass; the slope / stratified form runs on its own first, inside mhh_rhs_exec
                p.buoyancy = fold_buoyancy->swspatialorder; p.buoyancy_kind = 1; p.th_for_N2 = scalar_index(fields, fold_buoyancy->b);
                p.bg_n2 = fold_buoyancy->n2; p.alpha = fold_buoyancy->alpha; p.utrans = fold_buoyancy->utrans;
            }
            advec.mark_limited(f);
            mhh_check(mhh_rhs_exec(&g, a, scheme, &f, &p, stream));
        }
        double get_dn(double dt, void* stream = nullptr)
        {
            if (scheme == 0) return 1.e-9;                // Constants::dsmall (src/diff_disabled.cxx:56-60)
            if (scheme != MHH_DIFF_SMAG2) return dnmul*dt;
            mhh_grid g = grid.abi(); double d = 0;
            mhh_check(mhh_smag2_dnmul(&g, fields.sd.at("evisc")->fld_g, tPr, work, &d, stream));
            return d*dt;
        }
        unsigned long get_time_limit(unsigned long idt, double dt, void* stream = nullptr)
        {
            if (scheme == 0) return ~0ul;                 // Constants::ulhuge
            if (scheme != MHH_DIFF_SMAG2) return idt * dnmax / (dt * dnmul);
            mhh_grid g = grid.abi(); double d = 0;
            mhh_check(mhh_smag2_dnmul(&g, fields.sd.at("evisc")->fld_g, tPr, work, &d, stream));
            d = std::max(1.e-9, d);                       // Constants::dsmall
            return idt * dnmax / (dt * d);
        }
        mhh_diff_params params(Thermo<TF>* thermo) const
        {
            mhh_diff_params p{};
            p.cs = cs; p.tPr = tPr; p.surface_model = (boundary.get_switch() != "default"); p.mlen0 = mlen0_g;
            p.neutral = thermo ? (thermo->get_switch() == "0") : 0;
            if (mlen2_g && mlen2_neutral == (p.neutral != 0)) p.mlen2 = mlen2_g;
            p.th_for_N2 = -1;
            if (thermo && !p.neutral)
            {
                p.N2 = thermo->N2_g;
                if (p.N2) {}
                else if (thermo->get_switch() == "buoy")      // N2 of b inside the kernel (Thermo_buoy calc_N2, src/thermo_buoy.cxx:49-61)
                {
                    p.th_for_N2 = scalar_index(fields, thermo->b); p.buoyancy_kind = 1; p.bg_n2 = thermo->n2;
                }
                else { p.th_for_N2 = scalar_index(fields, thermo->th); p.thref = thermo->thref_g; p.grav = thermo->grav; }
            }
            return p;
        }
        TF tPr;
    protected:
        Grid<TF>& grid; Fields<TF>& fields; Boundary<TF>& boundary; int scheme; double dnmax; TF cs; double dnmul; TF* mlen0_g; void* work; TF* mlen2_g; bool mlen2_neutral;
};

// ---- Pres (include/pres.h:39-85) ---------------------------------------------------------------------------------
template<typename TF>
class Pres
{
    public:
        Pres(Grid<TF>& gridin, Fields<TF>& fieldsin, int orderin) : grid(gridin), fields(fieldsin), order(orderin), plan(nullptr), work(nullptr) {}
        virtual ~Pres() { clear_device(); }
        static std::shared_ptr<Pres> factory(Grid<TF>& g, Fields<TF>& f, const std::string& swpres)
        {
            if (swpres == "0") return std::make_shared<Pres>(g, f, 0);     // Pres_disabled (src/pres_disabled.cxx): every member does nothing
            if (swpres == "2") return std::make_shared<Pres>(g, f, 2);
            if (swpres == "4") return std::make_shared<Pres>(g, f, 4);
            throw std::runtime_error("\"" + swpres + "\" is an illegal value for swpres");
        }
        void init() {}
        void set_values() {}                  // the coefficient tables are built inside prepare_device from the host metrics
        void create(Stats&) {}
        void set_reduce_workspace(void* device_scratch) { work = device_scratch; }
        void prepare_device()
        {
            clear_device();
            if (order == 0) return;
            auto& gd = grid.get_grid_data();
            mhh_grid gh = grid.abi(true);
            mhh_check(mhh_pres_plan_create(&gh, order, gd.dz.data(), gd.dzhi.data(), gd.dzi4.data(), gd.dzhi4.data(), fields.rhoref.data(), fields.rhorefh.data(), &plan));
        }
        void clear_device() { if (plan) { mhh_pres_plan_destroy(plan); plan = nullptr; } }
        void exec(double dt, Stats&, void* stream = nullptr)
        {
            if (order == 0) return;
            if (!plan) throw std::runtime_error("Pres::exec before prepare_device");
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields);
            mhh_check(mhh_pres_exec(plan, &g, &f, dt, stream));
        }
        // pres->exec(sub_dt) and the momentum part of timeloop.exec() (src/model.cxx:411,484; src/timeloop.cxx:250-334) in one call:
        // the sub-step of u, v, w is applied in the kernel that stores the corrected tendencies. The caller's Timeloop::exec then
        // covers the scalars only. Same bits as exec() followed by the three sub-steps.
        void exec_with_timeloop(double sub_dt, int rkorder, int substep, double dt, Stats&, void* stream = nullptr)
        {
            if (order == 0) return;
            if (!plan) throw std::runtime_error("Pres::exec before prepare_device");
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields);
            mhh_check(mhh_pres_exec_rk(plan, &g, &f, sub_dt, rkorder, substep, dt, stream));
        }
        TF check_divergence(void* stream = nullptr)
        {
            if (order == 0) return TF(0);                          // src/pres_disabled.cxx: check_divergence returns 0
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields); double d = 0;
            mhh_check(mhh_pres_check_divergence(&g, order, &f, work, &d, stream));
            return static_cast<TF>(d);
        }
    protected:
        Grid<TF>& grid; Fields<TF>& fields; int order; mhh_pres_plan* plan; void* work;
};

// ---- Field3d_operators (include/field3d_operators.h:32-58; src/field3d_operators.cxx:45-66,132-155) ------------------------
// The reduction scratch is the caller's: device memory of scratch_elems(nfields) doubles (set_scratch). One rank; a slab rank
// sums its shares over the ranks itself (the reference's master.sum).
template<typename TF>
class Field3d_operators
{
    public:
        Field3d_operators(Grid<TF>& gridin, Fields<TF>&) : grid(gridin), scratch(nullptr) {}   // Fields: the reference's argument, not read here
        unsigned long long scratch_elems(int nfields) const { mhh_grid g = grid.abi(); return mhh_field_mean_scratch_elems(&g, nfields); }
        void set_scratch(double* device_scratch) { scratch = device_scratch; }
        void calc_mean_profile_g(TF* prof, const TF* fld, void* stream = nullptr)
        {
            mhh_grid g = grid.abi(); const void* f[1] = {fld}; void* p[1] = {prof};
            mhh_check(mhh_field_mean_profile(&g, f, 1, p, scratch, stream));
        }
        // the volume sums of several fields into DEVICE doubles (what Force's fixed flux reads without a host round trip)
        void calc_sums_g(double* sums_device, const TF* const* flds, int n, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_field_mean_sum(&g, reinterpret_cast<const void* const*>(flds), n, sums_device, scratch, stream));
        }
        // calc_mean_g returns a host TF, as the reference's does; download(dst_host, src_device, bytes) is the caller's D2H copy
        template<class Download> TF calc_mean_g(const TF* fld, double* sum_device, Download download, void* stream = nullptr)
        {
            auto& gd = grid.get_grid_data();
            const TF* f[1] = {fld};
            calc_sums_g(sum_device, f, 1, stream);
            mhh_check(mhh_synchronize(stream));
            double sum = 0; download(&sum, sum_device, sizeof(double));
            const TF mean = sum / (gd.itot * gd.jtot * gd.zsize);
            return mean;
        }
    private:
        Grid<TF>& grid; double* scratch;
};

// ---- Buffer (include/buffer.h:38-80; src/buffer.cxx) ---------------------------------------------------------------------------
template<typename TF>
class Buffer
{
    public:
        Buffer(Grid<TF>& gridin, Fields<TF>& fieldsin, bool swbufferin, bool swupdatein = false, TF zstartin = 0, TF sigmain = 2., TF betain = 2.) :
            grid(gridin), fields(fieldsin), zstart(zstartin), sigma(sigmain), beta(betain), bufferkstart(0), bufferkstarth(0),
            swbuffer(swbufferin), swupdate(swupdatein), sigma_g(nullptr), sigmah_g(nullptr) {}
        void init() {}
        // the starting levels of src/buffer.cxx:107-126, with its error
        void create(Stats&)
        {
            if (!swbuffer) return;
            auto& gd = grid.get_grid_data();
            bufferkstart = gd.kstart; bufferkstarth = gd.kstart;
            for (int k=gd.kstart; k<gd.kend; ++k)
            {
                if (gd.z[k] < zstart) ++bufferkstart;
                if (gd.zh[k] < zstart) ++bufferkstarth;
            }
            if (bufferkstarth == gd.kend) throw std::runtime_error("Buffer is too close to the model top");
        }
        // sigma_device = caller-owned [2*kcells] device buffer for the two sponge tables; the fixed profiles go into bufferprofs_g
        template<class Upload> void prepare_device(TF* sigma_device, Upload upload)
        {
            if (!swbuffer) return;
            auto& gd = grid.get_grid_data();
            std::vector<TF> sg(2*gd.kcells);
            mhh_grid gh = grid.abi(true);
            mhh_check(mhh_buffer_sigma_host(&gh, zstart, sigma, beta, 0, sg.data()));
            mhh_check(mhh_buffer_sigma_host(&gh, zstart, sigma, beta, 1, sg.data() + gd.kcells));
            upload(sigma_device, sg.data(), sg.size()*sizeof(TF));
            sigma_g = sigma_device; sigmah_g = sigma_device + gd.kcells;
        }
        void clear_device() { sigma_g = sigmah_g = nullptr; }
        mhh_buffer_params params() const
        {
            mhh_buffer_params b{};
            if (!swbuffer) return b;
            b.swbuffer = 1; b.bufferkstart = bufferkstart; b.bufferkstarth = bufferkstarth; b.sigma = sigma_g; b.sigmah = sigmah_g;
            auto prof = [&](const std::string& nm, const Field3d<TF>& f) -> const void* {
                if (swupdate) return f.fld_mean_g;
                auto it = bufferprofs_g.find(nm); return it == bufferprofs_g.end() ? nullptr : it->second; };
            b.abuf_u = prof("u", *fields.mp.at("u")); b.abuf_v = prof("v", *fields.mp.at("v")); b.abuf_w = prof("w", *fields.mp.at("w"));
            int n = 0;
            for (auto& it : fields.sp) b.abuf_s[n++] = prof(it.first, *it.second);
            return b;
        }
        void exec(Stats&, void* stream = nullptr)
        {
            if (!swbuffer) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields); mhh_buffer_params b = params();
            mhh_check(mhh_buffer_exec(&g, &f, &b, stream));
        }
        std::map<std::string, TF*> bufferprofs_g;
        int get_bufferkstart() const { return bufferkstart; }
        int get_bufferkstarth() const { return bufferkstarth; }
    private:
        Grid<TF>& grid; Fields<TF>& fields; TF zstart, sigma, beta; int bufferkstart, bufferkstarth; bool swbuffer, swupdate; TF* sigma_g; TF* sigmah_g;
};

// ---- Force (include/force.h:52-140; src/force.cxx) ------------------------------------------------------------------------------
enum class Large_scale_pressure_type {Disabled, Fixed_flux, Geo_wind, Pressure_gradient};
enum class Large_scale_subsidence_type {Disabled, Mean_field, Local_field};
template<typename TF>
class Force
{
    public:
        Force(Grid<TF>& gridin, Fields<TF>& fieldsin) : swlspres(Large_scale_pressure_type::Disabled), swwls(Large_scale_subsidence_type::Disabled),
            grid(gridin), fields(fieldsin), field3d_operators(gridin, fieldsin) {}
        Large_scale_pressure_type swlspres; Large_scale_subsidence_type swwls; bool swls = false, swnudge = false, swwls_mom = false;
        int swspatialorder = 2;                      // grid.get_spatial_order()
        TF uflux = 0, dpdx = 0, fc = 0, utrans = 0, vtrans = 0;
        TF* ug_g = nullptr; TF* vg_g = nullptr; TF* wls_g = nullptr; TF* nudge_factor_g = nullptr;
        std::vector<std::string> lslist, nudgelist, scalednudgelist;
        std::map<std::string, TF*> lsprofs_g, nudgeprofs_g;
        Large_scale_pressure_type get_switch_lspres() { return swlspres; }
        // device scratch for the two volume sums of the fixed flux: scratch_elems(2) + 2 doubles
        unsigned long long scratch_elems() const { return field3d_operators.scratch_elems(2) + 2; }
        void set_reduce_workspace(double* device_scratch) { work = device_scratch; field3d_operators.set_scratch(device_scratch + 2); }
        mhh_force_params params(double dt) const
        {
            if (swnudge && !scalednudgelist.empty()) throw std::runtime_error("scalednudgelist: rescale the host profile before the upload");
            mhh_force_params p{};
            auto put = [&](const std::string& nm, const void* prof, const void*& u, const void*& v, const void** s) {
                if (nm == "u") u = prof; else if (nm == "v") v = prof;
                else { const int n = scalar_index(fields, nm); if (n < 0) throw std::runtime_error("force: \"" + nm + "\" is not u, v or a prognostic scalar"); s[n] = prof; } };
            if (swlspres == Large_scale_pressure_type::Fixed_flux) { p.swlspres = MHH_LSPRES_UFLUX; p.uflux = uflux; p.dt = dt; p.utrans = utrans; p.uflux_sums = work; }
            else if (swlspres == Large_scale_pressure_type::Pressure_gradient) { p.swlspres = MHH_LSPRES_DPDX; p.dpdx = dpdx; }
            else if (swlspres == Large_scale_pressure_type::Geo_wind)
            { p.swlspres = MHH_LSPRES_GEO; p.order = swspatialorder; p.fc = fc; p.utrans = utrans; p.vtrans = vtrans; p.ug = ug_g; p.vg = vg_g; }
            if (swls) { p.swls = 1; for (auto& nm : lslist) put(nm, lsprofs_g.at(nm), p.ls_u, p.ls_v, p.ls_s); }
            if (swwls != Large_scale_subsidence_type::Disabled)
            { p.swwls = (swwls == Large_scale_subsidence_type::Mean_field) ? MHH_WLS_MEAN : MHH_WLS_LOCAL; p.swwls_mom = swwls_mom; p.wls = wls_g; }
            p.mean_u = fields.mp.at("u")->fld_mean_g; p.mean_v = fields.mp.at("v")->fld_mean_g;
            int n = 0;
            for (auto& it : fields.sp) p.mean_s[n++] = it.second->fld_mean_g;
            if (swnudge) { p.swnudge = 1; p.nudge_factor = nudge_factor_g; for (auto& nm : nudgelist) put(nm, nudgeprofs_g.at(nm), p.nudge_u, p.nudge_v, p.nudge_s); }
            return p;
        }
        // the two volume sums of the fixed flux, left on the device for the pass
        void calc_fixed_flux_sums(void* stream)
        {
            if (swlspres != Large_scale_pressure_type::Fixed_flux) return;
            if (!work) throw std::runtime_error("Force::exec before set_reduce_workspace");
            const TF* uu[2] = {fields.mp.at("u")->fld_g, fields.mt.at("u")->fld_g};
            field3d_operators.calc_sums_g(work, uu, 2, stream);
        }
        void exec(double dt, Thermo<TF>&, Stats&, void* stream = nullptr)
        {
            calc_fixed_flux_sums(stream);
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields); mhh_force_params p = params(dt);
            mhh_check(mhh_force_exec(&g, &f, &p, stream));
        }
        // buffer->exec and force->exec (src/model.cxx:395,404) as one pass over the tendencies: the same bits
        void exec_with_buffer(Buffer<TF>& buffer, double dt, Thermo<TF>&, Stats&, void* stream = nullptr)
        {
            calc_fixed_flux_sums(stream);
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields); mhh_force_params p = params(dt); mhh_buffer_params b = buffer.params();
            mhh_check(mhh_buffer_force_exec(&g, &f, &b, &p, stream));
        }
    private:
        Grid<TF>& grid; Fields<TF>& fields; Field3d_operators<TF> field3d_operators; double* work = nullptr;
};

// ---- Boundary_surface (include/boundary_surface.h; src/boundary_surface.cxx) -----------------------------------------------------
// The Monin-Obukhov surface layer with the lookup solver. It IS the Boundary the Diff classes read: dudz_g, dvdz_g, dbdz_g, z0m_g
// are its outputs. Device arrays are the caller's ([ijcells] each; nobuk int, the tables float[MHH_SURFACE_NZL]); the host
// fills travel through upload(dst_device, src_host, bytes), the caller's H2D copy, as in Diff::prepare_device.
template<typename TF>
class Boundary_surface : public Boundary<TF>
{
    public:
        Boundary_surface(Grid<TF>& gridin, Fields<TF>& fieldsin) : grid(gridin), fields(fieldsin) { this->swboundary = "surface"; }
        // [boundary]: mbcbot (noslip = MHH_BC_DIRICHLET | ustar = MHH_BC_USTAR), ubot, vbot, ustar, z0m, z0h, sbcbot / sbot per scalar
        int mbcbot = MHH_BC_DIRICHLET; TF ubot = 0, vbot = 0, ustarin = 0, z0m_hom = TF(0.1), z0h_hom = TF(0.1), utrans = 0, vtrans = 0;
        bool sw_constant_z0 = true, sw_charnock = false;
        TF thref_kstart = 300, threfh_kstart = 300;      // bs.thref[kstart], bs.threfh[kstart] of Thermo_dry (host values)
        std::map<std::string, int> sbcbot; std::map<std::string, TF> sbot;
        TF* obuk_g = nullptr; TF* ustar_g = nullptr; TF* z0h_g = nullptr; TF* dutot_g = nullptr; int* nobuk_g = nullptr;
        float* zL_sl_g = nullptr; float* f_sl_g = nullptr;
        // what the library refuses is refused here, before anything is uploaded
        void init()
        {
            auto& gd = grid.get_grid_data();
            if (!sw_constant_z0) throw std::runtime_error("Boundary_surface: swconstantz0 = false (the iterative solvers) is not built");
            if (sw_charnock) throw std::runtime_error("Boundary_surface: swcharnock is not built");
            if (gd.igc < 2 || gd.jgc < 2) throw std::runtime_error("Boundary_surface: needs igc >= 2 and jgc >= 2 (calc_dutot reads u[i+2], v[j+2])");
        }
        // src/boundary_surface.cxx:537-574: obuk = dsmall, ustar = 1e-2, nobuk = 0, uniform z0m / z0h
        template<class Upload> void init_surface(Upload upload)
        {
            const size_t n = grid.get_grid_data().ijcells;
            fill(upload, obuk_g, n, TF(1.e-9)); fill(upload, ustar_g, n, TF(1e-2));
            fill(upload, this->z0m_g, n, z0m_hom); fill(upload, z0h_g, n, z0h_hom);
            std::vector<int> zero(n, 0);
            upload(nobuk_g, zero.data(), n*sizeof(int));
        }
        // :748-779: the surface values of u and v (Dirichlet whatever mbcbot says), set_bc of every scalar, set_ustar, init_solver
        template<class Upload> void set_values(Thermo<TF>& thermo, Upload upload)
        {
            const size_t n = grid.get_grid_data().ijcells;
            fill(upload, fields.mp.at("u")->fld_bot_g, n, ubot - utrans); fill(upload, fields.mp.at("v")->fld_bot_g, n, vbot - vtrans);
            for (auto& it : fields.sp)
            {
                const int bc = sbcbot.at(it.first); const TF val = sbot.at(it.first);
                if (bc == MHH_BC_DIRICHLET) fill(upload, it.second->fld_bot_g, n, val);
                else if (bc == MHH_BC_NEUMANN) fill(upload, it.second->grad_bot_g, n, val);
                else if (bc == MHH_BC_FLUX) fill(upload, it.second->flux_bot_g, n, val);
            }
            if (mbcbot == MHH_BC_USTAR) set_ustar(upload);
            init_solver(thermo, upload);
        }
        // :781-809: ustar limited at 1e-4
        template<class Upload> void set_ustar(Upload upload) { fill(upload, ustar_g, grid.get_grid_data().ijcells, std::max(static_cast<TF>(0.0001), ustarin)); }
        // :812-826: the table on the host with the host C library
        template<class Upload> void init_solver(Thermo<TF>& thermo, Upload upload)
        {
            auto& gd = grid.get_grid_data();
            std::vector<float> zL(MHH_SURFACE_NZL), f(MHH_SURFACE_NZL);
            mhh_check(mhh_surface_lut_host(gd.z[gd.kstart], z0m_hom, z0h_hom, mbcbot, thermobc(thermo), mhh_dtype<TF>(), zL.data(), f.data()));
            upload(zL_sl_g, zL.data(), zL.size()*sizeof(float)); upload(f_sl_g, f.data(), f.size()*sizeof(float));
        }
        mhh_surface_params params(Thermo<TF>& thermo) const
        {
            mhh_surface_params p{};
            p.mbcbot = mbcbot; p.swconstantz0 = sw_constant_z0; p.swcharnock = sw_charnock;
            const std::string sw = thermo.get_switch();
            p.thermo_kind = (sw == "dry") ? MHH_THERMO_DRY : (sw == "buoy") ? MHH_THERMO_BUOY : MHH_THERMO_NONE;
            if (p.thermo_kind) { p.thermo_index = scalar_index(fields, sw == "dry" ? thermo.th : thermo.b); p.thermobc = thermobc(thermo); }
            if (p.thermo_kind == MHH_THERMO_DRY) { p.thref_kstart = thref_kstart; p.threfh_kstart = threfh_kstart; }
            p.grav = thermo.grav; p.bg_n2 = thermo.n2;
            p.zL = zL_sl_g; p.f = f_sl_g; p.z0m = this->z0m_g; p.z0h = z0h_g; p.ustar = ustar_g; p.obuk = obuk_g; p.nobuk = nobuk_g;
            p.ubot = fields.mp.at("u")->fld_bot_g; p.vbot = fields.mp.at("v")->fld_bot_g;
            p.ugradbot = fields.mp.at("u")->grad_bot_g; p.vgradbot = fields.mp.at("v")->grad_bot_g;
            int n = 0;
            for (auto& it : fields.sp) { p.sbot[n] = it.second->fld_bot_g; p.sgradbot[n] = it.second->grad_bot_g; p.sbcbot[n] = sbcbot.at(it.first); ++n; }
            return p;
        }
        // :830-983 on one rank: three kernels and three 2-D cyclic fills
        void exec(Thermo<TF>& thermo, void* stream = nullptr)
        {
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, this); mhh_surface_params p = params(thermo);
            mhh_check(mhh_boundary_surface_exec(&g, &f, &p, dutot_g, stream));
        }
        // the same on a slab: the stages, with halo2d(TF*) -- the caller's east-west wrap and north-south exchange of a 2-D array --
        // where the reference calls boundary_cyclic.exec_2d. nobuk is per rank and never exchanged.
        template<class Halo2d> void exec_slab(Thermo<TF>& thermo, Halo2d halo2d, void* stream = nullptr)
        {
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields, this); mhh_surface_params p = params(thermo);
            mhh_check(mhh_surface_dutot(&g, &f, &p, dutot_g, stream));
            halo2d(dutot_g);
            mhh_check(mhh_surface_stability(&g, &f, &p, dutot_g, stream));
            mhh_check(mhh_surface_momentum(&g, &f, &p, stream));
            halo2d(fields.mp.at("u")->flux_bot_g); halo2d(fields.mp.at("v")->flux_bot_g);
            for (int n=0; n<f.nscalars; ++n) mhh_check(mhh_surface_scalar(&g, &f, &p, n, stream));
            mhh_check(mhh_surface_mo_gradients(&g, &f, &p, stream));
        }
    private:
        int thermobc(Thermo<TF>& thermo) const
        {
            const std::string sw = thermo.get_switch();
            if (sw != "dry" && sw != "buoy") return MHH_BC_DIRICHLET;
            return sbcbot.at(sw == "dry" ? thermo.th : thermo.b);
        }
        template<class Upload> static void fill(Upload upload, TF* dst, size_t n, TF v)
        {
            if (!dst) throw std::runtime_error("Boundary_surface: a device array is missing");
            std::vector<TF> h(n, v);
            upload(dst, h.data(), n*sizeof(TF));
        }
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Thermo_moist (src/thermo_moist.cxx): swthermo = moist with the scalars thl and qt, second order ---------------------------
// The base-state tables and the counter are the caller's device arrays ([kcells] of TF; nonconv_g one int, zeroed), as the other
// classes here take theirs. `upload(dst_device, src_host, bytes)` is the caller's copy (create_basestate runs once, outside a step).
template<typename TF>
class Thermo_moist
{
    public:
        Thermo_moist(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        // [thermo] pbot, swbasestate ("anelastic" | "boussinesq"), thvref0, swupdatebasestate
        TF pbot = 0; std::string swbasestate = "anelastic"; TF thvref0 = 0; bool swupdatebasestate = true;
        std::string thl = "thl", qt = "qt";
        TF* pref_g = nullptr; TF* prefh_g = nullptr; TF* rhoref_g = nullptr; TF* rhorefh_g = nullptr;
        TF* thvref_g = nullptr; TF* thvrefh_g = nullptr; TF* exnref_g = nullptr; TF* exnrefh_g = nullptr;
        int* nonconv_g = nullptr;
        std::vector<TF> thl0, qt0, pref, prefh, rhoref, rhorefh, thvref, thvrefh, exnref, exnrefh;      // host copies of the creation-time state
        std::string get_switch() const { return "moist"; }

        // Thermo_moist::create_basestate (:1189-1247): thl0_in, qt0_in are the ktot initial values; the tables on the host with the
        // host's C library, uploaded; fields.rhoref / rhorefh set once (never updated)
        template<class Upload> void create_basestate(const std::vector<TF>& thl0_in, const std::vector<TF>& qt0_in, Upload&& upload)
        {
            const auto& gd = grid.get_grid_data();
            if (swbasestate != "anelastic" && swbasestate != "boussinesq") throw std::runtime_error("Invalid option for \"swbasestate\"");
            if ((int)thl0_in.size() != gd.ktot || (int)qt0_in.size() != gd.ktot) throw std::runtime_error("create_basestate: ktot values of thl and qt");
            if (!(pref_g && prefh_g && rhoref_g && rhorefh_g && thvref_g && thvrefh_g && exnref_g && exnrefh_g)) throw std::runtime_error("create_basestate: the eight device tables");
            const size_t nk = gd.kcells;
            thl0.assign(nk, 0); qt0.assign(nk, 0);
            for (int k=0; k<gd.ktot; ++k) { thl0[gd.kstart+k] = thl0_in[k]; qt0[gd.kstart+k] = qt0_in[k]; }
            for (std::vector<TF>* v : {&pref, &prefh, &rhoref, &rhorefh, &thvref, &thvrefh, &exnref, &exnrefh}) v->assign(nk, 0);
            mhh_grid g = grid.abi(true);
            int nonconv = 0;
            mhh_check(mhh_thermo_moist_base_state_host(&g, thl0.data(), qt0.data(), pbot, swbasestate == "boussinesq" ? 1 : 0, thvref0,
                                                       pref.data(), prefh.data(), rhoref.data(), rhorefh.data(), thvref.data(), thvrefh.data(),
                                                       exnref.data(), exnrefh.data(), &nonconv));
            if (nonconv) throw std::runtime_error("Non-converging saturation adjustment in the base state");
            TF* dst[8] = {pref_g, prefh_g, rhoref_g, rhorefh_g, thvref_g, thvrefh_g, exnref_g, exnrefh_g};
            const std::vector<TF>* src[8] = {&pref, &prefh, &rhoref, &rhorefh, &thvref, &thvrefh, &exnref, &exnrefh};
            for (int n=0; n<8; ++n) upload(dst[n], src[n]->data(), nk*sizeof(TF));
            fields.rhoref = rhoref; fields.rhorefh = rhorefh;
            if (fields.rhoref_g && fields.rhorefh_g) { upload(fields.rhoref_g, rhoref.data(), nk*sizeof(TF)); upload(fields.rhorefh_g, rhorefh.data(), nk*sizeof(TF)); }
        }
        // Thermo_moist::exec (:1273-1303): with swupdatebasestate the base state from fld_mean_g of thl and qt (Field3d_operators'
        // calc_mean_profile, the caller's), all eight profiles on the device; then the buoyancy tendency of w
        void exec(void* stream = nullptr)
        {
            const auto& gd = grid.get_grid_data();
            if (gd.kgc < 1) throw std::runtime_error("Thermo_moist: one vertical ghost cell");
            mhh_grid g = grid.abi();
            auto& a = *fields.sp.at(thl); auto& q = *fields.sp.at(qt);
            if (swupdatebasestate)
            {
                if (!a.fld_mean_g || !q.fld_mean_g) throw std::runtime_error("Thermo_moist::exec: fld_mean_g of thl and qt (swupdatebasestate)");
                mhh_check(mhh_thermo_moist_base_state(&g, a.fld_mean_g, q.fld_mean_g, pbot, pref_g, prefh_g, rhoref_g, rhorefh_g, thvref_g, thvrefh_g,
                                                      exnref_g, exnrefh_g, nonconv_g, stream));
            }
            mhh_check(mhh_thermo_moist_buoyancy_tend(&g, fields.mt.at("w")->fld_g, a.fld_g, q.fld_g, prefh_g, exnrefh_g, thvrefh_g, nonconv_g, stream));
        }
        // Thermo_moist::get_thermo_field_g (:1418-1500) for b | ql | qi | T | N2 into a caller-owned 3-D device field; with
        // swupdatebasestate the pressure and Exner profiles are refreshed from the means first. Any other name is refused.
        void get_thermo_field(TF* out, const std::string& name, void* stream = nullptr)
        {
            if (name != "b" && name != "ql" && name != "qi" && name != "T" && name != "N2")
                throw std::runtime_error("get_thermo_field: \"" + name + "\" is not built (b | ql | qi | T | N2)");
            mhh_grid g = grid.abi();
            auto& a = *fields.sp.at(thl); auto& q = *fields.sp.at(qt);
            if (swupdatebasestate && a.fld_mean_g && q.fld_mean_g)
                mhh_check(mhh_thermo_moist_base_state(&g, a.fld_mean_g, q.fld_mean_g, pbot, pref_g, prefh_g, nullptr, nullptr, nullptr, nullptr,
                                                      exnref_g, exnrefh_g, nonconv_g, stream));
            if (name == "N2") { mhh_check(mhh_calc_N2(&g, out, a.fld_g, thvref_g, 9.81, stream)); return; }       // calc_N2 (:460-475)
            mhh_check(mhh_thermo_moist_fields(&g, a.fld_g, q.fld_g, pref_g, exnref_g, thvref_g, name == "b" ? out : nullptr, name == "ql" ? out : nullptr,
                                              name == "qi" ? out : nullptr, name == "T" ? out : nullptr, nonconv_g, stream));
        }
        // get_buoyancy_surf, get_buoyancy_fluxbot, get_db_ref (:1610-1717) are evaluated inside the surface layer's kernels from the
        // device tables: these three name what they set in its parameter block (thermo_kind 3; thl_index, qt_index = the scalars)
        void get_buoyancy_surf(mhh_surface_params& p, int thl_index, int qt_index) const
        { p.thermo_kind = MHH_THERMO_MOIST; p.thermo_index = thl_index; p.qt_index = qt_index; p.thvref = thvref_g; p.thvrefh = thvrefh_g; }
        void get_buoyancy_fluxbot(mhh_surface_params& p, int thl_index, int qt_index) const { get_buoyancy_surf(p, thl_index, qt_index); }
        // the creation-time value (the kernels evaluate the current one from the tables)
        TF get_db_ref() const { const int ks = grid.get_grid_data().kstart; return TF(9.81)/thvref[ks]*(thvref[ks] - thvrefh[ks]); }
        // get_basestate_vector: the device table by name
        TF* get_basestate_vector(const std::string& name) const
        {
            if (name == "pref") return pref_g; if (name == "prefh") return prefh_g; if (name == "rhoref") return rhoref_g; if (name == "rhorefh") return rhorefh_g;
            if (name == "thvref") return thvref_g; if (name == "thvrefh") return thvrefh_g; if (name == "exnref") return exnref_g; if (name == "exnrefh") return exnrefh_g;
            throw std::runtime_error("get_basestate_vector: " + name);
        }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Microphys_2mom_warm (src/microphys_2mom_warm.cxx): swmicro = 2mom_warm with the scalars thl, qt, qr and nr ------------------
// rr_bot_g ([ijcells]), the four scratch fields ([ncells] each: the reference's get_tmp_g) and work_g (mhh_reduce_work_bytes()) are
// the caller's device arrays. The base state, rhoref included, comes from the Thermo_moist it is handed, as the reference's exec
// takes its thermo.
template<typename TF>
class Microphys_2mom_warm
{
    public:
        Microphys_2mom_warm(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        // [micro] Nc0, cflmax
        TF Nc0 = 0; TF cflmax = 2.;
        int processes = MHH_MICRO_ALL;
        TF* rr_bot_g = nullptr; TF* scratch_g[4] = {nullptr, nullptr, nullptr, nullptr}; void* work_g = nullptr;
        std::string get_switch() const { return "2mom_warm"; }

        // Microphys_2mom_warm::exec (:639-752); dt is the full step, timeloop->get_dt()
        void exec(Thermo_moist<TF>& thermo, const double dt, void* stream = nullptr)
        {
            if (!(Nc0 > 0)) throw std::runtime_error("Microphys_2mom_warm: Nc0 (no default)");
            mhh_grid g = grid.abi();
            mhh_micro_params p{}; p.Nc0 = Nc0; p.dt = dt; p.processes = processes;
            void* const scratch[4] = {scratch_g[0], scratch_g[1], scratch_g[2], scratch_g[3]};
            mhh_check(mhh_micro_2mom_warm_exec(&g, &p, fields.sp.at("qr")->fld_g, fields.sp.at("nr")->fld_g, fields.sp.at("thl")->fld_g, fields.sp.at("qt")->fld_g,
                                               fields.st.at("qr")->fld_g, fields.st.at("nr")->fld_g, fields.st.at("thl")->fld_g, fields.st.at("qt")->fld_g, rr_bot_g,
                                               fields.rhoref_g, thermo.pref_g, thermo.exnref_g, scratch, thermo.nonconv_g, stream));
        }
        // get_time_limit (:965-982): idt * cflmax / cfl in TF, truncated. `max_over_ranks` is Master::max (the identity on one rank).
        template<class Max> unsigned long get_time_limit(unsigned long idt, const double dt, Max&& max_over_ranks, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            double out = 0;
            mhh_check(mhh_micro_2mom_warm_cfl(&g, fields.sp.at("qr")->fld_g, fields.sp.at("nr")->fld_g, fields.rhoref_g, dt, work_g, &out, stream));
            TF cfl = TF(out);
            max_over_ranks(&cfl);
            return idt * cflmax / cfl;
        }
        unsigned long get_time_limit(unsigned long idt, const double dt) { return get_time_limit(idt, dt, [](TF*) {}); }
        // get_surface_rain_rate: the device array exec wrote
        TF* get_surface_rain_rate() const { return rr_bot_g; }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Microphys_nsw6 (src/microphys_nsw6.cxx): swmicro = nsw6 with the scalars thl, qt, qr, qs and qg ---------------------------
// The three surface rates ([ijcells] each), the six scratch fields ([ncells] each: the reference's get_tmp_g, two per species) and
// work_g (mhh_reduce_work_bytes()) are the caller's device arrays. ql and qi are the saturation adjustment of the Thermo_moist it
// is handed, evaluated per cell inside the conversion kernel; the base state, rhoref included, comes from it too.
template<typename TF>
class Microphys_nsw6
{
    public:
        Microphys_nsw6(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        // [micro] Nc0, cflmax
        TF Nc0 = 0; TF cflmax = 1.2;
        int processes = MHH_NSW6_ALL;
        int impl = MHH_NSW6_IMPL_DEFAULT;
        TF* rr_bot_g = nullptr; TF* rs_bot_g = nullptr; TF* rg_bot_g = nullptr;
        TF* scratch_g[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; void* work_g = nullptr;
        std::string get_switch() const { return "nsw6"; }

        // Microphys_nsw6::exec (:983-1073); dt is the full step, timeloop->get_dt()
        void exec(Thermo_moist<TF>& thermo, const double dt, void* stream = nullptr)
        {
            if (!(Nc0 > 0)) throw std::runtime_error("Microphys_nsw6: Nc0 (no default)");
            mhh_grid g = grid.abi();
            mhh_micro_params p{}; p.Nc0 = Nc0; p.dt = dt; p.processes = processes;
            void* const scratch[6] = {scratch_g[0], scratch_g[1], scratch_g[2], scratch_g[3], scratch_g[4], scratch_g[5]};
            mhh_check(mhh_micro_nsw6_exec_impl(&g, impl, &p, fields.sp.at("qr")->fld_g, fields.sp.at("qs")->fld_g, fields.sp.at("qg")->fld_g,
                                               fields.sp.at("thl")->fld_g, fields.sp.at("qt")->fld_g, nullptr, nullptr,
                                               fields.st.at("qr")->fld_g, fields.st.at("qs")->fld_g, fields.st.at("qg")->fld_g,
                                               fields.st.at("thl")->fld_g, fields.st.at("qt")->fld_g, rr_bot_g, rs_bot_g, rg_bot_g,
                                               fields.rhoref_g, thermo.pref_g, thermo.exnref_g, scratch, thermo.nonconv_g, stream));
        }
        // get_time_limit (:1119-1177): the CFL number is a double there, idt * cflmax a TF. `max_over_ranks` is Master::max (the
        // identity on one rank).
        template<class Max> unsigned long get_time_limit(unsigned long idt, const double dt, Max&& max_over_ranks, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            double cfl = 0;
            mhh_check(mhh_micro_nsw6_cfl_impl(&g, impl, fields.sp.at("qr")->fld_g, fields.sp.at("qs")->fld_g, fields.sp.at("qg")->fld_g, fields.rhoref_g, dt,
                                              work_g, &cfl, stream));
            max_over_ranks(&cfl);
            return idt * cflmax / cfl;
        }
        unsigned long get_time_limit(unsigned long idt, const double dt) { return get_time_limit(idt, dt, [](double*) {}); }
        // the device arrays exec wrote; get_surface_rain_rate (:1194-1202) is their sum, the caller's to form
        TF* get_surface_rain_rate() const { return rr_bot_g; }
        TF* get_surface_snow_rate() const { return rs_bot_g; }
        TF* get_surface_graupel_rate() const { return rg_bot_g; }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Limiter (src/limiter.cxx): [limiter] limitlist ----------------------------------------------------------------------------
template<typename TF>
class Limiter
{
    public:
        Limiter(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        std::vector<std::string> limit_list;
        // Limiter::exec (:78-94) with the sub-step dt
        void exec(const double dt, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            for (const std::string& name : limit_list)
                mhh_check(mhh_limiter_exec(&g, fields.st.at(name)->fld_g, fields.sp.at(name)->fld_g, dt, stream));
        }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Radiation_gcss (src/radiation_gcss.cxx): swradiation = gcss, the CPU path's physics ---------------------------------------
// The two scratch fields ([ncells] each: the reference's get_tmp_g; its CPU path takes four) are the caller's device arrays. ql is
// the saturation adjustment of the Thermo_moist it is handed, as the reference's exec takes its thermo. day_of_year is
// Timeloop::calc_day_of_year(); the zenith angle is a host number, so a captured step keeps the one it was captured with.
template<typename TF>
class Radiation_gcss
{
    public:
        Radiation_gcss(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        // [radiation] xka, fr0, fr1, div (no defaults in the reference)
        TF xka = 0, fr0 = 0, fr1 = 0, div = 0;
        const TF mu_min = 0.035;
        const std::string tend_name = "rad";
        int parts = MHH_RAD_LW | MHH_RAD_SW;
        TF* scratch_g[2] = {nullptr, nullptr};
        std::string get_switch() const { return "gcss"; }
        unsigned long get_time_limit(unsigned long) const { return ~0ul; }            // Constants::ulhuge (:345-349)
        bool check_field_exists(const std::string& name) const { return name == "rflx" || name == "sflx"; }      // (:383-389, as written)

        // calc_zenith (:39-76) at grid.lat, grid.lon
        TF calc_zenith(const double day_of_year) const
        {
            double mu = 0;
            const auto& gd = grid.get_grid_data();
            mhh_check(mhh_radiation_gcss_zenith_host(mhh_dtype<TF>(), gd.lat, gd.lon, day_of_year, &mu));
            return TF(mu);
        }
        // Radiation_gcss::exec (:353-379)
        void exec(Thermo_moist<TF>& thermo, const double day_of_year, void* stream = nullptr)
        {
            call(thermo, day_of_year, fields.st.at("thl")->fld_g, nullptr, nullptr, stream);
        }
        // get_radiation_field (:392-436) into a caller-owned 3-D device field: lflx | sflx, other names are refused
        void get_radiation_field(TF* fld, const std::string& name, Thermo_moist<TF>& thermo, const double day_of_year, void* stream = nullptr)
        {
            if (name != "lflx" && name != "sflx")
                throw std::runtime_error("get_radiation_field: \"" + name + "\" is not built (lflx | sflx)");
            call(thermo, day_of_year, nullptr, name == "lflx" ? fld : nullptr, name == "sflx" ? fld : nullptr, stream);
        }
    private:
        void call(Thermo_moist<TF>& thermo, const double day_of_year, TF* thlt, TF* lflx, TF* sflx, void* stream)
        {
            mhh_grid g = grid.abi();
            mhh_radiation_gcss_params p{}; p.xka = xka; p.fr0 = fr0; p.fr1 = fr1; p.div = div; p.mu = calc_zenith(day_of_year); p.parts = parts;
            void* const scratch[2] = {scratch_g[0], scratch_g[1]};
            mhh_check(mhh_radiation_gcss_exec(&g, &p, thlt, nullptr, fields.sp.at("thl")->fld_g, fields.sp.at("qt")->fld_g, fields.rhoref_g,
                                              thermo.pref_g, thermo.exnref_g, lflx, sflx, scratch, thermo.nonconv_g, stream));
        }
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Stats (src/stats.cxx): the sampling of second-order cases on the device ----------------------------------------------------
// The reference's call surface as far as it is built: add_mask, add_profs, add_time_series, add_tendency, initialize_masks,
// set_mask_thres, finalize_masks, calc_stats, calc_tend, calc_stats_2d; get_prof and get_time_series are accessors in place of the
// NetCDF writer and return DEVICE pointers (a profile of kcells, one value). The host Field3d carries no location, so add_profs takes
// the zloc of the reference ("z" | "zh") and calc_stats finds it by name. The device memory is the caller's, as everywhere in this
// header (the reference's own vectors and tmp fields): mfield_g [ncells] and mfield_bot_g [ijcells] words, zero2d_g [ijcells] zeros,
// nmask_g [nmask_elems()] ints, work_g [work_elems()] doubles, prof_g [prof_elems()] of TF, sized once every mask, profile and
// series is registered. Operations: "mean", "2", "3", "4", "frac", "grad", "path", "cover", and the fluxes "w", "diff", "flux" of a
// full-level variable (set flux_of(name) and the schemes first; the variable "w" must be registered with its mean, and its
// calc_stats come first, as Fields::exec_stats has it). A slab rank (npy > 1) sets sum_ranks, the sum over the ranks of n device
// doubles (Master::sum): it runs between every sums call and its finish call; without it a slab grid is refused.
// (`Stats` itself is this header's placeholder that the operators' create() and exec() take: the class is Stats_sampler<TF>.)
enum class Stats_mask_type { Plus, Min };
template<typename TF>
class Stats_sampler
{
    public:
        Stats_sampler(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        unsigned int* mfield_g = nullptr; unsigned int* mfield_bot_g = nullptr;
        TF* zero2d_g = nullptr; int* nmask_g = nullptr; double* work_g = nullptr; TF* prof_g = nullptr;
        std::function<void(double*, size_t)> sum_ranks;              // the sum over the ranks, in place, of device doubles
        // what the fluxes need beyond the field: the schemes (MHH_ADVEC_2 | _2I5, MHH_DIFF_2 | _SMAG2), boundary.get_switch() !=
        // "default", diff.tPr, and per variable where it lives (0 scalar, 1 u, 2 v), its visc, whether advec.fluxlimit_list holds it
        int swadvec = MHH_ADVEC_2I5, swdiff = MHH_DIFF_SMAG2; bool surface_model = true; TF tPr = TF(1./3.);
        struct Flux_info { int kind = 0; TF visc = 0; bool limit = false; };
        Flux_info& flux_of(const std::string& name) { return flux_info[name]; }

        void add_mask(const std::string& name)                       // (:841-850): flag = 1 << 2n, flagh = 1 << (2n+1)
        {
            if (masks.size() >= MHH_STATS_MAX_MASKS) throw std::runtime_error("Stats: at most MHH_STATS_MAX_MASKS masks");
            masks.push_back(name);
        }
        void add_profs(const std::string& name, const std::string& zloc, const std::vector<std::string>& operations)   // (:853-911)
        {
            if (zloc != "z" && zloc != "zh") throw std::runtime_error("Stats: zloc is \"z\" or \"zh\"");
            Var v; v.loc = (zloc == "zh");
            auto has = [&](const char* op) { for (auto& o : operations) if (o == op) return true; return false; };
            for (auto& o : operations)
                if (o != "mean" && o != "2" && o != "3" && o != "4" && o != "frac" && o != "grad" && o != "path" && o != "cover" && o != "w" && o != "diff" && o != "flux")
                    throw std::runtime_error("Stats: unknown operation \"" + o + "\"");
            if (has("w") || has("diff") || has("flux"))
            {
                if (v.loc) throw std::runtime_error("Stats: the flux of a half-level variable cannot be delivered at that location");
                if (!has("mean") || (has("flux") && !(has("w") && has("diff")))) throw std::runtime_error("Stats: a flux needs the mean; _flux needs _w and _diff");
            }
            if ((has("2") || has("3") || has("4")) && !has("mean")) throw std::runtime_error("Stats: a moment needs the mean of its variable");
            if (has("mean")) { v.mean = nslots; slot[name] = nslots++; }
            v.first_b = nslots;                                   // pass B: one slot per operation, contiguous, in the order given
            for (auto& o : operations)
                if (o == "2" || o == "3" || o == "4" || o == "frac" || o == "grad")
                {
                    v.ops_b.push_back(o == "2" ? MHH_STATS_MOMENT2 : o == "3" ? MHH_STATS_MOMENT3 : o == "4" ? MHH_STATS_MOMENT4 : o == "frac" ? MHH_STATS_FRAC : MHH_STATS_GRAD);
                    slot[name + "_" + o] = nslots++;
                }
            if (v.ops_b.size() > MHH_STATS_MAX_JOBS) throw std::runtime_error("Stats: too many operations");
            v.first_f = nslots;                                   // the fluxes: _w, _diff, _flux, contiguous, in that order
            for (const char* o : {"w", "diff", "flux"})
                if (has(o)) { v.ops_f.push_back(o[0] == 'w' ? MHH_STATS_FLUX_W : o[0] == 'd' ? MHH_STATS_FLUX_DIFF : MHH_STATS_FLUX_SUM); slot[name + "_" + o] = nslots++; }
            if (has("path") || has("cover"))
            {
                if (v.loc) throw std::runtime_error("Stats: path and cover are taken of full-level variables");
                v.column = nslots++;                              // cover and path per mask: [nmasks][2] at the head of the slot
                if (has("cover")) series[name + "_cover"] = {v.column, 0};
                if (has("path"))  series[name + "_path"]  = {v.column, 1};
            }
            vars[name] = v;
        }
        void add_time_series(const std::string& name) { series2d[name] = nslots++; }                                    // (:1177-1211)
        void add_tendency(const std::string& var, const std::string& zloc, const std::string& tend_name)                // (:913-927)
        {
            tends[var + "_" + tend_name] = (zloc == "zh"); slot[var + "_" + tend_name] = nslots++;
        }
        size_t nmask_elems() const { return masks.size()*(2*(size_t)grid.gd.kcells + 1); }
        size_t prof_elems() const { return (size_t)(nslots + 2)*masks.size()*grid.gd.kcells; }      // + area, areah
        size_t work_elems() const
        {
            mhh_grid g = grid.abi();
            const size_t nm = masks.size(), kc = grid.gd.kcells;
            return (size_t)mhh_stats_scratch_elems(&g, (int)nm, MHH_STATS_MAX_JOBS) + (MHH_STATS_MAX_JOBS + 2)*nm*kc + 3*nm;
        }

        void initialize_masks(void* stream = nullptr)                // (:1214-1227)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_stats_mask_init(&g, mfield_g, mfield_bot_g, (int)masks.size(), stream));
        }
        // (:1264-1301): fldh's fld_bot is what the reference passes; zeros where the field has none
        void set_mask_thres(const std::string& mask_name, Field3d<TF>& fld, Field3d<TF>& fldh, TF threshold, Stats_mask_type mode, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_stats_mask_thres(&g, mfield_g, mfield_bot_g, mask_index(mask_name), fld.fld_g, fldh.fld_g, fldh.fld_bot_g ? fldh.fld_bot_g : zero2d_g,
                                           threshold, mode == Stats_mask_type::Plus ? MHH_STATS_MASK_PLUS : MHH_STATS_MASK_MIN, stream));
        }
        void finalize_masks(void* stream = nullptr)                  // (:1229-1262)
        {
            mhh_grid g = grid.abi();
            const int nm = (int)masks.size();
            mhh_check(mhh_stats_mask_count(&g, mfield_g, mfield_bot_g, nm, csums(), work_g, stream));
            all_ranks(csums(), 2*(size_t)nm*grid.gd.kcells);
            mhh_check(mhh_stats_mask_finish(&g, nm, csums(), nmask_g, nmask_g + (size_t)nm*2*grid.gd.kcells, prof(nslots), prof(nslots + 1), stream));
        }
        // (:1607-1890): the mean, then what reads it, then the column pass
        void calc_stats(const std::string& varname, const Field3d<TF>& fld, const TF offset, const TF threshold, void* stream = nullptr)
        {
            auto it = vars.find(varname);
            if (it == vars.end()) return;                            // not in the varlist
            const Var& v = it->second;
            if (v.mean >= 0)
            {
                mhh_stats_job j{}; j.fld = fld.fld_g; j.loc = v.loc; j.op = MHH_STATS_MEAN; j.offset = offset; j.threshold = threshold;
                run(&j, 1, prof(v.mean), stream);
            }
            if (!v.ops_b.empty())
            {
                std::vector<mhh_stats_job> jobs(v.ops_b.size());
                for (size_t n=0; n<jobs.size(); ++n)
                {
                    mhh_stats_job& j = jobs[n];
                    j.fld = fld.fld_g; j.loc = v.loc; j.op = v.ops_b[n]; j.offset = offset; j.threshold = threshold;
                    j.mean = (j.op >= MHH_STATS_MOMENT2 && j.op <= MHH_STATS_MOMENT4) ? prof(v.mean) : nullptr;
                }
                run(jobs.data(), (int)jobs.size(), prof(v.first_b), stream);
            }
            if (!v.ops_f.empty())
            {
                auto w = vars.find("w");
                if (w == vars.end() || w->second.mean < 0) throw std::runtime_error("Stats: the resolved flux needs the variable w registered with its mean");
                const Flux_info& fi = flux_info[varname];
                std::vector<mhh_stats_job> jobs(v.ops_f.size());
                for (size_t n=0; n<jobs.size(); ++n)
                {
                    mhh_stats_job& j = jobs[n];
                    j.fld = fld.fld_g; j.loc = v.loc; j.op = v.ops_f[n]; j.offset = offset; j.threshold = threshold; j.mean = prof(v.mean);
                    j.kind = fi.kind; j.w = fields.mp.at("w")->fld_g; j.wmean = prof(w->second.mean);
                    j.scheme = (j.op == MHH_STATS_FLUX_W) ? swadvec : swdiff; j.limit = fi.limit; j.surface_model = surface_model;
                    j.evisc = fields.sd.count("evisc") ? fields.sd.at("evisc")->fld_g : nullptr;
                    j.flux_bot = fld.flux_bot_g; j.flux_top = fld.flux_top_g; j.visc = fi.visc; j.tPr = tPr; j.a = 0; j.b = 1;
                }
                run(jobs.data(), (int)jobs.size(), prof(v.first_f), stream);
            }
            if (v.column >= 0)
            {
                mhh_grid g = grid.abi();
                const int nm = (int)masks.size();
                mhh_check(mhh_stats_columns(&g, mfield_g, nm, fld.fld_g, v.loc, offset, threshold, fields.rhoref_g, colsums(), work_g, stream));
                all_ranks(colsums(), 3*(size_t)nm);
                mhh_check(mhh_stats_columns_finish(&g, nm, colsums(), prof(v.column), stream));
            }
        }
        void calc_tend(Field3d<TF>& fld, const std::string& var, const std::string& tend_name, void* stream = nullptr)   // (:1893-1919)
        {
            auto it = tends.find(var + "_" + tend_name);
            if (it == tends.end()) return;
            mhh_stats_job j{}; j.fld = fld.fld_g; j.loc = it->second; j.op = MHH_STATS_MEAN;
            run(&j, 1, prof(slot.at(it->first)), stream);
        }
        void calc_stats_2d(const std::string& varname, const TF* fld_g, const TF offset, void* stream = nullptr)         // (:1921-1937)
        {
            auto it = series2d.find(varname);
            if (it == series2d.end()) return;
            mhh_stats_job j{}; j.fld = fld_g; j.op = MHH_STATS_MEAN2D; j.offset = offset;
            run(&j, 1, prof(it->second), stream);
        }
        // accessors: DEVICE pointers, valid once the stream has run
        const TF* get_prof(const std::string& mask, const std::string& name) const
        {
            const int m = mask_index(mask);
            const int s = (name == "area") ? nslots : (name == "areah") ? nslots + 1 : slot.at(name);
            return prof(s) + (size_t)m*grid.gd.kcells;
        }
        const TF* get_time_series(const std::string& mask, const std::string& name) const
        {
            const int m = mask_index(mask);
            auto it = series.find(name);
            if (it != series.end()) return prof(it->second.first) + m*2 + it->second.second;
            return prof(series2d.at(name)) + (size_t)m*grid.gd.kcells;
        }
        const int* get_nmask(const std::string& mask, bool half) const { return nmask_g + ((size_t)mask_index(mask)*2 + (half ? 1 : 0))*grid.gd.kcells; }
        const int* get_nmask_bot(const std::string& mask) const { return nmask_g + masks.size()*2*(size_t)grid.gd.kcells + mask_index(mask); }
        const std::vector<std::string>& get_masks() const { return masks; }      // Budget_2_sampler averages under the same masks

    private:
        struct Var { int loc = 0, mean = -1, first_b = 0, first_f = 0, column = -1; std::vector<int> ops_b, ops_f; };
        // the sum over the ranks between a sums call and its finish call; a slab grid without the hook is refused
        void all_ranks(double* d, size_t n)
        {
            if (grid.gd.npy == 1) return;
            if (!sum_ranks) throw std::runtime_error("Stats: a slab rank (npy > 1) needs sum_ranks, the sum over the ranks");
            sum_ranks(d, n);
        }
        std::map<std::string, Flux_info> flux_info;
        int mask_index(const std::string& name) const
        {
            for (size_t n=0; n<masks.size(); ++n) if (masks[n] == name) return (int)n;
            throw std::runtime_error("Invalid mask name in set_mask_thres()");
        }
        TF* prof(int s) const { return prof_g + (size_t)s*masks.size()*grid.gd.kcells; }
        double* sums() const { mhh_grid g = grid.abi(); return work_g + mhh_stats_scratch_elems(&g, (int)masks.size(), MHH_STATS_MAX_JOBS); }
        double* csums() const { return sums() + (size_t)MHH_STATS_MAX_JOBS*masks.size()*grid.gd.kcells; }
        double* colsums() const { return csums() + 2*masks.size()*(size_t)grid.gd.kcells; }
        // sums, the sum over the ranks, the finish
        void run(const mhh_stats_job* jobs, int njobs, TF* out, void* stream)
        {
            mhh_grid g = grid.abi();
            const int nm = (int)masks.size();
            mhh_check(mhh_stats_sums(&g, mfield_g, nm, jobs, njobs, sums(), work_g, stream));
            all_ranks(sums(), (size_t)njobs*nm*grid.gd.kcells);
            mhh_check(mhh_stats_finish(&g, nm, jobs, njobs, sums(), nmask_g, out, stream));
        }
        Grid<TF>& grid; Fields<TF>& fields;
        std::vector<std::string> masks;
        std::map<std::string, Var> vars;
        std::map<std::string, int> slot, series2d;
        std::map<std::string, std::pair<int, int>> series;
        std::map<std::string, bool> tends;
        int nslots = 0;
};

// Budget_2<TF>::exec_stats (src/budget_2.cxx:1414-1818) on the device, under the masks of a Stats_sampler whose finalize_masks has
// run: the model profiles (Stats::calc_mask_mean_profile), bmean and pmean (field3d_operators.calc_mean_profile) and every calc_*
// loop with the calc_mask_stats that follows it, as mhh_budget_2_sums + mhh_budget_2_finish (csrc/budget_2.h). `groups` are the
// MHH_BUDGET_* bits Budget_2::create (:1315-1412) would register: MHH_BUDGET_COR with a geostrophic forcing, MHH_BUDGET_DIFF with
// diff_smag2, the four buoyancy bits with a thermo, whose b (get_thermo_field "b" with its cyclic fill) is b_g. fields.mp holds u, v, w
// (u and v with flux_bot_g for the LES diffusion group), fields.sd p and evisc. The device memory is the caller's: work_g
// [work_elems()] doubles, prof_g [prof_elems()] of TF. A slab rank adds the double sums over the ranks through the Stats_sampler's
// sum_ranks between every sums call and its finish call, and the shares of bmean and pmean -- profiles of TF, summed as the
// reference's master.sum(prof, kcells) does after the division -- through sum_ranks_prof (TF = double: sum_ranks where it is unset).
// get_prof returns DEVICE pointers.
template<typename TF>
class Budget_2_sampler
{
    public:
        Budget_2_sampler(Grid<TF>& grid_in, Fields<TF>& fields_in, Stats_sampler<TF>& stats_in) : grid(grid_in), fields(fields_in), stats(stats_in) {}
        double* work_g = nullptr; TF* prof_g = nullptr; const TF* b_g = nullptr;
        unsigned int groups = MHH_BUDGET_KE | MHH_BUDGET_SHEAR | MHH_BUDGET_TURB | MHH_BUDGET_PRES | MHH_BUDGET_RDSTR;
        int swdiff = MHH_DIFF_SMAG2; TF utrans = 0, vtrans = 0, fc = 0;
        std::function<void(TF*, size_t)> sum_ranks_prof;             // the sum over the ranks, in place, of device values of TF

        int nprofs() const { const int n = mhh_budget_2_nprofs(groups); if (n < 0) throw std::runtime_error("Budget_2: unknown group bit"); return n; }
        size_t work_elems() const
        {
            mhh_grid g = grid.abi();
            return (size_t)mhh_budget_2_scratch_elems(&g, nm()) + (size_t)mhh_field_mean_scratch_elems(&g, 2) + (size_t)(nprofs() + 3)*nm()*grid.gd.kcells;
        }
        size_t prof_elems() const { return ((size_t)(nprofs() + 3)*nm() + 2)*grid.gd.kcells; }

        void exec_stats(void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            const int n = nm(), np = nprofs();
            const size_t kc = grid.gd.kcells;
            double* scratch = work_g;
            double* mscratch = scratch + mhh_budget_2_scratch_elems(&g, n);
            double* sums = mscratch + mhh_field_mean_scratch_elems(&g, 2);
            TF* model = prof_g + (size_t)np*n*kc;                    // umodel, vmodel, wmodel [nmasks][kcells] each, then bmean, pmean
            TF* means = model + 3*(size_t)n*kc;
            const TF* u = fields.mp.at("u")->fld_g; const TF* v = fields.mp.at("v")->fld_g; const TF* w = fields.mp.at("w")->fld_g;
            const TF* p = fields.sd.count("p") ? fields.sd.at("p")->fld_g : nullptr;
            mhh_check(mhh_budget_2_model_sums(&g, stats.mfield_g, n, u, v, w, sums, scratch, stream));
            all_ranks(sums, 3*(size_t)n*kc, stream);
            mhh_check(mhh_budget_2_model_finish(&g, n, sums, stats.nmask_g, model, stream));
            const bool thermo = groups & (MHH_BUDGET_BUOY | MHH_BUDGET_BW_BUOY | MHH_BUDGET_ADV_S | MHH_BUDGET_PRES_S);
            if (thermo)
            {
                if (!b_g || !p) throw std::runtime_error("Budget_2: the buoyancy, b2 and bw groups need b and p");
                const void* flds[2] = {b_g, p}; void* profs[2] = {means, means + kc};
                mhh_check(mhh_field_mean_profile(&g, flds, 2, profs, mscratch, stream));      // a slab rank: its share of the means
                if (grid.gd.npy != 1)
                {
                    if (sum_ranks_prof) sum_ranks_prof(means, 2*kc);
                    else if (sizeof(TF) == sizeof(double)) all_ranks(reinterpret_cast<double*>(means), 2*kc, stream);
                    else throw std::runtime_error("Budget_2: a slab rank (npy > 1) needs sum_ranks_prof, the sum over the ranks of a profile");
                }
            }
            mhh_budget_2_desc d{};
            d.u = u; d.v = v; d.w = w; d.p = p; d.b = b_g;
            d.evisc = fields.sd.count("evisc") ? fields.sd.at("evisc")->fld_g : nullptr;
            d.u_fluxbot = fields.mp.at("u")->flux_bot_g; d.v_fluxbot = fields.mp.at("v")->flux_bot_g;
            d.umodel = model; d.vmodel = model + (size_t)n*kc; d.wmodel = model + 2*(size_t)n*kc;
            if (thermo) { d.bmean = means; d.pmean = means + kc; }
            d.utrans = utrans; d.vtrans = vtrans; d.fc = fc; d.order = 2; d.diff_scheme = swdiff; d.groups = groups;
            mhh_check(mhh_budget_2_sums(&g, stats.mfield_g, n, &d, sums, scratch, stream));
            all_ranks(sums, (size_t)np*n*kc, stream);
            mhh_check(mhh_budget_2_finish(&g, n, &d, sums, stats.nmask_g, prof_g, stream));
        }
        const TF* get_prof(const std::string& mask, const std::string& name) const
        {
            const auto& masks = stats.get_masks();
            size_t m = 0;
            while (m < masks.size() && masks[m] != mask) ++m;
            if (m == masks.size()) throw std::runtime_error("Budget_2: no such mask");
            for (int n=0; n<nprofs(); ++n)
                if (name == mhh_budget_2_prof_name(groups, n, nullptr)) return prof_g + ((size_t)n*masks.size() + m)*grid.gd.kcells;
            throw std::runtime_error("Budget_2: no such profile: " + name);
        }
        const TF* get_model(int which, const std::string& mask) const      // 0 umodel, 1 vmodel, 2 wmodel
        {
            const auto& masks = stats.get_masks();
            size_t m = 0;
            while (m < masks.size() && masks[m] != mask) ++m;
            if (m == masks.size()) throw std::runtime_error("Budget_2: no such mask");
            if (which < 0 || which > 2) throw std::runtime_error("Budget_2: model profiles are 0 umodel, 1 vmodel, 2 wmodel");
            return prof_g + (((size_t)nprofs() + which)*masks.size() + m)*grid.gd.kcells;
        }

    private:
        int nm() const { return (int)stats.get_masks().size(); }
        void all_ranks(double* d, size_t n, void*)
        {
            if (grid.gd.npy == 1) return;
            if (!stats.sum_ranks) throw std::runtime_error("Budget_2: a slab rank (npy > 1) needs the Stats_sampler's sum_ranks");
            stats.sum_ranks(d, n);
        }
        Grid<TF>& grid; Fields<TF>& fields; Stats_sampler<TF>& stats;
};

// ---- Cross (include/cross.h; src/cross.cxx) ---------------------------------------------------------------------------------
// The cross-section files with the fields left on the device: the index lists of Cross::create (:323-460, mhh_cross_indices_host), a
// staging buffer the planes of one call are packed into (one launch), ONE copy of it to the host, and the slice writers of
// src/field3d_io.cxx (:754-861; the MPI forms :234-...): exclusive creation ("wbx"), the global file on a slab. Every `data` is a
// DEVICE pointer. The memory is the caller's: staging_g [staging_elems()] of TF on the device; to_host copies device memory to the
// host (hipMemcpy, device to host) after synchronising the stream. A slab rank (npy > 1) needs barrier, and the filled north halo
// of a field whose half-level xz row jtot is asked for; lngrad needs the filled ghost cells of its field.
enum class Cross_direction { Top_to_bottom, Bottom_to_top };
template<typename TF>
class Cross_sampler
{
    public:
        Cross_sampler(Grid<TF>& grid_in, Fields<TF>& fields_in, const std::string& path_in = ".") : grid(grid_in), fields(fields_in), path(path_in) {}
        std::vector<TF> xy, xz, yz;                                  // [cross] xy, xz, yz: heights, y and x locations
        std::vector<int> kxy, kxyh, jxz, jxzh, ixz, ixzh;            // global interior indices, full and half
        TF* staging_g = nullptr;
        std::function<void(void*, const void*, size_t)> to_host;
        std::function<void()> barrier;

        // Cross::create (:323-460): a location outside the domain throws, and the message names it
        void create()
        {
            mhh_grid g = grid.abi(true);
            auto run = [&](int kind, const std::vector<TF>& loc, std::vector<int>& full, std::vector<int>& half)
            {
                std::vector<double> l(loc.begin(), loc.end());
                full.assign(loc.size(), 0); half.assign(loc.size(), 0);
                int nf = 0, nh = 0;
                mhh_check(mhh_cross_indices_host(&g, kind, l.data(), (int)l.size(), full.data(), &nf, half.data(), &nh));
                full.resize(nf); half.resize(nh);
            };
            run(MHH_CROSS_XY, xy, kxy, kxyh); run(MHH_CROSS_XZ, xz, jxz, jxzh); run(MHH_CROSS_YZ, yz, ixz, ixzh);
        }
        // the planes of the largest call: every section of one variable
        size_t staging_elems() const
        {
            const auto& gd = grid.gd;
            const size_t nj = std::max(jxz.size(), jxzh.size()), ni = std::max(ixz.size(), ixzh.size()), nk = std::max(kxy.size(), kxyh.size());
            return std::max<size_t>(1, nj*gd.kmax*gd.imax + ni*gd.kmax*gd.jmax + nk*gd.jmax*gd.imax) + (size_t)gd.jmax*gd.imax;
        }

        // Cross::cross_simple (:564-636); loc = {1,0,0} u, {0,1,0} v, {0,0,1} w: the half-level list of that direction
        int cross_simple(const TF* data, TF offset, const std::string& name, int iotime, const std::array<int,3>& loc, void* stream = nullptr)
        {
            return sections(data, offset, name, iotime, 0, loc[1] ? jxzh : jxz, loc[0] ? ixzh : ixz, loc[2] ? kxyh : kxy, stream);
        }
        // Cross::cross_lngrad (:653-703): order 2 calc_lngrad_2nd, 4 calc_lngrad_4th, on the cells of the sections alone
        int cross_lngrad(const TF* a, const std::string& name, int iotime, int order, void* stream = nullptr)
        {
            return sections(a, TF(0), name, iotime, order, jxz, ixz, kxy, stream);
        }
        // Cross::cross_plane (:638-651): data is a 2-D array [ijcells]
        int cross_plane(const TF* data, TF offset, const std::string& name, int iotime, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_cross_job j{}; j.fld = data; j.kind = MHH_CROSS_PLANE; j.offset = offset; j.out = staging_g;
            mhh_check(mhh_cross_gather(&g, &j, 1, stream));
            return write_plane(name, iotime);
        }
        // Cross::cross_path (:705-725)
        int cross_path(const TF* data, const std::string& name, int iotime, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_cross_path(&g, data, fields.rhoref_g, staging_g, stream));
            return write_plane(name, iotime);
        }
        // Cross::cross_height_threshold (:738-760)
        int cross_height_threshold(const TF* data, TF threshold, Cross_direction direction, const std::string& name, int iotime, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_cross_height_threshold(&g, data, threshold, direction == Cross_direction::Bottom_to_top, staging_g, stream));
            return write_plane(name, iotime);
        }

    private:
        std::string filename(const std::string& name, const char* sect, int index, int iotime) const
        {
            char buf[512];
            if (index < 0) std::snprintf(buf, sizeof(buf), "%s/%s.%s.%07d", path.c_str(), name.c_str(), sect, iotime);
            else           std::snprintf(buf, sizeof(buf), "%s/%s.%s.%05d.%07d", path.c_str(), name.c_str(), sect, index, iotime);
            return buf;
        }
        void fetch(size_t n)
        {
            if (!to_host) throw std::runtime_error("Cross: to_host, the copy of device memory to the host, is not set");
            host.resize(n);
            to_host(host.data(), staging_g, n*sizeof(TF));
        }
        void meet() const
        {
            if (grid.gd.npy == 1) return;
            if (!barrier) throw std::runtime_error("Cross: a slab rank (npy > 1) needs barrier");
            barrier();
        }
        // One file written by this rank alone, exclusively ("wbx", src/field3d_io.cxx:779-785)
        static int write_own(const std::string& fn, const TF* data, size_t n)
        {
            FILE* f = std::fopen(fn.c_str(), "wbx");
            if (!f) return 1;
            int nerror = (std::fwrite(data, sizeof(TF), n, f) != n);
            if (std::fclose(f)) ++nerror;
            return nerror;
        }
        // One global file of rows x (cols per rank) x npy: rank 0 creates it exclusively and writes its share, the others follow after
        // a barrier (MPI_File_open with MPI_MODE_CREATE | MPI_MODE_EXCL and the subarray view, :320-350)
        int write_shared(const std::string& fn, const TF* data, int rows, int cols, bool split_rows)
        {
            const auto& gd = grid.gd;
            if (gd.npy == 1) return write_own(fn, data, (size_t)rows*cols);
            int nerror = 0;
            auto put = [&](const char* mode)
            {
                FILE* f = std::fopen(fn.c_str(), mode);
                if (!f) { ++nerror; return; }
                if (split_rows)                 // xy: [jtot][itot], this rank's rows in one piece
                {
                    if (std::fseek(f, (long)((size_t)gd.mpicoordy*rows*cols*sizeof(TF)), SEEK_SET) || std::fwrite(data, sizeof(TF), (size_t)rows*cols, f) != (size_t)rows*cols) ++nerror;
                }
                else                            // yz: [kmax][jtot], this rank's columns of every row
                    for (int r=0; r<rows && !nerror; ++r)
                        if (std::fseek(f, (long)(((size_t)r*cols*gd.npy + (size_t)gd.mpicoordy*cols)*sizeof(TF)), SEEK_SET) ||
                            std::fwrite(data + (size_t)r*cols, sizeof(TF), cols, f) != (size_t)cols) ++nerror;
                if (std::fclose(f)) ++nerror;
            };
            if (gd.mpicoordy == 0) put("wbx");
            meet();
            if (gd.mpicoordy != 0) put("r+b");
            meet();
            return nerror;
        }
        int write_plane(const std::string& name, int iotime)
        {
            const auto& gd = grid.gd;
            fetch((size_t)gd.jmax*gd.imax);
            return write_shared(filename(name, "xy", -1, iotime), host.data(), gd.jmax, gd.imax, true);
        }
        int sections(const TF* data, TF offset, const std::string& name, int iotime, int order, const std::vector<int>& jlist, const std::vector<int>& ilist,
                     const std::vector<int>& klist, void* stream)
        {
            const auto& gd = grid.gd;
            mhh_grid g = grid.abi();
            std::vector<mhh_cross_job> jobs; std::vector<long long> jpos(jlist.size(), -1);
            size_t pos = 0;
            auto add = [&](int kind, int index, size_t cells)
            {
                mhh_cross_job j{}; j.fld = data; j.kind = kind; j.index = index; j.k0 = gd.kstart; j.k1 = gd.kend; j.offset = offset; j.out = staging_g + pos;
                jobs.push_back(j); pos += cells;
            };
            const int jtot = gd.jmax*gd.npy;
            for (size_t n=0; n<jlist.size(); ++n)
            {
                // the row's owner; the half-level row jtot is the cyclic image of row 0: the last rank's north ghost row
                const bool top = (jlist[n] == jtot);
                if ((top ? gd.npy - 1 : jlist[n]/gd.jmax) != gd.mpicoordy) continue;
                jpos[n] = (long long)pos;
                add(MHH_CROSS_XZ, top ? gd.jend : jlist[n] % gd.jmax + gd.jgc, (size_t)gd.kmax*gd.imax);
            }
            const size_t ipos = pos;
            for (int i : ilist) add(MHH_CROSS_YZ, i % gd.imax + gd.igc, (size_t)gd.kmax*gd.jmax);
            const size_t kpos = pos;
            for (int k : klist) add(MHH_CROSS_XY, k + gd.kgc, (size_t)gd.jmax*gd.imax);
            if (!jobs.empty())
            {
                if (order == 0) mhh_check(mhh_cross_gather(&g, jobs.data(), (int)jobs.size(), stream));
                else            mhh_check(mhh_cross_lngrad(&g, order, jobs.data(), (int)jobs.size(), stream));
                fetch(pos);
            }
            int nerror = 0;
            for (size_t n=0; n<jlist.size(); ++n)
                if (jpos[n] >= 0) nerror += write_own(filename(name, "xz", jlist[n], iotime), host.data() + jpos[n], (size_t)gd.kmax*gd.imax);
            for (size_t n=0; n<ilist.size(); ++n)
                nerror += write_shared(filename(name, "yz", ilist[n], iotime), host.data() + ipos + n*(size_t)gd.kmax*gd.jmax, gd.kmax, gd.jmax, false);
            for (size_t n=0; n<klist.size(); ++n)
                nerror += write_shared(filename(name, "xy", klist[n], iotime), host.data() + kpos + n*(size_t)gd.jmax*gd.imax, gd.jmax, gd.imax, true);
            return nerror;
        }
        Grid<TF>& grid; Fields<TF>& fields; std::string path;
        std::vector<TF> host;
};

// ---- Immersed_boundary (include/immersed_boundary.h; src/immersed_boundary.cxx, src/immersed_boundary.cu) -----------------------
// sw_immersed_boundary=dem on one rank or a y-slab. create() is the host set-up of Immersed_boundary::create (:766-918) over
// mhh_ib_ghost_cells_host, _interp_dem_host and _k_dem_host: `dem` [ijcells] and the planes of `sbot_spatial` hold the data WITH
// filled halos (boundary_cyclic.exec_2d, :800, is the caller's, as is the reading of the files). prepare_device() builds the device
// tables of mhh_ib_job (one cell offset per point, the per-point arrays transposed) through the caller's alloc / upload / release.
// exec_momentum and exec_scalars are one launch each; the cyclic fills that follow (.cu:134-136, :166) go through `cyclic`, which a
// slab rank sets to its exchange (default: Boundary_cyclic::exec_g of every field). The halos of k_dem (boundary_cyclic.exec_2d, :916)
// are filled on the host in create(): east-west by a local wrap, north-south by a local wrap on one rank and through
// `exchange_k_dem` on a slab, without which create() throws there.
template<typename TF>
struct Ghost_cells
{
    int nghost = 0;
    std::vector<int> i, j, k, ip_i, ip_j, ip_k;
    std::vector<TF> xb, yb, zb, xi, yi, zi, di, ip_d, c_idw, c_idw_sum;
    std::map<std::string, std::vector<TF>> sbot;
    std::vector<TF> mbot;
    int* cell_g = nullptr; int* ip_g = nullptr;                                 // [nghost], [n_idw][nghost]
    TF* c_idw_g = nullptr; TF* c_idw_sum_g = nullptr; TF* di_g = nullptr;      // [n_idw][nghost], [nghost], [nghost]
    std::map<std::string, TF*> sbot_g;
    TF* mbot_g = nullptr;
};

template<typename TF>
class Immersed_boundary
{
    public:
        Immersed_boundary(Grid<TF>& grid_in, Fields<TF>& fields_in) : grid(grid_in), fields(fields_in) {}
        int n_idw_points = 0;                                        // [IB] n_idw_points
        int sbcbot = MHH_IB_DIRICHLET;                               // [IB] sbcbot: MHH_IB_*
        std::map<std::string, TF> sbc;                               // [IB] sbot[scalar]
        std::map<std::string, std::vector<TF>> sbot_spatial;         // <scalar>_sbot.0000000 as [ijcells], halos filled
        std::vector<TF> dem;                                         // dem.0000000 as [ijcells], halos filled
        std::vector<unsigned int> k_dem;                             // [ijcells], halos filled
        unsigned int* k_dem_g = nullptr; TF* dem_g = nullptr;
        std::map<std::string, Ghost_cells<TF>> ghost;
        std::function<void*(size_t)> alloc;                          // device memory of that many bytes
        std::function<void(void*, const void*, size_t)> upload;      // host to device
        std::function<void(void*)> release;
        std::function<void(const std::vector<TF*>&, void*)> cyclic;  // the cyclic fills of these fields on the stream
        // slab ranks: fill the jgc south and jgc north ghost rows of this host plane [jcells][icells] from the ring neighbours' interior
        // rows (the rows arrive with their east-west halos filled)
        std::function<void(unsigned int*)> exchange_k_dem;

        void create()
        {
            const auto& gd = grid.gd;
            if ((int)dem.size() != gd.ijcells) throw std::runtime_error("Immersed_boundary: dem holds ijcells values, halos filled");
            std::vector<TF> x(gd.icells), xh(gd.icells), y(gd.jcells), yh(gd.jcells);
            const double yoff = gd.mpicoordy * gd.ysize / gd.npy;            // src/grid.cxx:248-262
            for (int i=0; i<gd.icells; ++i) { x[i] = 0.5*gd.dx + (i-gd.igc)*gd.dx + 0.; xh[i] = (i-gd.igc)*gd.dx + 0.; }
            for (int j=0; j<gd.jcells; ++j) { y[j] = 0.5*gd.dy + (j-gd.jgc)*gd.dy + yoff; yh[j] = (j-gd.jgc)*gd.dy + yoff; }
            offx = gd.igc; offy = -gd.mpicoordy*gd.jmax + gd.jgc;             // :781-782
            ghost.clear();
            calc(ghost["u"], xh, y, gd.z, gd.dz, MHH_IB_DIRICHLET);
            calc(ghost["v"], x, yh, gd.z, gd.dz, MHH_IB_DIRICHLET);
            calc(ghost["w"], x, y, gd.zh, gd.dzh, MHH_IB_DIRICHLET);
            for (const char* n : {"u", "v", "w"}) ghost.at(n).mbot.assign(ghost.at(n).nghost, TF(0));
            mhh_grid g = grid.abi(true);
            if (!fields.sp.empty())
            {
                Ghost_cells<TF>& gs = ghost["s"];
                calc(gs, x, y, gd.z, gd.dz, sbcbot);
                for (auto& it : fields.sp)
                {
                    std::vector<TF>& bv = gs.sbot[it.first];
                    bv.assign(gs.nghost, sbc.count(it.first) ? sbc.at(it.first) : TF(0));
                    if (sbot_spatial.count(it.first))           // interp2_dem at (xb, yb) (:891-897)
                        mhh_check(mhh_ib_interp_dem_host(&g, sbot_spatial.at(it.first).data(), x.data(), y.data(), gs.xb.data(), gs.yb.data(), gs.nghost, offx, offy, bv.data()));
                }
            }
            k_dem.assign(gd.ijcells, 0u);
            mhh_check(mhh_ib_k_dem_host(&g, dem.data(), gd.z.data(), k_dem.data()));
            const int ic = gd.icells;
            for (int j=gd.jstart; j<gd.jend; ++j)
                for (int i=0; i<gd.igc; ++i)
                {
                    k_dem[j*ic + i] = k_dem[j*ic + gd.iend-gd.igc + i];
                    k_dem[j*ic + gd.iend + i] = k_dem[j*ic + gd.istart + i];
                }
            if (gd.npy == 1)
                for (int j=0; j<gd.jgc; ++j)
                    for (int i=0; i<ic; ++i)
                    {
                        // (jtot == 1 replicates the row, as Boundary_cyclic does)
                        k_dem[j*ic + i] = k_dem[(gd.jtot == 1 ? gd.jstart : gd.jend - gd.jgc + j)*ic + i];
                        k_dem[(gd.jend + j)*ic + i] = k_dem[(gd.jtot == 1 ? gd.jstart : gd.jstart + j)*ic + i];
                    }
            else if (exchange_k_dem) exchange_k_dem(k_dem.data());
            else throw std::runtime_error("Immersed_boundary: a slab rank (npy > 1) needs exchange_k_dem for the north-south halos of k_dem");
        }

        void prepare_device()
        {
            if (!alloc || !upload) throw std::runtime_error("Immersed_boundary: alloc and upload are not set");
            const auto& gd = grid.gd;
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
                        c[q*n + m] = gh.c_idw[m*nq + q];
                    }
                }
                gh.cell_g = put(cell); gh.ip_g = put(ip); gh.c_idw_g = put(c); gh.c_idw_sum_g = put(gh.c_idw_sum); gh.di_g = put(gh.di);
                gh.mbot_g = put(gh.mbot);
                for (auto& sb : gh.sbot) gh.sbot_g[sb.first] = put(sb.second);
            }
            dem_g = put(dem);
            k_dem_g = put(k_dem);
        }

        void clear_device()
        {
            auto drop = [&](auto*& p) { if (p && release) release(p); p = nullptr; };
            for (auto& it : ghost)
            {
                Ghost_cells<TF>& gh = it.second;
                drop(gh.cell_g); drop(gh.ip_g); drop(gh.c_idw_g); drop(gh.c_idw_sum_g); drop(gh.di_g); drop(gh.mbot_g);
                for (auto& sb : gh.sbot_g) drop(sb.second);
                gh.sbot_g.clear();
            }
            drop(dem_g); drop(k_dem_g);
        }

        // Immersed_boundary::exec_momentum (:640-674, .cu:108-137)
        void exec_momentum(void* stream = nullptr)
        {
            if (ghost.empty()) return;
            mhh_grid g = grid.abi();
            mhh_ib_job jobs[3];
            std::vector<TF*> flds;
            int n = 0;
            for (const char* name : {"u", "v", "w"})
            {
                const Ghost_cells<TF>& gh = ghost.at(name);
                jobs[n++] = job(fields.mp.at(name)->fld_g, gh.mbot_g, MHH_IB_DIRICHLET, fields.visc, gh);
                flds.push_back(fields.mp.at(name)->fld_g);
            }
            mhh_check(mhh_ib_set_ghost_cells(&g, n_idw_points, jobs, 3, stream));
            fill(flds, stream);
        }
        // Immersed_boundary::exec_scalars (:677-696, .cu:140-168)
        void exec_scalars(void* stream = nullptr)
        {
            if (ghost.empty() || fields.sp.empty()) return;
            mhh_grid g = grid.abi();
            const Ghost_cells<TF>& gh = ghost.at("s");
            std::vector<mhh_ib_job> jobs;
            std::vector<TF*> flds;
            for (auto& it : fields.sp)
            {
                jobs.push_back(job(it.second->fld_g, gh.sbot_g.at(it.first), sbcbot, it.second->visc, gh));
                flds.push_back(it.second->fld_g);
            }
            mhh_check(mhh_ib_set_ghost_cells(&g, n_idw_points, jobs.data(), (int)jobs.size(), stream));
            fill(flds, stream);
        }
        // Immersed_boundary::get_mask (:930-946): calc_mask into two device fields; the caller hands them to
        // Stats_sampler::set_mask_thres("ib", mask, maskh, 0.5, Plus) (:942)
        bool has_mask(const std::string& name) const { return name == "ib"; }
        void get_mask(TF* mask_g, TF* maskh_g, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            mhh_check(mhh_ib_mask(&g, dem_g, mask_g, maskh_g, stream));
        }
        // Immersed_boundary::exec_cross (:950-985): <scalar>fluxbot_ib of every listed scalar, a plane with no offset; flux_g [ijcells]
        // is the caller's scratch (tmp->flux_bot)
        int exec_cross(Cross_sampler<TF>& cross, const std::vector<std::string>& crosslist, int iotime, TF* flux_g, void* stream = nullptr)
        {
            mhh_grid g = grid.abi();
            int nerror = 0;
            const std::string ending = "fluxbot_ib";
            for (const std::string& s : crosslist)
            {
                if (s.size() < ending.size() || s.compare(s.size() - ending.size(), ending.size(), ending)) continue;
                const std::string scalar = s.substr(0, s.size() - ending.size());
                if (!fields.sp.count(scalar)) continue;
                mhh_check(mhh_ib_fluxbot(&g, flux_g, k_dem_g, fields.sp.at(scalar)->fld_g, fields.sp.at(scalar)->visc, stream));
                nerror += cross.cross_plane(flux_g, TF(0.), s, iotime, stream);
            }
            return nerror;
        }

    private:
        void calc(Ghost_cells<TF>& gh, const std::vector<TF>& x, const std::vector<TF>& y, const std::vector<TF>& z, const std::vector<TF>& dz, int bc)
        {
            mhh_grid g = grid.abi(true);
            int n = 0;
            mhh_check(mhh_ib_ghost_cells_host(&g, dem.data(), x.data(), y.data(), z.data(), dz.data(), n_idw_points, bc, offx, offy, &n, nullptr));
            const size_t np = (size_t)n*n_idw_points;
            gh.nghost = n;
            for (auto* v : {&gh.i, &gh.j, &gh.k}) v->assign(n, 0);
            for (auto* v : {&gh.ip_i, &gh.ip_j, &gh.ip_k}) v->assign(np, 0);
            for (auto* v : {&gh.xb, &gh.yb, &gh.zb, &gh.xi, &gh.yi, &gh.zi, &gh.di, &gh.c_idw_sum}) v->assign(n, TF(0));
            for (auto* v : {&gh.ip_d, &gh.c_idw}) v->assign(np, TF(0));
            mhh_ib_ghost_lists l{gh.i.data(), gh.j.data(), gh.k.data(), gh.xb.data(), gh.yb.data(), gh.zb.data(), gh.xi.data(), gh.yi.data(), gh.zi.data(),
                                 gh.di.data(), gh.ip_i.data(), gh.ip_j.data(), gh.ip_k.data(), gh.ip_d.data(), gh.c_idw.data(), gh.c_idw_sum.data()};
            mhh_check(mhh_ib_ghost_cells_host(&g, dem.data(), x.data(), y.data(), z.data(), dz.data(), n_idw_points, bc, offx, offy, &n, &l));
        }
        // (an empty vector still gets one element: a null table pointer would be refused where nghost > 0 only, but a valid address
        // keeps every job uniform)
        template<class T> T* put(const std::vector<T>& v)
        {
            T* d = static_cast<T*>(alloc(std::max<size_t>(1, v.size())*sizeof(T)));
            if (!v.empty()) upload(d, v.data(), v.size()*sizeof(T));
            return d;
        }
        mhh_ib_job job(TF* fld, const TF* bv, int bc, TF visc, const Ghost_cells<TF>& gh) const
        {
            mhh_ib_job j{};
            j.fld = fld; j.boundary_value = bv; j.bc = bc; j.nghost = gh.nghost; j.visc = visc;
            j.cell = gh.cell_g; j.ip = gh.ip_g; j.c_idw = gh.c_idw_g; j.c_idw_sum = gh.c_idw_sum_g; j.di = gh.di_g;
            return j;
        }
        void fill(const std::vector<TF*>& flds, void* stream)
        {
            if (cyclic) { cyclic(flds, stream); return; }
            mhh_grid g = grid.abi();
            std::vector<void*> p(flds.begin(), flds.end());
            mhh_check(mhh_boundary_cyclic_n(&g, p.data(), (int)p.size(), MHH_EDGE_BOTH, stream));
        }
        Grid<TF>& grid; Fields<TF>& fields;
        int offx = 0, offy = 0;
};

// ---- Source (include/source.h:33-100; src/source.cxx) ------------------------------------------------------------------------------
// The reference's lists as public members (what its constructor reads from [source]), init / create / exec with its meaning.
// create() hands them to mhh_source_create, which redoes calc_shape / calc_shape_profile / calc_norm on the host; exec() is
// Source::exec (:355-432) after the Timedep interpolation, which stays the caller's: set source_x0 .. strength and call update().
template<typename TF>
class Source
{
    public:
        Source(Grid<TF>& gridin, Fields<TF>& fieldsin) : grid(gridin), fields(fieldsin) {}
        ~Source() { if (handle) mhh_source_destroy(handle); }
        Source(const Source&) = delete;
        bool swsource = false, sw_emission_profile = false;
        std::vector<std::string> sourcelist;
        std::vector<TF> source_x0, source_y0, source_z0, sigma_x, sigma_y, sigma_z, strength, line_x, line_y, line_z;
        std::vector<bool> sw_vmr;
        std::vector<int> profile_index;
        std::map<int, std::vector<TF>> profile_z;                    // [kcells] each, as Source::create reads them (:280-286)
        void init() {}
        void create(void* stream = nullptr)
        {
            if (!swsource) return;
            auto& gd = grid.get_grid_data();
            const size_t n = source_x0.size();
            std::vector<int> rows;                                   // the unique profile indices in order -> rows of the table
            std::vector<TF> prof;
            for (auto& it : profile_z)
            {
                if ((int)it.second.size() != gd.kcells) throw std::runtime_error("mhh: an emission profile holds kcells elements");
                rows.push_back(it.first); prof.insert(prof.end(), it.second.begin(), it.second.end());
            }
            std::vector<mhh_source_desc> d(n);
            for (size_t m=0; m<n; ++m)
            {
                d[m] = mhh_source_desc{};
                d[m].scalar = scalar_index(fields, sourcelist[m]);
                d[m].swvmr = sw_vmr[m]; d[m].profile_index = -1;
                if (sw_emission_profile)
                    d[m].profile_index = (int)(std::find(rows.begin(), rows.end(), profile_index[m]) - rows.begin());
                d[m].x0 = source_x0[m]; d[m].y0 = source_y0[m]; d[m].z0 = source_z0[m];
                d[m].sigma_x = sigma_x[m]; d[m].sigma_y = sigma_y[m]; d[m].sigma_z = sigma_z[m];
                d[m].line_x = line_x[m]; d[m].line_y = line_y[m]; d[m].line_z = line_z[m]; d[m].strength = strength[m];
            }
            mhh_grid gh = grid.abi(true);
            if (handle) { mhh_source_destroy(handle); handle = nullptr; }
            mhh_check(mhh_source_create(&gh, d.data(), (int)n, prof.empty() ? nullptr : prof.data(), (int)rows.size(), fields.rhoref.data(), stream, &handle));
        }
        // swtimedep_location / swtimedep_strength (:362-401): the members hold what Timedep interpolated
        void update(bool location, bool strength_too, void* stream = nullptr)
        {
            if (!swsource || !(location || strength_too)) return;
            std::vector<double> x(source_x0.begin(), source_x0.end()), y(source_y0.begin(), source_y0.end()), z(source_z0.begin(), source_z0.end()),
                                q(strength.begin(), strength.end());
            mhh_check(mhh_source_update(handle, -1, location ? x.data() : nullptr, location ? y.data() : nullptr, location ? z.data() : nullptr,
                                        strength_too ? q.data() : nullptr, stream));
        }
        void exec(void* stream = nullptr)
        {
            if (!swsource) return;
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields);
            mhh_check(mhh_source_exec(handle, &g, &f, stream));
        }
        TF get_norm(int n) const { double v; mhh_check(mhh_source_norm(handle, n, &v)); return TF(v); }
        std::array<int, 6> get_ranges(int n) const { std::array<int, 6> r; mhh_check(mhh_source_ranges(handle, n, r.data())); return r; }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
        mhh_source* handle = nullptr;
};

// ---- Decay (include/decay.h:42-78; src/decay.cxx) -------------------------------------------------------------------------------------
enum class Decay_type {disabled, enabled, exponential};
template<typename TF>
class Decay
{
    public:
        Decay(Grid<TF>& gridin, Fields<TF>& fieldsin) : grid(gridin), fields(fieldsin) {}
        struct Decay_var { double timescale; Decay_type type; };
        std::map<std::string, Decay_var> dmap;                      // what init() reads from [decay] (:66-88)
        TF nstd_couvreux = 1.;
        void init() {}
        void create(Stats&) {}
        void exec(double dt, Stats&, void* stream = nullptr)        // (:97-111); stats.calc_tend is a no-op off sampling steps
        {
            mhh_decay_params p{};
            for (auto& it : dmap)
                if (it.second.type == Decay_type::exponential)
                {
                    const int n = scalar_index(fields, it.first);
                    if (n < 0) throw std::runtime_error("mhh: decay of an unknown scalar " + it.first);
                    p.exponential[n] = 1; p.timescale[n] = it.second.timescale;
                }
            mhh_grid g = grid.abi(); mhh_fields f = abi_fields(fields);
            mhh_check(mhh_decay_exec(&g, &f, &p, dt, stream));
        }
        bool has_mask(std::string name) { return name == "couvreux"; }
        // (:123-187). couvreux, couvreuxh: the two tmp fields; work: mhh_decay_couvreux_scratch_elems + 2*kcells device doubles;
        // sum_ranks: the sum over the ranks, in place, of device doubles (empty on one rank), as master.sum
        void get_mask(Stats_sampler<TF>& stats, std::string mask_name, Field3d<TF>& couvreux, Field3d<TF>& couvreuxh, double* work,
                      std::function<void(double*, size_t)> sum_ranks = nullptr, void* stream = nullptr)
        {
            if (mask_name != "couvreux") throw std::runtime_error("Decay cannot provide mask: \"" + mask_name + "\"");
            if (fields.sp.find("couvreux") == fields.sp.end()) throw std::runtime_error("Couvreux mask not available without couvreux scalar");
            mhh_grid g = grid.abi();
            double* sums = work + mhh_decay_couvreux_scratch_elems(&g);
            const TF* s = fields.sp.at("couvreux")->fld_g;
            mhh_check(mhh_decay_couvreux_sums(&g, s, work, sums, stream));
            if (sum_ranks) sum_ranks(sums, 2*(size_t)grid.get_grid_data().kcells);
            mhh_check(mhh_decay_couvreux_field(&g, s, sums, nstd_couvreux, couvreux.fld_g, couvreuxh.fld_g, stream));
            stats.set_mask_thres(mask_name, couvreux, couvreuxh, TF(0.), Stats_mask_type::Plus, stream);
        }
    private:
        Grid<TF>& grid; Fields<TF>& fields;
};

// ---- Boundary_outflow (include/boundary_outflow.h:33-51; src/boundary_outflow.cxx) ---------------------------------------------------
// Open lateral boundaries for scalars. The constructor takes what the reference's reads from [boundary] (flow_direction[west ..
// north], :207-225) and the scalar_outflow list that Boundary holds (src/boundary.cxx:464-469); exec(data, inflow_prof) is the
// reference's member, exec_all is Boundary::set_prognostic_outflow_bcs for all scalars of the list in the launches of one. The
// sequence of Model::exec calls exec_all directly after the cyclic fills (src/model.cxx:347) and, with an immersed boundary, once
// more after ib->exec_scalars (:383). swspatialorder: grid.get_spatial_order().
enum class Edge_location {West, East, South, North};
enum class Flow_direction {Inflow, Outflow};
template<typename TF>
class Boundary_outflow
{
    public:
        Boundary_outflow(Grid<TF>& gridin, std::map<Edge_location, Flow_direction> flow_directionin, std::vector<std::string> scalar_outflowin,
                         int swspatialorderin = 2) :
            scalar_outflow(std::move(scalar_outflowin)), swspatialorder(swspatialorderin), grid(gridin), flow_direction(std::move(flow_directionin))
        {
            if (!scalar_outflow.empty())
                for (Edge_location e : {Edge_location::West, Edge_location::East, Edge_location::South, Edge_location::North})
                    if (!flow_direction.count(e)) throw std::runtime_error("Boundary_outflow: a flow_direction is missing");
        }
        std::vector<std::string> scalar_outflow;
        int swspatialorder;
        // Boundary::process_inflow (src/boundary.cxx:411-426): ktot values at kstart .. kend-1 of a zeroed kcells vector (host)
        std::vector<TF> inflow_profile(const std::vector<TF>& prof_ktot) const
        {
            const auto& gd = grid.get_grid_data();
            if ((int)prof_ktot.size() != gd.ktot) throw std::runtime_error("Boundary_outflow: an inflow profile holds ktot values");
            std::vector<TF> table(gd.kcells);
            mhh_grid g = grid.abi(true);
            mhh_check(mhh_boundary_outflow_profile_host(&g, prof_ktot.data(), table.data()));
            return table;
        }
        // the edges this rank owns: mpicoordx == 0 == npx-1; mpicoordy == 0, mpicoordy == npy-1 (:247-323)
        int edges() const
        {
            const auto& gd = grid.get_grid_data();
            return MHH_OUTFLOW_WEST | MHH_OUTFLOW_EAST | (gd.mpicoordy == 0 ? MHH_OUTFLOW_SOUTH : 0) | (gd.mpicoordy == gd.npy-1 ? MHH_OUTFLOW_NORTH : 0);
        }
        // Boundary_outflow<TF>::exec (:236-343): data and inflow_prof [kcells] are device memory
        void exec(TF* data, const TF* inflow_prof, void* stream = nullptr)
        {
            void* f[1] = {data}; const void* p[1] = {inflow_prof};
            launch(f, p, 1, edges(), stream);
        }
        // Boundary::set_prognostic_outflow_bcs (src/boundary.cxx:464-469): every scalar of scalar_outflow, at most two launches
        void exec_all(Fields<TF>& fields, const std::map<std::string, TF*>& inflow_profiles_g, void* stream = nullptr) { exec_all(fields, inflow_profiles_g, edges(), stream); }
        void exec_all(Fields<TF>& fields, const std::map<std::string, TF*>& inflow_profiles_g, int edges_mask, void* stream = nullptr)
        {
            if (scalar_outflow.empty()) return;
            if (scalar_outflow.size() > MHH_MAX_SCALARS) throw std::runtime_error("mhh: more than MHH_MAX_SCALARS scalars");
            void* f[MHH_MAX_SCALARS]; const void* p[MHH_MAX_SCALARS];
            int n = 0;
            for (auto& s : scalar_outflow) { f[n] = fields.sp.at(s)->fld_g; p[n] = inflow_profiles_g.at(s); ++n; }
            launch(f, p, n, edges_mask, stream);
        }
    private:
        void launch(void* const* f, const void* const* p, int n, int edges_mask, void* stream)
        {
            int dirs[4];
            int e = 0;
            for (Edge_location loc : {Edge_location::West, Edge_location::East, Edge_location::South, Edge_location::North})
                dirs[e++] = flow_direction.at(loc) == Flow_direction::Inflow ? MHH_OUTFLOW_INFLOW : MHH_OUTFLOW_OUTFLOW;
            mhh_grid g = grid.abi();
            mhh_check(mhh_boundary_outflow_exec(&g, swspatialorder, f, n, p, dirs, edges_mask, stream));
        }
        Grid<TF>& grid;
        std::map<Edge_location, Flow_direction> flow_direction;
};

} // namespace mhh_host
