// integration/adaptor_cross.cxx -- the device form of the sampling members of the reference's Cross<TF> (src/cross.cxx has no .cu:
// its GPU build copies every prognostic field to the host whenever a section is due, src/model.cxx:444-451): cross_simple (:564-636),
// cross_plane (:638-651), cross_lngrad (:653-703), cross_path (:705-725) and cross_height_threshold (:738-760). Build src/cross.cxx
// with these members left out under USECUDA and this file in their place, and have the callers (Fields::exec_cross,
// src/fields.cxx:1221-1271, and the exec_cross of thermo, microphysics, boundary and radiation) hand over the DEVICE pointers
// (fld_g, flux_bot_g, ...) where they hand over fld.data() today; the copy of src/model.cxx:444-451 then goes.
//
// What crosses to the host is the planes alone: the jobs of one call are gathered (or evaluated: lngrad, path, threshold height)
// into one packed staging buffer on the device, copied in one piece, and put back at the places of a host tmp field that the
// reference's own writers read (Field3d_io::save_xy_slice / save_xz_slice / save_yz_slice, src/field3d_io.cxx:234-..., :754-861).
// The files, their names, the exclusive creation and the MPI layout are therefore the reference's, byte for byte. The offset is
// added by the writer, as there (TF data0). Index lists, Cross::create and everything else stay as they are.
#include <array>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>
#include "master.h"
#include "grid.h"
#include "soil_grid.h"
#include "fields.h"
#include "cross.h"
#include "mhh_adaptor.h"

#ifdef USECUDA
extern "C" int hipMalloc(void** ptr, size_t size);
extern "C" int hipFree(void* ptr);
extern "C" int hipMemcpy(void* dst, const void* src, size_t size, int kind);   // kind 2 = device to host

namespace
{
    struct Staging { void* dev = nullptr; size_t bytes = 0; };
    Staging staging;

    void* mhh_staging(size_t bytes)
    {
        if (bytes > staging.bytes)
        {
            if (staging.dev) hipFree(staging.dev);
            if (hipMalloc(&staging.dev, bytes) != 0) throw std::runtime_error("hipMalloc");
            staging.bytes = bytes;
        }
        return staging.dev;
    }

    // one plane of a call: what the job reads, and where its packed cells go in the host tmp field the writer reads
    struct Plane { int kind, index, k0, k1; size_t pos, cells; };

    template<typename TF, class GD>
    Plane mhh_plane(const GD& gd, int kind, int index, size_t pos)
    {
        const bool flat = (kind == MHH_CROSS_XY || kind == MHH_CROSS_PLANE);
        const size_t cells = (size_t)(kind == MHH_CROSS_YZ ? gd.jmax : gd.imax) * (flat ? gd.jmax : gd.kmax);
        return Plane{kind, index, gd.kstart, gd.kend, pos, cells};
    }

    // the packed planes of `planes` from `data_g` (order 0: the gather with no offset; 2, 4: lngrad) into the host array `packed`
    template<typename TF>
    void mhh_fetch(const mhh_grid& g, const TF* data_g, const std::vector<Plane>& planes, int order, std::vector<TF>& packed)
    {
        size_t total = 0;
        for (const Plane& p : planes) total += p.cells;
        packed.resize(total);
        if (!total) return;
        TF* out = static_cast<TF*>(mhh_staging(total*sizeof(TF)));
        std::vector<mhh_cross_job> jobs;
        for (const Plane& p : planes)
        {
            mhh_cross_job j{}; j.fld = data_g; j.kind = p.kind; j.index = p.index; j.k0 = p.k0; j.k1 = p.k1; j.offset = 0.; j.out = out + p.pos;
            jobs.push_back(j);
        }
        if (order == 0) mhh_check(mhh_cross_gather(&g, jobs.data(), (int)jobs.size(), nullptr));
        else            mhh_check(mhh_cross_lngrad(&g, order, jobs.data(), (int)jobs.size(), nullptr));
        mhh_check(mhh_synchronize(nullptr));
        if (hipMemcpy(packed.data(), out, total*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
    }

    // a packed plane back at the places of the ghosted host field `fld` where the writer of its kind reads it
    template<typename TF, class GD>
    void mhh_place(const GD& gd, const Plane& p, const TF* packed, TF* fld)
    {
        const int jj = gd.icells, kk = gd.ijcells;
        const TF* src = packed + p.pos;
        if (p.kind == MHH_CROSS_XY || p.kind == MHH_CROSS_PLANE)
        {
            const int k = (p.kind == MHH_CROSS_XY) ? p.index : 0;
            for (int j=0; j<gd.jmax; ++j)
                for (int i=0; i<gd.imax; ++i)
                    fld[i+gd.igc + (j+gd.jgc)*jj + k*kk] = src[i + j*gd.imax];
        }
        else if (p.kind == MHH_CROSS_XZ)
            for (int k=p.k0; k<p.k1; ++k)
                for (int i=0; i<gd.imax; ++i)
                    fld[i+gd.igc + p.index*jj + k*kk] = src[i + (k-p.k0)*gd.imax];
        else
            for (int k=p.k0; k<p.k1; ++k)
                for (int j=0; j<gd.jmax; ++j)
                    fld[p.index + (j+gd.jgc)*jj + k*kk] = src[j + (k-p.k0)*gd.jmax];
    }

    // The sections of one variable over its three index lists: fetched in one launch and one copy, written by the reference's
    // writers. A row of an xz section lives on the rank mpicoordy == j / jmax (save_xz_slice, src/field3d_io.cxx:251-258); the
    // serial writer reads row j + jgc, the north ghost row for j == jtot (:774). Every rank calls every writer: they are collective.
    template<typename TF>
    int mhh_sections(Master& master, Grid<TF>& grid, Fields<TF>& fields, Field3d_io<TF>& io, TF* data_g, TF offset, const std::string& name, int iotime,
                     int order, const std::vector<int>& jlist, const std::vector<int>& ilist, const std::vector<int>& klist)
    {
        auto& gd = grid.get_grid_data();
        auto& md = master.get_MPI_data();
        mhh_grid g = mhh_make_grid(gd, md);
        const bool serial = (md.npx*md.npy == 1);
        std::vector<Plane> planes; std::vector<int> jplane(jlist.size(), -1), iplane(ilist.size(), -1), kplane(klist.size(), -1);
        size_t pos = 0;
        auto add = [&](int kind, int index) { planes.push_back(mhh_plane<TF>(gd, kind, index, pos)); pos += planes.back().cells; return (int)planes.size() - 1; };
        for (size_t n=0; n<jlist.size(); ++n)
            if (serial || md.mpicoordy == jlist[n]/gd.jmax)
                jplane[n] = add(MHH_CROSS_XZ, (serial ? jlist[n] : jlist[n] % gd.jmax) + gd.jgc);
        for (size_t n=0; n<ilist.size(); ++n)
            iplane[n] = add(MHH_CROSS_YZ, ilist[n] % gd.imax + gd.igc);
        for (size_t n=0; n<klist.size(); ++n)
            kplane[n] = add(MHH_CROSS_XY, klist[n] + gd.kgc);
        std::vector<TF> packed;
        mhh_fetch<TF>(g, data_g, planes, order, packed);

        int nerror = 0;
        char filename[256];
        auto hostfld = fields.get_tmp();
        auto tmpfld = fields.get_tmp();
        TF* host = hostfld->fld.data();
        TF* tmp = tmpfld->fld.data();
        auto failed = [&](int error) { if (error) master.print_message("Saving \"%s\" ... FAILED\n", filename); return error ? 1 : 0; };
        for (size_t n=0; n<jlist.size(); ++n)
        {
            if (jplane[n] >= 0) mhh_place(gd, planes[jplane[n]], packed.data(), host);
            std::snprintf(filename, sizeof(filename), "%s.%s.%05d.%07d", name.c_str(), "xz", jlist[n], iotime);
            nerror += failed(io.save_xz_slice(host, offset, tmp, filename, jlist[n], gd.kstart, gd.kend));
        }
        for (size_t n=0; n<ilist.size(); ++n)
        {
            mhh_place(gd, planes[iplane[n]], packed.data(), host);
            std::snprintf(filename, sizeof(filename), "%s.%s.%05d.%07d", name.c_str(), "yz", ilist[n], iotime);
            nerror += failed(io.save_yz_slice(host, offset, tmp, filename, ilist[n], gd.kstart, gd.kend));
        }
        for (size_t n=0; n<klist.size(); ++n)
        {
            mhh_place(gd, planes[kplane[n]], packed.data(), host);
            std::snprintf(filename, sizeof(filename), "%s.%s.%05d.%07d", name.c_str(), "xy", klist[n], iotime);
            nerror += failed(io.save_xy_slice(host, offset, tmp, filename, klist[n] + gd.kgc));
        }
        fields.release_tmp(tmpfld);
        fields.release_tmp(hostfld);
        return nerror;
    }

    // one 2-D array that is on the device already, packed [jmax][imax] at `packed_g` or ghosted [ijcells] at `plane_g`: to the host,
    // then Cross::cross_plane's write (src/cross.cxx:638-651)
    template<typename TF>
    int mhh_write_plane(Master& master, Grid<TF>& grid, Fields<TF>& fields, Field3d_io<TF>& io, const TF* plane_g, const TF* packed_g, TF offset,
                        const std::string& name, int iotime)
    {
        auto& gd = grid.get_grid_data();
        mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
        const Plane p = mhh_plane<TF>(gd, MHH_CROSS_PLANE, 0, 0);
        std::vector<TF> packed(p.cells);
        if (plane_g)
            mhh_fetch<TF>(g, plane_g, {p}, 0, packed);
        else
        {
            mhh_check(mhh_synchronize(nullptr));
            if (hipMemcpy(packed.data(), packed_g, p.cells*sizeof(TF), 2) != 0) throw std::runtime_error("hipMemcpy");
        }
        auto hostfld = fields.get_tmp();
        auto tmpfld = fields.get_tmp();
        mhh_place(gd, p, packed.data(), hostfld->fld.data());
        char filename[256];
        std::snprintf(filename, sizeof(filename), "%s.%s.%07d", name.c_str(), "xy", iotime);
        int nerror = io.save_xy_slice(hostfld->fld.data(), offset, tmpfld->fld.data(), filename);
        if (nerror) master.print_message("Saving \"%s\" ... FAILED\n", filename);
        fields.release_tmp(tmpfld);
        fields.release_tmp(hostfld);
        return nerror ? 1 : 0;
    }
}

// data: the DEVICE pointer of the field
template<typename TF>
int Cross<TF>::cross_simple(TF* restrict data, TF restrict offset, const std::string& name, const int iotime, const std::array<int,3>& loc)
{
    auto& gd = grid.get_grid_data();
    return mhh_sections<TF>(master, grid, fields, field3d_io, data, offset, name, iotime, 0,
                            loc == gd.vloc ? jxzh : jxz, loc == gd.uloc ? ixzh : ixz, loc == gd.wloc ? kxyh : kxy);
}

// data: the DEVICE pointer of a 2-D array [ijcells]
template<typename TF>
int Cross<TF>::cross_plane(TF* restrict data, TF restrict offset, std::string name, int iotime)
{
    return mhh_write_plane<TF>(master, grid, fields, field3d_io, data, nullptr, offset, name, iotime);
}

// calc_lngrad_2nd / calc_lngrad_4th on the cells of the sections alone; a: the DEVICE pointer, its ghost cells filled
template<typename TF>
int Cross<TF>::cross_lngrad(TF* restrict a, std::string name, int iotime)
{
    const int order = (grid.get_spatial_order() == Grid_order::Second) ? 2 : 4;
    TF no_offset = 0;
    return mhh_sections<TF>(master, grid, fields, field3d_io, a, no_offset, name, iotime, order, jxz, ixz, kxy);
}

template<typename TF>
int Cross<TF>::cross_path(TF* restrict data, std::string name, int iotime)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    TF* out = static_cast<TF*>(mhh_staging((size_t)gd.imax*gd.jmax*sizeof(TF)));
    mhh_check(mhh_cross_path(&g, data, fields.rhoref_g, out, nullptr));
    TF no_offset = 0.;
    return mhh_write_plane<TF>(master, grid, fields, field3d_io, nullptr, out, no_offset, name, iotime);
}

template<typename TF>
int Cross<TF>::cross_height_threshold(TF* restrict data, TF threshold, Cross_direction direction, std::string name, int iotime)
{
    auto& gd = grid.get_grid_data();
    mhh_grid g = mhh_make_grid(gd, master.get_MPI_data());
    TF* out = static_cast<TF*>(mhh_staging((size_t)gd.imax*gd.jmax*sizeof(TF)));
    mhh_check(mhh_cross_height_threshold(&g, data, threshold, direction == Cross_direction::Bottom_to_top, out, nullptr));
    TF no_offset = 0.;
    return mhh_write_plane<TF>(master, grid, fields, field3d_io, nullptr, out, no_offset, name, iotime);
}

// the members alone: the class itself is instantiated by src/cross.cxx
#define MHH_CROSS_MEMBERS(TF) \
    template int Cross<TF>::cross_simple(TF*, const TF, const std::string&, const int, const std::array<int,3>&); \
    template int Cross<TF>::cross_plane(TF*, const TF, std::string, int); \
    template int Cross<TF>::cross_lngrad(TF*, std::string, int); \
    template int Cross<TF>::cross_path(TF*, std::string, int); \
    template int Cross<TF>::cross_height_threshold(TF*, TF, Cross_direction, std::string, int);
MHH_CROSS_MEMBERS(double)
MHH_CROSS_MEMBERS(float)
#endif
