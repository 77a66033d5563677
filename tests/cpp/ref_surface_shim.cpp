// ref_surface_shim.cpp -- TEST infrastructure: the reference's own surface-layer templates behind a C interface.
//
// Compiled by tests/surface_ref.py (tests/refshim.py holds the command) into a temporary directory with the reference's include
// directory on the include path; nothing compiled from it is kept. What comes from the reference
// at compile time: Boundary_surface_kernels (prepare_lut, calc_dutot, the lookup solvers, calc_duvdz_mo, calc_dbdz_mo) and
// Monin_obukhov. What is written here: four stub lines that let that header compile alone, a Boundary_cyclic whose exec_2d wraps a
// 2-D array, the file-local loops of src/boundary_surface.cxx (stability, stability_neutral, surfm, surfs) and of
// src/thermo_dry.cxx (the buoyancy hooks), which sit in anonymous namespaces and cannot be linked -- restated with the
// reference's expressions in its order -- and Boundary_surface::exec's call sequence (src/boundary_surface.cxx:830-983).
//
// The 3-D fields arrive as their level kstart only ([jcells][icells]); the loops run with kstart = 0.
#include <algorithm>
#include <cmath>
#include <vector>

#define restrict __restrict__
enum class Boundary_type {Dirichlet_type, Neumann_type, Flux_type, Ustar_type, Off_type};
const int nzL_lut = 10000;
template<typename TF> struct Boundary_cyclic
{
    int igc, jgc, istart, iend, jstart, jend, icells, jcells, jtot;
    void exec_2d(TF* a)
    {
        for (int j=0; j<jcells; ++j)
            for (int i=0; i<igc; ++i)
            {
                a[i + j*icells] = a[iend-igc+i + j*icells];
                a[iend+i + j*icells] = a[istart+i + j*icells];
            }
        for (int i=0; i<icells; ++i)
            for (int j=0; j<jgc; ++j)
            {
                if (jtot == 1) { a[i + j*icells] = a[i + jstart*icells]; a[i + (jend+j)*icells] = a[i + jstart*icells]; }
                else { a[i + j*icells] = a[i + (jend-jgc+j)*icells]; a[i + (jend+j)*icells] = a[i + (jstart+j)*icells]; }
            }
    }
};
#include "boundary_surface_kernels.h"
#include "ref_shim.h"

namespace bsk = Boundary_surface_kernels;
namespace most = Monin_obukhov;

#define MAXS 8
extern "C" struct ref_surface_io
{
    int dtype;                                   // 0 double, 1 float
    int itot, jtot, igc, jgc;
    int mbcbot, thermobc, thermo_kind, thermo_index, nscalars, skip_dutot;
    int sbcbot[MAXS];
    double zsl, thref, threfh, grav, n2;
    const float* zL; const float* f;
    void* u; void* v; void* s[MAXS];             // level kstart
    void* ubot; void* vbot; void* z0m; void* z0h;
    void* dutot; void* ustar; void* obuk; int* nobuk;
    void* ufluxbot; void* vfluxbot; void* ugradbot; void* vgradbot;
    void* sbot[MAXS]; void* sgradbot[MAXS]; void* sfluxbot[MAXS];
    void* dudz; void* dvdz; void* dbdz;
};

namespace
{
template<typename TF> TF* P(void* p) { return static_cast<TF*>(p); }

// src/boundary_surface.cxx:54-134, the lookup solver (sw_constant_z0 = true)
template<typename TF>
void stability(TF* ustar, TF* obuk, const TF* bfluxbot, const TF* b, const TF* bbot, const TF* dutot, const TF* z, const TF* z0m,
               const float* zL_sl, const float* f_sl, int* nobuk, const TF db_ref, const int kstart, const int ncol, const int kk,
               Boundary_type mbcbot, Boundary_type thermobc)
{
    if (mbcbot == Boundary_type::Ustar_type && thermobc == Boundary_type::Flux_type)
        for (int ij=0; ij<ncol; ++ij)
            obuk[ij] = -Fast_math::pow3(ustar[ij]) / (Constants::kappa<TF>*bfluxbot[ij]);
    else if (mbcbot == Boundary_type::Dirichlet_type && thermobc == Boundary_type::Flux_type)
        for (int ij=0; ij<ncol; ++ij)
        {
            obuk[ij] = bsk::calc_obuk_noslip_flux_lookup(zL_sl, f_sl, nobuk[ij], dutot[ij], bfluxbot[ij], z[kstart]);
            ustar[ij] = dutot[ij] * most::fm(z[kstart], z0m[ij], obuk[ij]);
        }
    else if (mbcbot == Boundary_type::Dirichlet_type && thermobc == Boundary_type::Dirichlet_type)
        for (int ij=0; ij<ncol; ++ij)
        {
            const TF db = b[ij + kstart*kk] - bbot[ij] + db_ref;
            obuk[ij] = bsk::calc_obuk_noslip_dirichlet_lookup(zL_sl, f_sl, nobuk[ij], dutot[ij], db, z[kstart]);
            ustar[ij] = dutot[ij] * most::fm(z[kstart], z0m[ij], obuk[ij]);
        }
}

// :137-177
template<typename TF>
void stability_neutral(TF* ustar, TF* obuk, const TF* dutot, const TF* z, const TF* z0m, const Boundary_cyclic<TF>& g, const int kstart,
                       Boundary_type mbcbot)
{
    if (mbcbot == Boundary_type::Ustar_type)
    {
        for (int j=g.jstart; j<g.jend; ++j)
            for (int i=g.istart; i<g.iend; ++i)
                obuk[i + j*g.icells] = -Constants::dbig;
    }
    else if (mbcbot == Boundary_type::Dirichlet_type)
        for (int ij=0; ij<g.icells*g.jcells; ++ij)
        {
            obuk [ij] = -Constants::dbig;
            ustar[ij] = dutot[ij] * most::fm(z[kstart], z0m[ij], obuk[ij]);
        }
}

// :180-288
template<typename TF>
void surfm(TF* ufluxbot, TF* vfluxbot, TF* ugradbot, TF* vgradbot, const TF* ustar, const TF* obuk, const TF* u, const TF* ubot,
           const TF* v, const TF* vbot, const TF* z0m, const TF zsl, const Boundary_type bcbot, Boundary_cyclic<TF>& g, const int kstart,
           const int kk)
{
    const int ii = 1, jj = g.icells;
    if (bcbot == Boundary_type::Dirichlet_type)
    {
        for (int j=g.jstart; j<g.jend; ++j)
            for (int i=g.istart; i<g.iend; ++i)
            {
                const int ij = i + j*jj, ijk = ij + kstart*kk;
                ufluxbot[ij] = -(u[ijk]-ubot[ij])*TF(0.5)*
                    (ustar[ij-ii]*most::fm(zsl, z0m[ij-ii], obuk[ij-ii]) + ustar[ij]*most::fm(zsl, z0m[ij], obuk[ij]));
                vfluxbot[ij] = -(v[ijk]-vbot[ij])*TF(0.5)*
                    (ustar[ij-jj]*most::fm(zsl, z0m[ij-jj], obuk[ij-jj]) + ustar[ij]*most::fm(zsl, z0m[ij], obuk[ij]));
            }
        g.exec_2d(ufluxbot);
        g.exec_2d(vfluxbot);
    }
    else if (bcbot == Boundary_type::Ustar_type)
    {
        const TF minval = 1.e-2;
        for (int j=g.jstart; j<g.jend; ++j)
            for (int i=g.istart; i<g.iend; ++i)
            {
                const int ij = i + j*jj, ijk = ij + kstart*kk;
                const TF vonu2 = std::max(minval, TF(0.25)*(
                            Fast_math::pow2(v[ijk-ii]-vbot[ij-ii]) + Fast_math::pow2(v[ijk-ii+jj]-vbot[ij-ii+jj])
                          + Fast_math::pow2(v[ijk   ]-vbot[ij   ]) + Fast_math::pow2(v[ijk   +jj]-vbot[ij   +jj])) );
                const TF uonv2 = std::max(minval, TF(0.25)*(
                            Fast_math::pow2(u[ijk-jj]-ubot[ij-jj]) + Fast_math::pow2(u[ijk+ii-jj]-ubot[ij+ii-jj])
                          + Fast_math::pow2(u[ijk   ]-ubot[ij   ]) + Fast_math::pow2(u[ijk+ii   ]-ubot[ij+ii   ])) );
                const TF u2 = std::max(minval, Fast_math::pow2(u[ijk]-ubot[ij]) );
                const TF v2 = std::max(minval, Fast_math::pow2(v[ijk]-vbot[ij]) );
                const TF ustaronu4 = TF(0.5)*(Fast_math::pow4(ustar[ij-ii]) + Fast_math::pow4(ustar[ij]));
                const TF ustaronv4 = TF(0.5)*(Fast_math::pow4(ustar[ij-jj]) + Fast_math::pow4(ustar[ij]));
                ufluxbot[ij] = -copysign(TF(1), u[ijk]-ubot[ij]) * std::pow(ustaronu4 / (TF(1) + vonu2 / u2), TF(0.5));
                vfluxbot[ij] = -copysign(TF(1), v[ijk]-vbot[ij]) * std::pow(ustaronv4 / (TF(1) + uonv2 / v2), TF(0.5));
            }
        g.exec_2d(ufluxbot);
        g.exec_2d(vfluxbot);
    }
    for (int ij=0; ij<g.icells*g.jcells; ++ij)
    {
        const int ijk = ij + kstart*kk;
        ugradbot[ij] = (u[ijk]-ubot[ij])/zsl;
        vgradbot[ij] = (v[ijk]-vbot[ij])/zsl;
    }
}

// :291-339
template<typename TF>
void surfs(TF* varbot, TF* vargradbot, TF* varfluxbot, const TF* ustar, const TF* obuk, const TF* var, const TF* z0h, const TF zsl,
           const Boundary_type bcbot, const int kstart, const int ncol, const int kk)
{
    if (bcbot == Boundary_type::Dirichlet_type)
        for (int ij=0; ij<ncol; ++ij)
        {
            const int ijk = ij + kstart*kk;
            varfluxbot[ij] = -(var[ijk]-varbot[ij])*ustar[ij]*most::fh(zsl, z0h[ij], obuk[ij]);
            vargradbot[ij] = (var[ijk]-varbot[ij])/zsl;
        }
    else if (bcbot == Boundary_type::Flux_type)
        for (int ij=0; ij<ncol; ++ij)
        {
            const int ijk = ij + kstart*kk;
            varbot[ij] = varfluxbot[ij] / (ustar[ij]*most::fh(zsl, z0h[ij], obuk[ij])) + var[ijk];
            vargradbot[ij] = (var[ijk]-varbot[ij])/zsl;
        }
}

// Thermo::get_buoyancy_surf / get_buoyancy_fluxbot / get_db_ref: Thermo_dry (src/thermo_dry.cxx:133-162,629-633) or Thermo_buoy's
// copies (src/thermo_buoy.cxx:425-448, include/thermo_buoy.h:66)
template<typename TF>
void buoyancy_fluxbot(std::vector<TF>& bfluxbot, const TF* thfluxbot, const ref_surface_io& io)
{
    const TF grav = io.grav, threfh = io.threfh;
    for (size_t ij=0; ij<bfluxbot.size(); ++ij)
        bfluxbot[ij] = (io.thermo_kind == 1) ? grav/threfh*thfluxbot[ij] : thfluxbot[ij];
}
template<typename TF>
TF buoyancy_surf(std::vector<TF>& b, std::vector<TF>& bbot, const TF* th, const TF* thbot, const ref_surface_io& io)
{
    const TF grav = io.grav, thref = io.thref, threfh = io.threfh;
    for (size_t ij=0; ij<b.size(); ++ij)
    {
        bbot[ij] = (io.thermo_kind == 1) ? grav/threfh * (thbot[ij] - threfh) : thbot[ij];
        b[ij]    = (io.thermo_kind == 1) ? grav/thref  * (th[ij]    - thref ) : th[ij];
    }
    return (io.thermo_kind == 1) ? grav/thref*(thref - threfh) : TF(io.n2);
}

// Boundary_surface<TF>::exec (src/boundary_surface.cxx:830-983), sw_constant_z0, no Charnock
template<typename TF>
void exec(const ref_surface_io& io)
{
    Boundary_cyclic<TF> g;
    g.igc = io.igc; g.jgc = io.jgc; g.istart = io.igc; g.jstart = io.jgc; g.iend = io.igc + io.itot; g.jend = io.jgc + io.jtot;
    g.icells = io.itot + 2*io.igc; g.jcells = io.jtot + 2*io.jgc; g.jtot = io.jtot;
    const int ncol = g.icells*g.jcells, kstart = 0, kk = ncol;
    const TF zsl = io.zsl;
    const TF* z = &zsl;
    const Boundary_type mbcbot = static_cast<Boundary_type>(io.mbcbot), thermobc = static_cast<Boundary_type>(io.thermobc);
    TF* dutot = P<TF>(io.dutot);
    const TF* u = P<TF>(io.u); const TF* v = P<TF>(io.v); const TF* ubot = P<TF>(io.ubot); const TF* vbot = P<TF>(io.vbot);
    const TF* z0m = P<TF>(io.z0m); const TF* z0h = P<TF>(io.z0h);
    TF* ustar = P<TF>(io.ustar); TF* obuk = P<TF>(io.obuk);

    if (!io.skip_dutot)
        bsk::calc_dutot(dutot, u, v, ubot, vbot, g.istart, g.iend, g.jstart, g.jend, kstart, g.icells, g.jcells, ncol, g);

    const int t = io.thermo_index;
    std::vector<TF> b(ncol), bbot(ncol), bfluxbot(ncol);
    if (io.thermo_kind == 0)
        stability_neutral(ustar, obuk, dutot, z, z0m, g, kstart, mbcbot);
    else
    {
        const TF db_ref = buoyancy_surf(b, bbot, P<TF>(io.s[t]), P<TF>(io.sbot[t]), io);
        buoyancy_fluxbot(bfluxbot, P<TF>(io.sfluxbot[t]), io);
        stability(ustar, obuk, bfluxbot.data(), b.data(), bbot.data(), dutot, z, z0m, io.zL, io.f, io.nobuk, db_ref, kstart, ncol, kk,
                  mbcbot, thermobc);
    }
    surfm(P<TF>(io.ufluxbot), P<TF>(io.vfluxbot), P<TF>(io.ugradbot), P<TF>(io.vgradbot), ustar, obuk, u, ubot, v, vbot, z0m, zsl, mbcbot,
          g, kstart, kk);
    for (int n=0; n<io.nscalars; ++n)
        surfs(P<TF>(io.sbot[n]), P<TF>(io.sgradbot[n]), P<TF>(io.sfluxbot[n]), ustar, obuk, P<TF>(io.s[n]), z0h, zsl,
              static_cast<Boundary_type>(io.sbcbot[n]), kstart, ncol, kk);
    bsk::calc_duvdz_mo(P<TF>(io.dudz), P<TF>(io.dvdz), u, v, ubot, vbot, P<TF>(io.ufluxbot), P<TF>(io.vfluxbot), ustar, obuk, z0m, zsl,
                       g.istart, g.iend, g.jstart, g.jend, kstart, g.icells, ncol);
    if (io.thermo_kind != 0)
    {
        buoyancy_fluxbot(bfluxbot, P<TF>(io.sfluxbot[t]), io);
        bsk::calc_dbdz_mo(P<TF>(io.dbdz), bfluxbot.data(), ustar, obuk, zsl, g.istart, g.iend, g.jstart, g.jend, g.icells);
    }
}
}

REF_API void ref_surface_exec(const ref_surface_io* io)
{
    if (io->dtype == 0) exec<double>(*io); else exec<float>(*io);
}
// Boundary_surface::init_solver (:812-826)
REF_API void ref_surface_lut(double zsl, double z0m, double z0h, int mbcbot, int thermobc, int dtype, float* zL, float* f)
{
    const Boundary_type m = static_cast<Boundary_type>(mbcbot), t = static_cast<Boundary_type>(thermobc);
    if (dtype == 0) bsk::prepare_lut<double>(zL, f, z0m, z0h, zsl, nzL_lut, m, t);
    else            bsk::prepare_lut<float>(zL, f, (float)z0m, (float)z0h, (float)zsl, nzL_lut, m, t);
}
