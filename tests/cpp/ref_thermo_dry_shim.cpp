// ref_thermo_dry_shim.cpp -- TEST infrastructure: the buoyancy kernels of the reference's thermo_dry.cxx behind a C interface.
//
// Compiled by tests/pres_ref.py together with ref_pres_shim.cpp (a translation unit of its own: include/finite_difference.h has no
// include guard, so thermo_dry.cxx and pres_4.cxx cannot share one). The kernels live in the anonymous namespace of the included file
// and need nothing of the seam; the class members, which do, are discarded at link time.
#include "thermo_dry.cxx"

#include "mhh_hip.h"

namespace
{
    template<class TF> TF* M(void* p) { return static_cast<TF*>(p); }
    template<class TF> const TF* K(const void* p) { return static_cast<const TF*>(p); }
}
#define REF_API extern "C" __attribute__((visibility("default")))
#define BY_TYPE(g, ...) do { if ((g)->dtype == MHH_F64) { typedef double TF; __VA_ARGS__; } else { typedef float TF; __VA_ARGS__; } } while (0)

// argument lists of Thermo_dry::exec, get_thermo_field, get_buoyancy_surf and get_buoyancy_fluxbot (src/thermo_dry.cxx:465-585)
REF_API double ref_thermo_dry_grav(void) { return Constants::grav<double>; }
REF_API void ref_buoyancy_tend(const mhh_grid* g, int order, void* wt, const void* th, const void* threfh)
{
    BY_TYPE(g,
        if (order == 2) calc_buoyancy_tend_2nd<TF>(M<TF>(wt), K<TF>(th), K<TF>(threfh), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells);
        else            calc_buoyancy_tend_4th<TF>(M<TF>(wt), K<TF>(th), K<TF>(threfh), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells));
}
REF_API void ref_calc_N2(const mhh_grid* g, void* N2, const void* th, const void* thref)
{
    BY_TYPE(g, calc_N2<TF>(M<TF>(N2), K<TF>(th), K<TF>(g->dzi), K<TF>(thref), g->istart, g->iend, g->jstart, g->jend, g->kstart, g->kend, g->icells, g->ijcells, g->kcells));
}
REF_API void ref_buoyancy_bot(const mhh_grid* g, void* b, void* bbot, const void* th, const void* thbot, const void* thref, const void* threfh)
{
    BY_TYPE(g, calc_buoyancy_bot<TF>(M<TF>(b), M<TF>(bbot), K<TF>(th), K<TF>(thbot), K<TF>(thref), K<TF>(threfh), g->icells, g->jcells, g->kstart, g->ijcells));
}
REF_API void ref_buoyancy_fluxbot(const mhh_grid* g, void* bfluxbot, const void* thfluxbot, const void* threfh)
{
    BY_TYPE(g, calc_buoyancy_fluxbot<TF>(M<TF>(bfluxbot), K<TF>(thfluxbot), K<TF>(threfh), g->icells, g->jcells, g->kstart, g->ijcells));
}
