// ref_force_shim.cpp -- TEST infrastructure: the kernels of the reference's force.cxx and buffer.cxx behind a C interface.
//
// Compiled by tests/pres_ref.py together with ref_pres_shim.cpp, as a translation unit of its own (include/finite_difference.h has no
// include guard). The kernels live in the anonymous namespaces of the included files and need nothing of the seam; the class members,
// which do, are discarded at link time. One entry point per kernel, with the argument lists of Force::exec (src/force.cxx:581-729) and
// Buffer::exec (src/buffer.cxx:163-206); the caller puts them in that order.
#include "force.cxx"
#include "buffer.cxx"

#include "mhh_hip.h"

namespace
{
    template<class TF> TF* M(void* p) { return static_cast<TF*>(p); }
    template<class TF> const TF* K(const void* p) { return static_cast<const TF*>(p); }
}
#define REF_API extern "C" __attribute__((visibility("default")))
#define BY_TYPE(g, ...) do { if ((g)->dtype == MHH_F64) { typedef double TF; __VA_ARGS__; } else { typedef float TF; __VA_ARGS__; } } while (0)
#define BOUNDS(g) (g)->istart, (g)->iend, (g)->jstart, (g)->jend, (g)->kstart, (g)->kend, (g)->icells, (g)->ijcells

// swlspres = dpdx: fbody = TF(-1.)*dpdx at the call site
REF_API void ref_force_dpdx(const mhh_grid* g, void* ut, double dpdx)
{
    BY_TYPE(g, const TF fbody = TF(-1.)*TF(dpdx); add_pressure_force<TF>(M<TF>(ut), fbody, BOUNDS(g)));
}
REF_API void ref_force_fixed_flux(const mhh_grid* g, void* ut, double uflux, double u_mean, double ut_mean, double utrans, double dt)
{
    BY_TYPE(g, enforce_fixed_flux<TF>(M<TF>(ut), TF(uflux), TF(u_mean), TF(ut_mean), TF(utrans), TF(dt), BOUNDS(g)));
}
REF_API void ref_force_coriolis(const mhh_grid* g, int order, void* ut, void* vt, const void* u, const void* v, const void* ug, const void* vg,
                                double fc, double utrans, double vtrans)
{
    BY_TYPE(g,
        if (order == 2) calc_coriolis_2nd<TF>(M<TF>(ut), M<TF>(vt), K<TF>(u), K<TF>(v), K<TF>(ug), K<TF>(vg), TF(fc), TF(utrans), TF(vtrans), BOUNDS(g));
        else            calc_coriolis_4th<TF>(M<TF>(ut), M<TF>(vt), K<TF>(u), K<TF>(v), K<TF>(ug), K<TF>(vg), TF(fc), TF(utrans), TF(vtrans), BOUNDS(g)));
}
REF_API void ref_force_large_scale_source(const mhh_grid* g, void* st, const void* sls)
{
    BY_TYPE(g, calc_large_scale_source<TF>(M<TF>(st), K<TF>(sls), BOUNDS(g)));
}
REF_API void ref_force_nudging(const mhh_grid* g, void* tend, const void* mean, const void* ref, const void* factor)
{
    BY_TYPE(g, calc_nudging_tendency<TF>(M<TF>(tend), K<TF>(mean), K<TF>(ref), K<TF>(factor), BOUNDS(g)));
}
// kind 0: advec_wls_2nd_mean (s = the mean profile), 1: advec_wls_2nd_local, 2: advec_wls_2nd_local_w (which takes dzi)
REF_API void ref_force_wls(const mhh_grid* g, int kind, void* st, const void* s, const void* wls)
{
    BY_TYPE(g,
        if (kind == 0)      advec_wls_2nd_mean<TF>(M<TF>(st), K<TF>(s), K<TF>(wls), K<TF>(g->dzhi), BOUNDS(g));
        else if (kind == 1) advec_wls_2nd_local<TF>(M<TF>(st), K<TF>(s), K<TF>(wls), K<TF>(g->dzhi), BOUNDS(g));
        else                advec_wls_2nd_local_w<TF>(M<TF>(st), K<TF>(s), K<TF>(wls), K<TF>(g->dzi), BOUNDS(g)));
}
// half = 0: z, bufferkstart; 1: zh, bufferkstarth (the w call of Buffer::exec)
REF_API void ref_buffer(const mhh_grid* g, int half, void* at, const void* a, const void* abuf, double zstart, double beta, double sigma, int bufferkstart)
{
    BY_TYPE(g, calc_buffer<TF>(M<TF>(at), K<TF>(a), K<TF>(abuf), K<TF>(half ? g->zh : g->z), TF(zstart), TF(g->zsize), TF(beta), TF(sigma),
                               g->istart, g->iend, g->icells, g->jstart, g->jend, g->ijcells, bufferkstart, g->kend));
}
