// ref_source_shim.cpp -- TEST infrastructure: the reference's own Source and Decay kernels behind a C interface.
//
// Compiled by tests/source_ref.py into a temporary directory with the reference's src and include directories and
// tests/stubs_syntax_only on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__, sections
// collected at link time, together with the reference's master.cxx and master_serial.cxx); nothing compiled from it is kept. The
// translation units are included in place and unmodified, so that the functions of their anonymous namespaces (calc_shape,
// calc_shape_profile, calc_source, enforce_exponential_decay) are visible here. What is written here is the calls only, with the
// arguments Source::create (:289-316), Source::exec (:403-431) and Decay::exec (:97-111) pass.
//
// Source::calc_norm is a private member that reads grid.get_grid_data() and calls master.sum. The seam, written here from scratch:
// Grid::get_grid_data (a Grid_data filled from the test's arrays), Input::get_item<bool> (the constructor's one read: it answers
// the default, swsource = false, after which the constructor reads nothing), a Master of one rank, and Grid, Fields and Input objects
// that are never constructed because no member of theirs is read. The private member is reached through explicit instantiation
// (which may name it), not by editing or redefining anything of the reference's.
#include "source.cxx"
#include "decay.cxx"
#include "ref_shim.h"

#include <cstdlib>
#include <cstring>
#include <new>

namespace seam
{
    template<class Tag> struct Slot { static typename Tag::type ptr; };
    template<class Tag> typename Tag::type Slot<Tag>::ptr;
    template<class Tag, typename Tag::type P> struct Bind { Bind() { Slot<Tag>::ptr = P; } static Bind self; };
    template<class Tag, typename Tag::type P> Bind<Tag, P> Bind<Tag, P>::self;
    template<class Tag> typename Tag::type get() { return Slot<Tag>::ptr; }

    struct Master_md { typedef MPI_data Master::* type; };
    template struct Bind<Master_md, &Master::md>;

    template<class TF> struct Norm
    {
        typedef TF (Source<TF>::*type)(const TF* const, const TF, const TF, const TF, const TF* const, const TF, const TF, const TF,
                                       const TF* const, const TF, const TF, const TF, const TF* const,
                                       std::vector<int>, std::vector<int>, std::vector<int>, const TF* const, const bool, const bool);
    };
    template struct Bind<Norm<double>, &Source<double>::calc_norm>;
    template struct Bind<Norm<float>, &Source<float>::calc_norm>;

    template<class TF> Grid_data<TF>& grid_data() { static Grid_data<TF> gd; return gd; }

    // storage of an object that is never constructed and never read, filled with 0xA5 so that a read would show at once
    template<class T> T* blank()
    {
        void* raw = std::malloc(sizeof(T));
        std::memset(raw, 0xA5, sizeof(T));
        return static_cast<T*>(raw);
    }

    Master& master()
    {
        static Master* m = nullptr;     // never destroyed: the destructor prints
        if (!m)
        {
            m = new (std::calloc(1, sizeof(Master))) Master;
            MPI_data& md = m->*get<Master_md>();
            md.nprocs = 1; md.npx = 1; md.npy = 1; md.mpiid = 0; md.mpicoordx = 0; md.mpicoordy = 0;
        }
        return *m;
    }
}

template<typename TF> const Grid_data<TF>& Grid<TF>::get_grid_data() { return seam::grid_data<TF>(); }
template const Grid_data<double>& Grid<double>::get_grid_data();
template const Grid_data<float>&  Grid<float>::get_grid_data();

// Source's constructor asks for [source] swsource with the default 0; the answer is the default
template<> bool Input::get_item<bool>(const std::string&, const std::string&, const std::string&, const bool value) { return value; }
// behind `if (swsource)`: never reached
namespace seam { [[noreturn]] void never(const char* what) { std::fprintf(stderr, "ref_source_shim: %s is outside the seam\n", what); std::abort(); } }
#define SEAM_NO_LIST(T) template<> std::vector<T> Input::get_list<T>(const std::string&, const std::string&, const std::string&) { seam::never("Input::get_list"); }
SEAM_NO_LIST(std::string) SEAM_NO_LIST(double) SEAM_NO_LIST(float) SEAM_NO_LIST(bool) SEAM_NO_LIST(int)

namespace
{
    template<class TF> const TF* K(const void* p) { return static_cast<const TF*>(p); }

    struct Desc { double x0, y0, z0, sigma_x, sigma_y, sigma_z, line_x, line_y, line_z, strength; int swvmr, use_profile; };

    template<class TF>
    void shape(const Dims& d, const Desc& s, const void* x, const void* y, const void* z, const void* prof, int* r)
    {
        std::vector<int> rx = calc_shape<TF>(K<TF>(x), TF(s.x0), TF(s.sigma_x), TF(s.line_x), d.istart, d.iend);
        std::vector<int> ry = calc_shape<TF>(K<TF>(y), TF(s.y0), TF(s.sigma_y), TF(s.line_y), d.jstart, d.jend);
        std::vector<int> rz = s.use_profile ? calc_shape_profile<TF>(K<TF>(prof), K<TF>(z), d.kstart, d.kend)
                                            : calc_shape<TF>(K<TF>(z), TF(s.z0), TF(s.sigma_z), TF(s.line_z), d.kstart, d.kend);
        r[0] = rx[0]; r[1] = rx[1]; r[2] = ry[0]; r[3] = ry[1]; r[4] = rz[0]; r[5] = rz[1];
    }

    template<class TF>
    double norm(const Dims& d, const Desc& s, const void* x, const void* y, const void* z, const void* dz, double dx, double dy,
                const void* prof, const int* r, const void* rhoref)
    {
        Grid_data<TF>& gd = seam::grid_data<TF>();
        gd.istart = d.istart; gd.iend = d.iend; gd.jstart = d.jstart; gd.jend = d.jend; gd.kstart = d.kstart; gd.kend = d.kend;
        gd.icells = d.icells; gd.ijcells = d.ijcells; gd.kcells = d.kcells;
        gd.dx = TF(dx); gd.dy = TF(dy);
        gd.dz.assign(K<TF>(dz), K<TF>(dz) + d.kcells);
        static Source<TF>* src = nullptr;       // never destroyed
        if (!src)
            src = new Source<TF>(seam::master(), *seam::blank<Grid<TF>>(), *seam::blank<Fields<TF>>(), *seam::blank<Input>());
        return (src->*seam::get<seam::Norm<TF>>())(
                K<TF>(x), TF(s.x0), TF(s.sigma_x), TF(s.line_x), K<TF>(y), TF(s.y0), TF(s.sigma_y), TF(s.line_y),
                K<TF>(z), TF(s.z0), TF(s.sigma_z), TF(s.line_z), s.use_profile ? K<TF>(prof) : nullptr,
                std::vector<int>{r[0], r[1]}, std::vector<int>{r[2], r[3]}, std::vector<int>{r[4], r[5]}, K<TF>(rhoref), s.swvmr != 0, s.use_profile != 0);
    }

    template<class TF>
    void emit(const Dims& d, const Desc& s, void* st, const void* x, const void* y, const void* z, const void* prof, double nrm, const int* r)
    {
        TF* t = static_cast<TF*>(st);
        if (s.use_profile)
            calc_source<TF, true>(t, K<TF>(x), K<TF>(y), K<TF>(z), K<TF>(prof), TF(s.x0), TF(s.sigma_x), TF(s.line_x), TF(s.y0), TF(s.sigma_y), TF(s.line_y),
                                  TF(s.z0), TF(s.sigma_z), TF(s.line_z), TF(s.strength), TF(nrm), r[0], r[1], r[2], r[3], r[4], r[5], d.icells, d.ijcells);
        else
            calc_source<TF, false>(t, K<TF>(x), K<TF>(y), K<TF>(z), nullptr, TF(s.x0), TF(s.sigma_x), TF(s.line_x), TF(s.y0), TF(s.sigma_y), TF(s.line_y),
                                   TF(s.z0), TF(s.sigma_z), TF(s.line_z), TF(s.strength), TF(nrm), r[0], r[1], r[2], r[3], r[4], r[5], d.icells, d.ijcells);
    }
}

REF_API void ref_source_shape(int dtype, const Dims* d, const Desc* s, const void* x, const void* y, const void* z, const void* prof, int* r)
{
    if (dtype == 0) shape<double>(*d, *s, x, y, z, prof, r); else shape<float>(*d, *s, x, y, z, prof, r);
}
REF_API double ref_source_norm(int dtype, const Dims* d, const Desc* s, const void* x, const void* y, const void* z, const void* dz, double dx, double dy,
                               const void* prof, const int* r, const void* rhoref)
{
    return dtype == 0 ? norm<double>(*d, *s, x, y, z, dz, dx, dy, prof, r, rhoref) : norm<float>(*d, *s, x, y, z, dz, dx, dy, prof, r, rhoref);
}
REF_API void ref_source_emit(int dtype, const Dims* d, const Desc* s, void* st, const void* x, const void* y, const void* z, const void* prof, double nrm, const int* r)
{
    if (dtype == 0) emit<double>(*d, *s, st, x, y, z, prof, nrm, r); else emit<float>(*d, *s, st, x, y, z, prof, nrm, r);
}
// Decay::exec (src/decay.cxx:104-107): decaytime is the map's TF, dt the double of exec narrowed by the call
REF_API void ref_decay(int dtype, const Dims* d, void* tend, const void* var, double timescale, double dt)
{
    if (dtype == 0) enforce_exponential_decay<double>(static_cast<double*>(tend), K<double>(var), timescale, dt, d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
    else            enforce_exponential_decay<float>(static_cast<float*>(tend), K<float>(var), float(timescale), float(dt), d->istart, d->iend, d->jstart, d->jend, d->kstart, d->kend, d->icells, d->ijcells);
}
