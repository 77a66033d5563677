// ref_pres_shim.cpp -- TEST infrastructure: the reference's own Pres_2, Pres_4, Boundary_cyclic and Field3d_operators behind a C interface,
// with the kernels of diff_smag2.cxx that end in a cyclic fill (calc_evisc, calc_evisc_neutral).
//
// Compiled by tests/pres_ref.py into a temporary directory with the reference's src and include directories, tests/stubs_syntax_only
// and this repository's include directory on the include path (g++ -std=c++17 -O2 -ffp-contract=off -DRESTRICTKEYWORD=__restrict__,
// sections collected at link time, together with the reference's master.cxx and master_serial.cxx); nothing compiled from it is kept.
// The translation units are included in place and unmodified. What they leave undefined is a narrow seam, written here from
// scratch: Grid::get_grid_data (a Grid_data filled from mhh_grid), the Pres base class's constructor and destructor, the FFT (two
// function pointers set from Python: none = the transforms do nothing, or the oracle's DFT), and members that only Pres::exec and
// Pres::create reach through the vtable, which abort. Private members are reached through explicit instantiation (which may name
// them), not by editing or redefining anything of the reference's.
#include "boundary_cyclic.cxx"
#include "field3d_operators.cxx"
#include "pres_2.cxx"
#include "pres_4.cxx"
#include "diff_smag2.cxx"

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "mhh_hip.h"

// ---- access to private members ------------------------------------------------------------------------------------------------
namespace seam
{
    template<class Tag> struct Slot { static typename Tag::type ptr; };
    template<class Tag> typename Tag::type Slot<Tag>::ptr;
    template<class Tag, typename Tag::type P> struct Bind { Bind() { Slot<Tag>::ptr = P; } static Bind self; };
    template<class Tag, typename Tag::type P> Bind<Tag, P> Bind<Tag, P>::self;
    template<class Tag> typename Tag::type get() { return Slot<Tag>::ptr; }
}
#define SEAM_BIND(tag, cls, member) \
    template struct seam::Bind<tag<double>, &cls<double>::member>; \
    template struct seam::Bind<tag<float>,  &cls<float>::member>;
#define SEAM_VECTOR(tag, cls, member) \
    template<class TF> struct tag { typedef std::vector<TF> cls<TF>::* type; }; \
    SEAM_BIND(tag, cls, member)

struct Master_md { typedef MPI_data Master::* type; };
template struct seam::Bind<Master_md, &Master::md>;

SEAM_VECTOR(P2_bmati, Pres_2, bmati) SEAM_VECTOR(P2_bmatj, Pres_2, bmatj) SEAM_VECTOR(P2_a, Pres_2, a) SEAM_VECTOR(P2_c, Pres_2, c)
SEAM_VECTOR(P4_bmati, Pres_4, bmati) SEAM_VECTOR(P4_bmatj, Pres_4, bmatj)
SEAM_VECTOR(P4_m1, Pres_4, m1) SEAM_VECTOR(P4_m2, Pres_4, m2) SEAM_VECTOR(P4_m3, Pres_4, m3) SEAM_VECTOR(P4_m4, Pres_4, m4)
SEAM_VECTOR(P4_m5, Pres_4, m5) SEAM_VECTOR(P4_m6, Pres_4, m6) SEAM_VECTOR(P4_m7, Pres_4, m7)

template<class TF> struct P2_input { typedef void (Pres_2<TF>::*type)(TF*, const TF*, const TF*, const TF*, TF*, TF*, TF*, const TF*, const TF*, const TF*, TF); };
template<class TF> struct P2_solve { typedef void (Pres_2<TF>::*type)(TF*, TF*, TF*, const TF*, const TF*); };
template<class TF> struct P2_output { typedef void (Pres_2<TF>::*type)(TF*, TF*, TF*, const TF*, const TF*); };
template<class TF> struct P2_div { typedef TF (Pres_2<TF>::*type)(const TF*, const TF*, const TF*, const TF*, const TF*, const TF*); };
SEAM_BIND(P2_input, Pres_2, input) SEAM_BIND(P2_solve, Pres_2, solve) SEAM_BIND(P2_output, Pres_2, output) SEAM_BIND(P2_div, Pres_2, calc_divergence)

template<class TF> struct P4_input { typedef void (Pres_4<TF>::*type)(TF*, const TF*, const TF*, const TF*, TF*, TF*, TF*, const TF*, TF); };
template<class TF> struct P4_input2d : P4_input<TF> {};
template<class TF> struct P4_solve { typedef void (Pres_4<TF>::*type)(TF*, TF*, const TF*, const TF*, const TF*, const TF*, const TF*, const TF*, const TF*, const TF*,
                                                                      TF*, TF*, TF*, TF*, TF*, TF*, TF*, TF*, TF*, TF*, int); };
template<class TF> struct P4_output { typedef void (Pres_4<TF>::*type)(TF*, TF*, TF*, const TF*, const TF*); };
template<class TF> struct P4_output2d : P4_output<TF> {};
template<class TF> struct P4_div { typedef TF (Pres_4<TF>::*type)(const TF*, const TF*, const TF*, const TF*); };
SEAM_BIND(P4_input, Pres_4, template input<true>) SEAM_BIND(P4_input2d, Pres_4, template input<false>)
SEAM_BIND(P4_output, Pres_4, template output<true>) SEAM_BIND(P4_output2d, Pres_4, template output<false>)
SEAM_BIND(P4_solve, Pres_4, solve) SEAM_BIND(P4_div, Pres_4, calc_divergence)

// ---- the seam: what the included translation units leave undefined ----------------------------------------------------------------
namespace seam
{
    typedef void (*fft_fn)(const mhh_grid*, void*);
    fft_fn fft_forward = nullptr, fft_backward = nullptr;      // none: the transforms do nothing
    const mhh_grid* grid_now = nullptr;

    template<class TF> Grid_data<TF>& grid_data() { static Grid_data<TF> gd; return gd; }

    [[noreturn]] void never(const char* what)
    {
        std::fprintf(stderr, "ref_pres_shim: %s is outside the seam\n", what);
        std::abort();
    }

    template<class TF>
    void fill_grid_data(const mhh_grid* g)
    {
        Grid_data<TF>& gd = grid_data<TF>();
        gd.itot = g->itot; gd.jtot = g->jtot; gd.ktot = g->ktot; gd.ntot = g->itot*g->jtot*g->ktot;
        gd.imax = g->imax; gd.jmax = g->jmax; gd.kmax = g->kmax; gd.nmax = g->imax*g->jmax*g->kmax;
        gd.iblock = g->itot / g->npy; gd.jblock = g->jtot / g->npx; gd.kblock = g->kmax / g->npx;
        gd.igc = g->igc; gd.jgc = g->jgc; gd.kgc = g->kgc;
        gd.icells = g->icells; gd.jcells = g->jcells; gd.ijcells = g->ijcells; gd.kcells = g->kcells; gd.ncells = (int)g->ncells;
        gd.istart = g->istart; gd.jstart = g->jstart; gd.kstart = g->kstart;
        gd.iend = g->iend; gd.jend = g->jend; gd.kend = g->kend;
        gd.xsize = TF(g->xsize); gd.ysize = TF(g->ysize); gd.zsize = TF(g->zsize);
        gd.dx = TF(g->dx); gd.dy = TF(g->dy); gd.dxi = TF(1.)/gd.dx; gd.dyi = TF(1.)/gd.dy;
        auto put = [&](std::vector<TF>& v, const void* src)
        {
            const TF* s = static_cast<const TF*>(src);
            v.assign(s, s + g->kcells);
        };
        put(gd.z, g->z); put(gd.zh, g->zh); put(gd.dz, g->dz); put(gd.dzh, g->dzh);
        put(gd.dzi, g->dzi); put(gd.dzhi, g->dzhi); put(gd.dzi4, g->dzi4); put(gd.dzhi4, g->dzhi4);
        grid_now = g;
    }

    // Storage for an object of a class whose constructor is outside the seam (Grid, Fields, FFT, Input). The object is NEVER
    // constructed: the reference's classes only keep a reference to it, and what they call on it is defined in this file
    // (Grid::get_grid_data, FFT::init / exec_*, which read no member) or aborts. The only members that are live are Fields::rhoref
    // and Fields::rhorefh, which World constructs in place; everything else must stay unread. The storage is filled with 0xA5, not
    // zeroes, so that a member the reference starts to read shows at once: a pointer or a size read from it is far out of range.
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

    // Master, Grid, Fields (rhoref and rhorefh only), FFT and Input as the constructors of the reference's classes take them
    template<class TF>
    struct World
    {
        Grid<TF>* grid; Fields<TF>* fields; FFT<TF>* fft; Input* settings;
        World(const mhh_grid* g, const void* rhoref, const void* rhorefh)
        {
            if (g->npx != 1 || g->npy != 1) never("a decomposed grid");
            fill_grid_data<TF>(g);
            grid = blank<Grid<TF>>(); fields = blank<Fields<TF>>(); fft = blank<FFT<TF>>(); settings = blank<Input>();
            new (&fields->rhoref) std::vector<TF>(); new (&fields->rhorefh) std::vector<TF>();
            if (rhoref)  fields->rhoref.assign(static_cast<const TF*>(rhoref), static_cast<const TF*>(rhoref) + g->kcells);
            if (rhorefh) fields->rhorefh.assign(static_cast<const TF*>(rhorefh), static_cast<const TF*>(rhorefh) + g->kcells);
        }
        ~World()
        {
            typedef std::vector<TF> V;
            fields->rhoref.~V(); fields->rhorefh.~V();
            std::free(grid); std::free(fields); std::free(fft); std::free(settings);
        }
        World(const World&) = delete;
    };
}

template<typename TF> const Grid_data<TF>& Grid<TF>::get_grid_data() { return seam::grid_data<TF>(); }
template const Grid_data<double>& Grid<double>::get_grid_data();
template const Grid_data<float>&  Grid<float>::get_grid_data();

template<typename TF> void FFT<TF>::init() {}
template<typename TF> void FFT<TF>::exec_forward(TF* const restrict data, TF* const restrict)
{
    if (seam::fft_forward) seam::fft_forward(seam::grid_now, data);
}
// the reference's backward transform leaves its result in the second array (src/fft.cxx, "swap array here")
template<typename TF> void FFT<TF>::exec_backward(TF* const restrict data, TF* const restrict tmp1)
{
    if (seam::fft_backward) seam::fft_backward(seam::grid_now, data);
    const Grid_data<TF>& gd = seam::grid_data<TF>();
    std::memcpy(tmp1, data, sizeof(TF)*(size_t)gd.itot*gd.jtot*gd.ktot);
}
template void FFT<double>::init(); template void FFT<double>::exec_forward(double*, double*); template void FFT<double>::exec_backward(double*, double*);
template void FFT<float>::init();  template void FFT<float>::exec_forward(float*, float*);   template void FFT<float>::exec_backward(float*, float*);

template<typename TF> Pres<TF>::Pres(Master& masterin, Grid<TF>& gridin, Fields<TF>& fieldsin, FFT<TF>& fftin, Input&) :
    master(masterin), grid(gridin), fields(fieldsin), fft(fftin), field3d_operators(masterin, gridin, fieldsin) {}
template<typename TF> Pres<TF>::~Pres() {}
template class Pres<double>;
template class Pres<float>;

// reached only from Pres::exec and Pres::create, which nothing here calls
template<typename TF> std::shared_ptr<Field3d<TF>> Fields<TF>::get_tmp() { seam::never("Fields::get_tmp"); }
template<typename TF> void Fields<TF>::release_tmp(std::shared_ptr<Field3d<TF>>&) { seam::never("Fields::release_tmp"); }
template std::shared_ptr<Field3d<double>> Fields<double>::get_tmp(); template void Fields<double>::release_tmp(std::shared_ptr<Field3d<double>>&);
template std::shared_ptr<Field3d<float>>  Fields<float>::get_tmp();  template void Fields<float>::release_tmp(std::shared_ptr<Field3d<float>>&);
template<typename TF> void Stats<TF>::add_tendency(const Field3d<TF>&, const std::string&, const std::string&, const std::string&, const std::string&)
{ seam::never("Stats::add_tendency"); }
template<typename TF> void Stats<TF>::calc_tend(Field3d<TF>&, const std::string&) { seam::never("Stats::calc_tend"); }
template void Stats<double>::add_tendency(const Field3d<double>&, const std::string&, const std::string&, const std::string&, const std::string&);
template void Stats<float>::add_tendency(const Field3d<float>&, const std::string&, const std::string&, const std::string&, const std::string&);
template void Stats<double>::calc_tend(Field3d<double>&, const std::string&);
template void Stats<float>::calc_tend(Field3d<float>&, const std::string&);

// ---- the operators ------------------------------------------------------------------------------------------------------------------
namespace
{
    template<class TF> TF* M(void* p) { return static_cast<TF*>(p); }
    template<class TF> const TF* K(const void* p) { return static_cast<const TF*>(p); }

    template<class TF> bool dim3_of(int dim3) { return dim3 < 0 ? seam::grid_data<TF>().jtot != 1 : dim3 != 0; }   // < 0: as Pres_4::exec chooses

    template<class TF>
    struct Pres2 : seam::World<TF>
    {
        Pres_2<TF> pres;
        Pres2(const mhh_grid* g, const void* r, const void* rh) : seam::World<TF>(g, r, rh), pres(seam::master(), *this->grid, *this->fields, *this->fft, *this->settings)
        { pres.init(); pres.set_values(); }
        const Grid_data<TF>& gd() { return seam::grid_data<TF>(); }
        // the call sites of Pres_2::exec (src/pres_2.cxx:66-94)
        void input(void* p, const void* u, const void* v, const void* w, void* ut, void* vt, void* wt, double dt)
        {
            (pres.*seam::get<P2_input<TF>>())(M<TF>(p), K<TF>(u), K<TF>(v), K<TF>(w), M<TF>(ut), M<TF>(vt), M<TF>(wt),
                                              gd().dzi.data(), this->fields->rhoref.data(), this->fields->rhorefh.data(), dt);
        }
        void solve(void* p)
        {
            std::vector<TF> tmp1(gd().ncells), tmp2(gd().ncells);
            (pres.*seam::get<P2_solve<TF>>())(M<TF>(p), tmp1.data(), tmp2.data(), gd().dz.data(), this->fields->rhoref.data());
        }
        void output(void* ut, void* vt, void* wt, const void* p)
        {
            (pres.*seam::get<P2_output<TF>>())(M<TF>(ut), M<TF>(vt), M<TF>(wt), K<TF>(p), gd().dzhi.data());
        }
        double divergence(const void* u, const void* v, const void* w)
        {
            return (pres.*seam::get<P2_div<TF>>())(K<TF>(u), K<TF>(v), K<TF>(w), gd().dzi.data(), this->fields->rhoref.data(), this->fields->rhorefh.data());
        }
        void coeffs(void* bmati, void* bmatj, void* bands)
        {
            const int kmax = gd().kmax;
            std::copy((pres.*seam::get<P2_bmati<TF>>()).begin(), (pres.*seam::get<P2_bmati<TF>>()).end(), M<TF>(bmati));
            std::copy((pres.*seam::get<P2_bmatj<TF>>()).begin(), (pres.*seam::get<P2_bmatj<TF>>()).end(), M<TF>(bmatj));
            std::copy((pres.*seam::get<P2_a<TF>>()).begin(), (pres.*seam::get<P2_a<TF>>()).end(), M<TF>(bands));
            std::copy((pres.*seam::get<P2_c<TF>>()).begin(), (pres.*seam::get<P2_c<TF>>()).end(), M<TF>(bands) + kmax);
        }
    };

    template<class TF>
    struct Pres4 : seam::World<TF>
    {
        Pres_4<TF> pres;
        Pres4(const mhh_grid* g) : seam::World<TF>(g, nullptr, nullptr), pres(seam::master(), *this->grid, *this->fields, *this->fft, *this->settings)
        { pres.init(); pres.set_values(); }
        const Grid_data<TF>& gd() { return seam::grid_data<TF>(); }
        template<class Tag> std::vector<TF>& vec() { return pres.*seam::get<Tag>(); }
        // the call sites of Pres_4::exec (src/pres_4.cxx:77-144)
        void input(int dim3, void* p, const void* u, const void* v, const void* w, void* ut, void* vt, void* wt, double dt)
        {
            if (dim3_of<TF>(dim3))
                (pres.*seam::get<P4_input<TF>>())(M<TF>(p), K<TF>(u), K<TF>(v), K<TF>(w), M<TF>(ut), M<TF>(vt), M<TF>(wt), gd().dzi4.data(), dt);
            else
                (pres.*seam::get<P4_input2d<TF>>())(M<TF>(p), K<TF>(u), K<TF>(v), K<TF>(w), M<TF>(ut), M<TF>(vt), M<TF>(wt), gd().dzi4.data(), dt);
        }
        void solve(void* p)
        {
            const int jslice = 1;
            const int ns = gd().iblock*jslice*(gd().kmax+4);
            std::vector<TF> tmp1(gd().ncells), tmp2(std::max(4*ns, gd().ncells)), tmp3(std::max(4*ns, gd().ncells));
            (pres.*seam::get<P4_solve<TF>>())(M<TF>(p), tmp1.data(), gd().dz.data(),
                    vec<P4_m1<TF>>().data(), vec<P4_m2<TF>>().data(), vec<P4_m3<TF>>().data(), vec<P4_m4<TF>>().data(),
                    vec<P4_m5<TF>>().data(), vec<P4_m6<TF>>().data(), vec<P4_m7<TF>>().data(),
                    &tmp2[0*ns], &tmp2[1*ns], &tmp2[2*ns], &tmp2[3*ns],
                    &tmp3[0*ns], &tmp3[1*ns], &tmp3[2*ns], &tmp3[3*ns],
                    vec<P4_bmati<TF>>().data(), vec<P4_bmatj<TF>>().data(),
                    jslice);
        }
        void output(int dim3, void* ut, void* vt, void* wt, const void* p)
        {
            if (dim3_of<TF>(dim3))
                (pres.*seam::get<P4_output<TF>>())(M<TF>(ut), M<TF>(vt), M<TF>(wt), K<TF>(p), gd().dzhi4.data());
            else
                (pres.*seam::get<P4_output2d<TF>>())(M<TF>(ut), M<TF>(vt), M<TF>(wt), K<TF>(p), gd().dzhi4.data());
        }
        double divergence(const void* u, const void* v, const void* w)
        {
            return (pres.*seam::get<P4_div<TF>>())(K<TF>(u), K<TF>(v), K<TF>(w), gd().dzi4.data());
        }
        void coeffs(void* bmati, void* bmatj, void* bands)
        {
            const int kmax = gd().kmax;
            std::copy(vec<P4_bmati<TF>>().begin(), vec<P4_bmati<TF>>().end(), M<TF>(bmati));
            std::copy(vec<P4_bmatj<TF>>().begin(), vec<P4_bmatj<TF>>().end(), M<TF>(bmatj));
            std::vector<TF>* m[7] = {&vec<P4_m1<TF>>(), &vec<P4_m2<TF>>(), &vec<P4_m3<TF>>(), &vec<P4_m4<TF>>(), &vec<P4_m5<TF>>(), &vec<P4_m6<TF>>(), &vec<P4_m7<TF>>()};
            for (int n=0; n<7; ++n)
                std::copy(m[n]->begin(), m[n]->end(), M<TF>(bands) + n*kmax);
        }
    };

    template<class TF>
    struct Cyclic : seam::World<TF>
    {
        Boundary_cyclic<TF> bc;
        Field3d_operators<TF> ops;
        Cyclic(const mhh_grid* g) : seam::World<TF>(g, nullptr, nullptr), bc(seam::master(), *this->grid), ops(seam::master(), *this->grid, *this->fields) { bc.init(); }
    };

    Edge edge_of(int edge) { return edge == MHH_EDGE_EW ? Edge::East_west_edge : edge == MHH_EDGE_NS ? Edge::North_south_edge : Edge::Both_edges; }
}

#define REF_API extern "C" __attribute__((visibility("default")))
#define BY_TYPE(g, ...) do { if ((g)->dtype == MHH_F64) { typedef double TF; __VA_ARGS__; } else { typedef float TF; __VA_ARGS__; } } while (0)
#define BY_ORDER(g, order, r, rh, call) \
    do { if ((order) == 2) BY_TYPE(g, Pres2<TF> P(g, r, rh); call); else BY_TYPE(g, Pres4<TF> P(g); call); } while (0)

// fwd, bwd: void (*)(const mhh_grid*, void* packed), both null for transforms that do nothing
REF_API void ref_pres_set_fft(void* fwd, void* bwd)
{
    seam::fft_forward = reinterpret_cast<seam::fft_fn>(fwd); seam::fft_backward = reinterpret_cast<seam::fft_fn>(bwd);
}
// bands: a, c (order 2) or m1..m7 (order 4), kmax values each, in the grid's type like bmati[itot] and bmatj[jtot]
REF_API void ref_pres_set_values(const mhh_grid* g, int order, const void* rhorefh, void* bmati, void* bmatj, void* bands)
{
    if (order == 2) BY_TYPE(g, Pres2<TF> P(g, rhorefh, rhorefh); P.coeffs(bmati, bmatj, bands));
    else            BY_TYPE(g, Pres4<TF> P(g); P.coeffs(bmati, bmatj, bands));
}
// p: a whole field of ncells, the packed values at its start, as the reference's exec passes it. dim3 (order 4): 1, 0, or -1 for exec's choice
REF_API void ref_pres_input(const mhh_grid* g, int order, int dim3, void* p, const void* u, const void* v, const void* w, void* ut, void* vt, void* wt,
                            const void* r, const void* rh, double dt)
{
    if (order == 2) BY_TYPE(g, Pres2<TF> P(g, r, rh); P.input(p, u, v, w, ut, vt, wt, dt));
    else            BY_TYPE(g, Pres4<TF> P(g); P.input(dim3, p, u, v, w, ut, vt, wt, dt));
}
REF_API void ref_pres_solve(const mhh_grid* g, int order, void* p, const void* r, const void* rh)
{
    BY_ORDER(g, order, r, rh, P.solve(p));
}
REF_API void ref_pres_output(const mhh_grid* g, int order, int dim3, void* ut, void* vt, void* wt, const void* p, const void* r, const void* rh)
{
    if (order == 2) BY_TYPE(g, Pres2<TF> P(g, r, rh); P.output(ut, vt, wt, p));
    else            BY_TYPE(g, Pres4<TF> P(g); P.output(dim3, ut, vt, wt, p));
}
REF_API void ref_pres_exec(const mhh_grid* g, int order, void* p, const void* u, const void* v, const void* w, void* ut, void* vt, void* wt,
                           const void* r, const void* rh, double dt)
{
    if (order == 2) BY_TYPE(g, Pres2<TF> P(g, r, rh); P.input(p, u, v, w, ut, vt, wt, dt); P.solve(p); P.output(ut, vt, wt, p));
    else            BY_TYPE(g, Pres4<TF> P(g); P.input(-1, p, u, v, w, ut, vt, wt, dt); P.solve(p); P.output(-1, ut, vt, wt, p));
}
REF_API double ref_pres_divergence(const mhh_grid* g, int order, const void* u, const void* v, const void* w, const void* r, const void* rh)
{
    double d = 0.;
    BY_ORDER(g, order, r, rh, d = P.divergence(u, v, w));
    return d;
}

REF_API void ref_boundary_cyclic(const mhh_grid* g, void* a, int edge) { BY_TYPE(g, Cyclic<TF> C(g); C.bc.exec(M<TF>(a), edge_of(edge))); }
REF_API void ref_boundary_cyclic_2d(const mhh_grid* g, void* a) { BY_TYPE(g, Cyclic<TF> C(g); C.bc.exec_2d(M<TF>(a))); }
REF_API void ref_boundary_cyclic_uint(const mhh_grid* g, unsigned int* a, int edge) { BY_TYPE(g, Cyclic<TF> C(g); C.bc.exec(a, edge_of(edge))); }
REF_API void ref_boundary_cyclic_2d_uint(const mhh_grid* g, unsigned int* a) { BY_TYPE(g, Cyclic<TF> C(g); C.bc.exec_2d(a)); }

// Field3d_operators::calc_mean: the volume-weighted mean at full levels, sum(fld*dz) / (itot*jtot*zsize), as a double
REF_API double ref_calc_mean(const mhh_grid* g, const void* fld)
{
    double mean = 0.;
    BY_TYPE(g, Cyclic<TF> C(g); mean = C.ops.calc_mean(K<TF>(fld)));
    return mean;
}
REF_API void ref_mean_profile(const mhh_grid* g, void* prof, const void* fld) { BY_TYPE(g, Cyclic<TF> C(g); C.ops.calc_mean_profile(M<TF>(prof), K<TF>(fld))); }
REF_API void ref_mean_profile_nogc(const mhh_grid* g, void* prof, const void* fld, int is_hlf)
{ BY_TYPE(g, Cyclic<TF> C(g); C.ops.calc_mean_profile_nogc(M<TF>(prof), K<TF>(fld), is_hlf != 0)); }
REF_API void ref_subtract_mean_profile(const mhh_grid* g, void* fld, const void* prof) { BY_TYPE(g, Cyclic<TF> C(g); C.ops.subtract_mean_profile(M<TF>(fld), K<TF>(prof))); }

// ---- diff_smag2.cxx: the kernels that end in Boundary_cyclic::exec; evisc holds strain2 on entry ------------------------------------------
// the call sites of Diff_smag2::exec_viscosity (src/diff_smag2.cxx:1100-1182): gd.dx, gd.dy, gd.zsize as Grid_data keeps them
REF_API void ref_smag2_evisc(const mhh_grid* g, int sm, void* evisc, const void* u, const void* v, const void* w, const void* N2, const void* bgradbot,
                             const void* z0m, double cs, double tPr)
{
    BY_TYPE(g, Cyclic<TF> C(g); const Grid_data<TF>& gd = seam::grid_data<TF>();
        if (sm) calc_evisc<TF, Surface_model::Enabled>(M<TF>(evisc), K<TF>(u), K<TF>(v), K<TF>(w), K<TF>(N2), K<TF>(bgradbot), gd.z.data(), gd.dz.data(),
                    gd.dzi.data(), K<TF>(z0m), gd.dx, gd.dy, TF(cs), TF(tPr), gd.istart, gd.iend, gd.jstart, gd.jend, gd.kstart, gd.kend,
                    gd.icells, gd.jcells, gd.ijcells, C.bc);
        else    calc_evisc<TF, Surface_model::Disabled>(M<TF>(evisc), K<TF>(u), K<TF>(v), K<TF>(w), K<TF>(N2), nullptr, gd.z.data(), gd.dz.data(),
                    gd.dzi.data(), nullptr, gd.dx, gd.dy, TF(cs), TF(tPr), gd.istart, gd.iend, gd.jstart, gd.jend, gd.kstart, gd.kend,
                    gd.icells, gd.jcells, gd.ijcells, C.bc));
}
REF_API void ref_smag2_evisc_neutral(const mhh_grid* g, int sm, void* evisc, const void* u, const void* v, const void* w, const void* ufluxbot,
                                     const void* vfluxbot, const void* z0m, double cs, double visc)
{
    BY_TYPE(g, Cyclic<TF> C(g); const Grid_data<TF>& gd = seam::grid_data<TF>();
        if (sm) calc_evisc_neutral<TF, Surface_model::Enabled>(M<TF>(evisc), K<TF>(u), K<TF>(v), K<TF>(w), K<TF>(ufluxbot), K<TF>(vfluxbot), gd.z.data(),
                    gd.dz.data(), gd.dzhi.data(), K<TF>(z0m), gd.dx, gd.dy, gd.zsize, TF(cs), TF(visc), gd.istart, gd.iend, gd.jstart, gd.jend,
                    gd.kstart, gd.kend, gd.icells, gd.jcells, gd.ijcells, C.bc);
        else    calc_evisc_neutral<TF, Surface_model::Disabled>(M<TF>(evisc), K<TF>(u), K<TF>(v), K<TF>(w), K<TF>(ufluxbot), K<TF>(vfluxbot), gd.z.data(),
                    gd.dz.data(), gd.dzhi.data(), nullptr, gd.dx, gd.dy, gd.zsize, TF(cs), TF(visc), gd.istart, gd.iend, gd.jstart, gd.jend,
                    gd.kstart, gd.kend, gd.icells, gd.jcells, gd.ijcells, C.bc));
}
