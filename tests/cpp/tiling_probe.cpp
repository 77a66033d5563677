// tests/cpp/tiling_probe.cpp -- host program, no GPU: the launch geometry of the library, from the library's own headers.
// Built with a host compiler against the emulation's HIP stand-in (-I tests/emul -I microhh_amd/csrc, with tests/emul/emul_globals.cpp),
// so make_tiling / decode_tile (k_common.h), make_march_tiling / decode_march / march_tile_rows (k_march_common.h), level_tiling /
// level_tile (level_reduce.h) and div_known (cell_ops.h) below are the functions the kernels run; nothing is restated.
//   tiling_probe cover            every tile of every swept tiling is decoded exactly once, the rows handed out are the rows asked for
//   tiling_probe describe [TUNE]  per stdin line "imax jmax kmax NJ kc tw [j0 j1 j2 j3]" one line of JSON: the three tilings of that
//                                 launch (kc goes through march_kc with the tuning variable TUNE, default MHH_MARCH_KC_RT)
//   tiling_probe divknown         div_known against the IEEE quotient for the divisors the tests hand to the library
#include "k_common.h"
#include "k_march_common.h"
#include "level_reduce.h"
#include <cstdarg>
#include <cstdint>
#include <thread>
#include <vector>

namespace mhh
{
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
}
using namespace mhh;

static mhh_grid grid_of(int imax, int jmax, int kmax, int jgc = 3)
{
    mhh_grid g; memset(&g, 0, sizeof g);
    g.itot = g.imax = imax; g.jtot = g.jmax = jmax; g.ktot = g.kmax = kmax;
    g.igc = 3; g.jgc = jgc; g.kgc = 1;
    g.icells = imax + 6; g.jcells = jmax + 2*jgc; g.kcells = kmax + 2; g.ijcells = g.icells*g.jcells;
    g.istart = 3; g.jstart = jgc; g.kstart = 1; g.iend = 3 + imax; g.jend = jgc + jmax; g.kend = 1 + kmax;
    g.dtype = MHH_F64; g.npx = g.npy = 1;
    return g;
}

// ---- cover ------------------------------------------------------------------------------------------------------------------------
static int fail_cell(const char* who, const Tiling& t, const char* what, unsigned L, int bx, int by, int kz)
{
    printf("%s: %s at L = %u -> (bx %d, by %d, kz %d) in Tiling{nbx %d, nby %d, nk %d, sr %d, ns %d, nseg %d, kseg %d}\n", who, what, L, bx, by, kz,
           t.nbx, t.nby, t.nk, t.sr, t.ns, t.nseg, t.kseg);
    return 1;
}
static int cover_cell(long long& ntilings)
{
    std::vector<unsigned char> seen;
    for (int nbx=1; nbx<=3; ++nbx) for (int nby=1; nby<=140; ++nby) for (int nk=1; nk<=20; ++nk)
    {
        const int ni = BX*(nbx-1) + 1 + (nby % BX), nj = BY*(nby-1) + 1 + (nk % BY);       // ragged last tiles in both directions
        const Tiling t = make_tiling(ni > BX*nbx ? BX*nbx : ni, nj, nk);
        if (t.nbx != nbx || t.nby != nby || t.nk != nk) return fail_cell("make_tiling", t, "extents", 0, nbx, nby, nk);
        seen.assign((size_t)nbx*nby*nk, 0);
        const unsigned nb = tiling_blocks(t);
        for (unsigned L=0; L<nb; ++L)
        {
            int bx = -1, by = -1, kz = -1;
            if (!decode_tile(t, L, bx, by, kz)) continue;
            if (bx < 0 || bx >= nbx || by < 0 || by >= nby || kz < 0 || kz >= nk) return fail_cell("decode_tile", t, "a tile outside the launch", L, bx, by, kz);
            if (seen[((size_t)kz*nby + by)*nbx + bx]++) return fail_cell("decode_tile", t, "a tile decoded twice", L, bx, by, kz);
        }
        for (int kz=0; kz<nk; ++kz) for (int by=0; by<nby; ++by) for (int bx=0; bx<nbx; ++bx)
            if (!seen[((size_t)kz*nby + by)*nbx + bx]) return fail_cell("decode_tile", t, "a tile never decoded", nb, bx, by, kz);
        ++ntilings;
    }
    return 0;
}

static int fail_march(const MarchTiling& t, int NJ, const char* what, unsigned L, int bx, int by, int kc)
{
    printf("decode_march: %s at L = %u -> (bx %d, by %d, kc %d), NJ %d, in MarchTiling{nbx %d, nby %d, nkc %d, sr %d, ns %d, kc %d, rows [%d, %d) + [%d, %d), nby1 %d}\n",
           what, L, bx, by, kc, NJ, t.nbx, t.nby, t.nkc, t.sr, t.ns, t.kc, t.jbase, t.jlim, t.jbase2, t.jlim2, t.nby1);
    return 1;
}
// one marching launch: every (bx, by, kc) once; the rows of the tiles are exactly rows.[j0, j1) + [j2, j3), each once per (bx, kc)
static int cover_march_one(const mhh_grid& g, int NJ, int kc, int tw, const MarchRows& rows, long long& ntilings)
{
    static std::vector<unsigned char> seen, rowhit;
    const MarchTiling t = make_march_tiling(&g, NJ, kc, tw, rows);
    const int j0 = rows.whole() ? g.jstart : rows.j0, j1 = rows.whole() ? g.jend : rows.j1;
    const int nrows = (j1 - j0) + (rows.second() ? rows.j3 - rows.j2 : 0);
    if (t.nbx != (g.imax + tw-1)/tw || t.nkc != (g.kmax + kc-1)/kc || t.nby < 1 || t.sr < 1 || t.ns*t.sr < t.nby)
        return fail_march(t, NJ, "extents", 0, t.nbx, t.nby, t.nkc);
    seen.assign((size_t)t.nbx*t.nby*t.nkc, 0);
    rowhit.assign((size_t)g.jcells, 0);
    const unsigned nb = march_blocks(t);
    for (unsigned L=0; L<nb; ++L)
    {
        int bx = -1, by = -1, c = -1;
        if (!decode_march(t, L, bx, by, c)) continue;
        if (bx < 0 || bx >= t.nbx || by < 0 || by >= t.nby || c < 0 || c >= t.nkc) return fail_march(t, NJ, "a tile outside the launch", L, bx, by, c);
        if (seen[((size_t)c*t.nby + by)*t.nbx + bx]++) return fail_march(t, NJ, "a tile decoded twice", L, bx, by, c);
        if (bx == 0 && c == 0)
        {
            int ja, jl; march_tile_rows(t, by, NJ, ja, jl);
            if (ja < 0 || ja >= jl) return fail_march(t, NJ, "a tile without rows", L, bx, by, c);
            for (int j=ja; j<ja+NJ && j<jl; ++j)          // the rows a tile works: j = j0 + ty < jlim (the kernels' guard)
            {
                if (j >= g.jcells || rowhit[j]++) return fail_march(t, NJ, "a row handed out twice or outside the array", L, bx, by, c);
                const bool asked = (j >= j0 && j < j1) || (rows.second() && j >= rows.j2 && j < rows.j3);
                if (!asked) return fail_march(t, NJ, "a row outside the ranges", L, bx, by, c);
            }
        }
    }
    for (int c=0; c<t.nkc; ++c) for (int by=0; by<t.nby; ++by) for (int bx=0; bx<t.nbx; ++bx)
        if (!seen[((size_t)c*t.nby + by)*t.nbx + bx]) return fail_march(t, NJ, "a tile never decoded", nb, bx, by, c);
    int hit = 0;
    for (int j=0; j<g.jcells; ++j) hit += rowhit[j];
    if (hit != nrows) return fail_march(t, NJ, "rows missing", nb, hit, nrows, 0);
    ++ntilings;
    return 0;
}
static int cover_march(long long& ntilings)
{
    const int NJ = 4, tw = 64;
    for (int nbx=1; nbx<=3; ++nbx) for (int nby=1; nby<=140; ++nby) for (int nkc=1; nkc<=20; ++nkc)
    {
        const int kc = 8;
        const mhh_grid g = grid_of(tw*(nbx-1) + 1 + (nby % tw), NJ*(nby-1) + 1 + (nkc % NJ), kc*(nkc-1) + 1 + (nby % kc));
        if (cover_march_one(g, NJ, kc, tw, MarchRows{}, ntilings)) return 1;
    }
    // the other tile shapes: two cells per lane (tw = 128), NJ = 2 and 8 (sr = 8, 2)
    for (int NJ2 : {2, 4, 8}) for (int nby=1; nby<=140; ++nby) for (int nkc=1; nkc<=20; nkc+=3)
    {
        const mhh_grid g = grid_of(256 + 2*(nby % 3), NJ2*nby - (nby % NJ2), 16*nkc - (nkc % 5));
        if (cover_march_one(g, NJ2, 16, 128, MarchRows{}, ntilings)) return 1;
    }
    // a second range: nby1 tile rows from jstart (the last one ragged or not), a gap, rows2 rows up to jend
    for (int nbx=1; nbx<=2; ++nbx) for (int nby1=1; nby1<=40; ++nby1) for (int cut1=0; cut1<NJ; cut1+=3) for (int rows2=1; rows2<=101; rows2+=(rows2 < 20 ? 1 : 9))
        for (int nkc=1; nkc<=20; nkc+=(nkc < 4 ? 1 : 5))
        {
            const int rows1 = NJ*nby1 - cut1, gap = 1 + (rows2 % 7);
            if (rows1 < 1) continue;
            const mhh_grid g = grid_of(tw*nbx - 5, rows1 + gap + rows2, 8*nkc - 3);
            MarchRows r; r.j0 = g.jstart; r.j1 = g.jstart + rows1; r.j2 = g.jend - rows2; r.j3 = g.jend;
            if (cover_march_one(g, NJ, 8, tw, r, ntilings)) return 1;
            MarchRows one; one.j0 = r.j2; one.j1 = r.j3;                                  // a single range that is not the whole interior
            if (cover_march_one(g, NJ, 8, tw, one, ntilings)) return 1;
        }
    return 0;
}

static int cover_level(long long& ntilings)
{
    std::vector<unsigned char> seen, rowhit;
    for (int chunks=1; chunks<=140; ++chunks) for (int cut=0; cut<2; ++cut) for (int nk=1; nk<=20; ++nk)
    {
        const mhh_grid g = grid_of(70, cut ? LEVEL_ROWS*(chunks-1) + 1 + (nk % (LEVEL_ROWS-1)) : LEVEL_ROWS*chunks, nk, 2);
        if (level_chunks(&g) != chunks) { printf("level_chunks: %d rows give %d chunks, not %d\n", g.jmax, level_chunks(&g), chunks); return 1; }
        const Tiling t = level_tiling(&g, nk);
        const LevelDomain D = level_domain(&g);
        seen.assign((size_t)chunks*nk, 0); rowhit.assign((size_t)g.jcells*nk, 0);
        if (t.nbx != 1 || t.nby != chunks || t.nk != nk) return fail_cell("level_tiling", t, "extents", 0, 1, chunks, nk);
        const unsigned nb = tiling_blocks(t);
        for (unsigned L=0; L<nb; ++L)
        {
            LevelTile T;
            if (!level_tile(t, L, 5, D, T)) continue;
            if (T.by < 0 || T.by >= chunks || T.kz < 0 || T.kz >= nk || T.k != 5 + T.kz) return fail_cell("level_tile", t, "a chunk outside the launch", L, 0, T.by, T.kz);
            if (seen[(size_t)T.kz*chunks + T.by]++) return fail_cell("level_tile", t, "a chunk decoded twice", L, 0, T.by, T.kz);
            if (T.j0 != g.jstart + T.by*LEVEL_ROWS || T.j1 <= T.j0 || T.j1 > g.jend || T.j1 - T.j0 > LEVEL_ROWS)
                return fail_cell("level_tile", t, "the rows of a chunk", L, T.j0, T.j1, T.kz);
            for (int j=T.j0; j<T.j1; ++j) if (rowhit[(size_t)T.kz*g.jcells + j]++) return fail_cell("level_tile", t, "a row handed out twice", L, j, T.by, T.kz);
        }
        for (int kz=0; kz<nk; ++kz)
        {
            for (int by=0; by<chunks; ++by) if (!seen[(size_t)kz*chunks + by]) return fail_cell("level_tile", t, "a chunk never decoded", nb, 0, by, kz);
            for (int j=0; j<g.jcells; ++j)
                if (rowhit[(size_t)kz*g.jcells + j] != (j >= g.jstart && j < g.jend ? 1 : 0)) return fail_cell("level_tile", t, "the rows of a level", nb, j, 0, kz);
        }
        ++ntilings;
    }
    return 0;
}

// ---- describe ---------------------------------------------------------------------------------------------------------------------
static void print_tiling(const char* name, const Tiling& t)
{
    printf("\"%s\": {\"nbx\": %d, \"nby\": %d, \"nk\": %d, \"sr\": %d, \"ns\": %d, \"nseg\": %d, \"kseg\": %d, \"blocks\": %u}", name, t.nbx, t.nby, t.nk, t.sr, t.ns,
           t.nseg, t.kseg, tiling_blocks(t));
}
static int describe(const char* tune)
{
    char line[256];
    while (fgets(line, sizeof line, stdin))
    {
        int imax, jmax, kmax, NJ, kc, tw, r[4] = {-1, -1, -1, -1};
        const int n = sscanf(line, "%d %d %d %d %d %d %d %d %d %d", &imax, &jmax, &kmax, &NJ, &kc, &tw, &r[0], &r[1], &r[2], &r[3]);
        if (n < 6) continue;
        const mhh_grid g = grid_of(imax, jmax, kmax);
        MarchRows rows;
        if (n >= 8) { rows.j0 = r[0]; rows.j1 = r[1]; }
        if (n >= 10) { rows.j2 = r[2]; rows.j3 = r[3]; }
        const MarchTiling m = make_march_tiling(&g, NJ, march_kc(&g, rows, kc, tune), tw, rows);
        // strips of a rows2 launch that hold tile rows of both ranges, found through the decoder
        std::vector<int> kinds((size_t)m.ns, 0);
        for (unsigned L=0; L<march_blocks(m); ++L)
        {
            int bx, by, c;
            if (!decode_march(m, L, bx, by, c)) continue;
            int ja, jl; march_tile_rows(m, by, NJ, ja, jl);
            kinds[by / m.sr] |= (rows.second() && ja >= m.jbase2 && by >= m.nby1) ? 2 : 1;
        }
        int straddle = 0;
        for (int k : kinds) straddle += (k == 3);
        printf("{");
        print_tiling("cell", make_tiling(imax, jmax, kmax));
        printf(", \"march\": {\"nbx\": %d, \"nby\": %d, \"nkc\": %d, \"sr\": %d, \"ns\": %d, \"kc\": %d, \"nby1\": %d, \"blocks\": %u, \"straddle\": %d}, ",
               m.nbx, m.nby, m.nkc, m.sr, m.ns, m.kc, m.nby1, march_blocks(m), straddle);
        print_tiling("level", level_tiling(&g, kmax));
        printf("}\n");
    }
    return 0;
}

// ---- divknown ---------------------------------------------------------------------------------------------------------------------
// The turbulent Prandtl numbers of the tests; the kernels divide by tPr (k_visc.hip) and by 2 tPr (k_march.hip)
static const double TPR[] = {1./3., 0.4, 0.7, 0.85, 1.0};
static const int F32_BOUND = -100, F64_BOUND = -960;        // exactness is claimed (cell_ops.h) for |x| >= 2^BOUND
static const int NONE = -1000;

template<class TF> static bool one(TF x, TF d, TF r, long long& bad, TF& xbad)
{
    const TF got = div_known(x, d, r), want = x / d;
    if (got == want || (got != got && want != want)) return true;
    if (!bad++) xbad = x;
    return false;
}
static float f32_of(uint32_t significand, int e)
{
    uint32_t u = 0x3F800000u | significand; float x; memcpy(&x, &u, 4);
    return std::ldexp(x, e);
}
// fp32, one divisor: every significand of x at exponent 0, both signs (the arithmetic is the same in every binade in which nothing
// underflows); then every 101st significand in every tenth binade from 2^100 down and in every binade from 2^-70 to the bound; then
// on downwards to find the binade in which the residuals start to underflow
struct F32Result { float d; long long bad; float xbad; int first; };
static void f32_job(F32Result* out)
{
    const float d = out->d, r = 1.f/d;
    long long bad = 0; float xbad = 0;
    for (uint32_t m=0; m<(1u<<23); ++m) { const float x = f32_of(m, 0); one(x, d, r, bad, xbad); one(-x, d, r, bad, xbad); }
    for (int e=100; e>=F32_BOUND; e-=(e > -70 ? 10 : 1)) for (uint32_t m=0; m<(1u<<23); m+=101)
    {
        const float x = f32_of(m, e);
        one(x, d, r, bad, xbad); one(-x, d, r, bad, xbad);
    }
    int first = NONE;
    for (int e=F32_BOUND-1; e>=-149 && first == NONE; --e) for (uint32_t m=0; m<(1u<<23); m+=101)
    {
        long long b = 0; float xb;
        if (!one(f32_of(m, e), d, r, b, xb)) { first = e; break; }
    }
    out->bad = bad; out->xbad = xbad; out->first = first;
}
// fp64: n random pairs (significand and sign of x random, exponent in [F64_BOUND, 960]) over the same divisors
struct F64Result { uint64_t seed; long long n, bad; double xbad, dbad; };
static void f64_job(F64Result* out)
{
    uint64_t st = out->seed;
    long long bad = 0;
    for (long long n=0; n<out->n; ++n)
    {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        const uint64_t a = st;
        const double d = ((a >> 60) & 1 ? 2. : 1.) * TPR[(a >> 56) % 5], r = 1./d;
        const uint64_t e = (uint64_t)(1023 + F64_BOUND) + (uint32_t)(a >> 20) % (uint32_t)(960 - F64_BOUND + 1);      // the biased exponent
        const uint64_t sb = a * 0x9E3779B97F4A7C15ull;                                                         // fresh bits for the significand
        uint64_t u = ((sb >> 12) | (e << 52)) | (a & 0x8000000000000000ull); double x; memcpy(&x, &u, 8);
        long long b = 0; double xb;
        if (!one(x, d, r, b, xb)) { if (!bad++) { out->xbad = x; out->dbad = d; } }
    }
    out->bad = bad;
}
static int divknown()
{
    int rc = 0;
    F32Result f32[10]; F64Result f64[4];
    std::vector<std::thread> pool;
    for (int n=0; n<10; ++n)
    {
        f32[n].d = (n & 1) ? 2.f*(float)TPR[n/2] : (float)TPR[n/2];
        if (!known_divisor_ok(f32[n].d)) { printf("divknown: %.9g is refused as a divisor\n", (double)f32[n].d); return 1; }
        pool.emplace_back(f32_job, &f32[n]);
    }
    const long long N = 100000000ll;
    for (int n=0; n<4; ++n) { f64[n] = {0x9E3779B97F4A7C15ull*(uint64_t)(n+1), N/4, 0, 0., 0.}; pool.emplace_back(f64_job, &f64[n]); }
    for (auto& t : pool) t.join();
    int worst32 = NONE;
    for (const F32Result& q : f32)
    {
        if (q.bad) { printf("divknown fp32 d = %.9g: %lld mismatches at |x| >= 2^%d, first x = %a\n", (double)q.d, q.bad, F32_BOUND, (double)q.xbad); rc = 1; continue; }
        if (q.first == NONE) printf("divknown fp32 d = %.9g: exact for |x| >= 2^%d; no mismatch below it either\n", (double)q.d, F32_BOUND);
        else printf("divknown fp32 d = %.9g: exact for |x| >= 2^%d; first mismatch in the binade 2^%d\n", (double)q.d, F32_BOUND, q.first);
        if (q.first > worst32) worst32 = q.first;
    }
    long long bad = 0;
    for (const F64Result& q : f64)
        if (q.bad) { if (!bad) printf("divknown fp64: first mismatch x = %a, d = %.17g\n", q.xbad, q.dbad); bad += q.bad; }
    if (bad) { printf("divknown fp64: %lld mismatches of %lld\n", bad, N); rc = 1; }
    else printf("divknown fp64: %lld random pairs exact for 2^%d <= |x| <= 2^960\n", N, F64_BOUND);
    printf("divknown fp32 bound: highest binade with a mismatch 2^%d\n", worst32);
    return rc;
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "";
    int rc = 2;
    if (!strcmp(mode, "cover"))
    {
        long long nc = 0, nm = 0, nl = 0;
        rc = cover_cell(nc) || cover_march(nm) || cover_level(nl);
        if (!rc) printf("cover: %lld cell, %lld march and %lld level tilings decode every tile once\n", nc, nm, nl);
    }
    else if (!strcmp(mode, "describe")) rc = describe(argc > 2 ? argv[2] : "MHH_MARCH_KC_RT");
    else if (!strcmp(mode, "divknown")) rc = divknown();
    else fprintf(stderr, "usage: tiling_probe cover | describe [TUNE] | divknown\n");
    if (!rc) printf("tiling_probe ok\n");
    return rc;
}
