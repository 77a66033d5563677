// k_slab.hip -- the pieces of the hot path that differ when the grid is slab-decomposed in y over the GPUs of
// a node (npx = 1, npy = N): north-south halo pack/unpack around the neighbour exchange, and
// the pressure solver split at the x<->y transpose. The exchanges themselves (ring send/recv, all-to-all)
// are issued by the host through torch.distributed (RCCL over xGMI); nothing here communicates.
//
// Reference semantics: Boundary_cyclic::exec's MPI path (src/boundary_cyclic.cxx:116-176) and the FFT/solve
// sequence of src/fft.cxx:451-583 with npx = 1, where only Transpose::exec_xy / exec_yx move data
// (src/transpose.cxx:170-219) and Pres_2::solve swaps the mode indices (src/pres_2.cxx:297-299).
#include <utility>
#include "fft_lifetime.h"
#include "pres_lds_slab.h"
#include "pres4_bands.h"

using namespace mhh;

// =======================================================================================================
// North-south halo: buffers are [field][k][jg][i] with all icells (x ghosts included, so corners are right
// once the east-west fill has run first, like the reference's ordering).
// =======================================================================================================
constexpr int MAXF = 8;
template<class TF> struct FieldList { TF* f[MAXF]; };

// rs rows travel south (my southernmost interior rows -> the first rs north ghost rows of the south neighbour), rn rows
// travel north (my northernmost interior rows -> the rn south ghost rows next to the north neighbour's interior).
// The full exchange is rs = rn = jgc; a consumer that reads one row beyond the slab in one direction only (pres input:
// vt[j+1]; pres output: p[j-1]) moves just that row.
template<class TF, bool PACK>
__global__ void __launch_bounds__(256) halo_ns_kernel(FieldList<TF> fl, TF* __restrict__ south, TF* __restrict__ north,
                                                      int icells, int ijcells, int kcells, int jgc, int jstart, int jend, int rs, int rn)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    const int k = blockIdx.y, n = blockIdx.z;
    if (i >= icells) return;
    TF* __restrict__ a = fl.f[n] + (size_t)k*ijcells;
    const size_t bs = ((size_t)n*kcells + k) * rs * icells + i, bn = ((size_t)n*kcells + k) * rn * icells + i;
    if (PACK)
    {
        for (int j=0; j<rs; ++j) south[bs + (size_t)j*icells] = a[i + (jstart + j)*icells];
        for (int j=0; j<rn; ++j) north[bn + (size_t)j*icells] = a[i + (jend - rn + j)*icells];
    }
    else
    {
        // `south` holds what the south neighbour sent north (its rn rows), `north` what the north neighbour sent south (rs rows)
        for (int j=0; j<rn; ++j) a[i + (jgc - rn + j)*icells] = south[bn + (size_t)j*icells];
        for (int j=0; j<rs; ++j) a[i + (jend + j)*icells] = north[bs + (size_t)j*icells];
    }
}
template<class TF, bool PACK>
static int halo_launch(const mhh_grid* g, void* const* fields, int nf, void* south, void* north, int rs, int rn, hipStream_t st)
{
    FieldList<TF> fl;
    for (int n=0; n<MAXF; ++n) fl.f[n] = mp<TF>(fields[n < nf ? n : 0]);
    hipLaunchKernelGGL((halo_ns_kernel<TF, PACK>), dim3((g->icells + 255)/256, g->kcells, nf), dim3(256), 0, st, fl, mp<TF>(south), mp<TF>(north),
                       g->icells, g->ijcells, g->kcells, g->jgc, g->jstart, g->jend, rs, rn);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
static int halo_check(const mhh_grid* g, void* const* fields, int nf, const void* a, const void* b)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(nf >= 1 && nf <= MAXF && fields && a && b, "1..8 fields, non-null buffers");
    for (int n=0; n<nf; ++n) MHH_REQUIRE(fields[n] != nullptr, "null field");
    MHH_REQUIRE(g->jmax >= g->jgc, "jmax >= jgc (src/grid.cxx:420)");
    return MHH_OK;
}
MHH_API int mhh_halo_pack_rows(const mhh_grid* g, void* const* fields, int nf, int rows_south, int rows_north, void* send_south, void* send_north, void* stream)
{
    if (int e = halo_check(g, fields, nf, send_south, send_north)) return e;
    MHH_REQUIRE(rows_south >= 0 && rows_south <= g->jgc && rows_north >= 0 && rows_north <= g->jgc && rows_south + rows_north > 0, "0 <= rows <= jgc");
    if (g->dtype == MHH_F64) return halo_launch<double, true>(g, fields, nf, send_south, send_north, rows_south, rows_north, as_stream(stream));
    return halo_launch<float, true>(g, fields, nf, send_south, send_north, rows_south, rows_north, as_stream(stream));
}
MHH_API int mhh_halo_unpack_rows(const mhh_grid* g, void* const* fields, int nf, int rows_south, int rows_north, const void* recv_south, const void* recv_north, void* stream)
{
    if (int e = halo_check(g, fields, nf, recv_south, recv_north)) return e;
    MHH_REQUIRE(rows_south >= 0 && rows_south <= g->jgc && rows_north >= 0 && rows_north <= g->jgc && rows_south + rows_north > 0, "0 <= rows <= jgc");
    if (g->dtype == MHH_F64) return halo_launch<double, false>(g, fields, nf, const_cast<void*>(recv_south), const_cast<void*>(recv_north), rows_south, rows_north, as_stream(stream));
    return halo_launch<float, false>(g, fields, nf, const_cast<void*>(recv_south), const_cast<void*>(recv_north), rows_south, rows_north, as_stream(stream));
}
MHH_API int mhh_halo_pack_ns(const mhh_grid* g, void* const* fields, int nf, void* send_south, void* send_north, void* stream)
{ return mhh_halo_pack_rows(g, fields, nf, g ? g->jgc : 0, g ? g->jgc : 0, send_south, send_north, stream); }
MHH_API int mhh_halo_unpack_ns(const mhh_grid* g, void* const* fields, int nf, const void* recv_south, const void* recv_north, void* stream)
{ return mhh_halo_unpack_rows(g, fields, nf, g ? g->jgc : 0, g ? g->jgc : 0, recv_south, recv_north, stream); }
MHH_API unsigned long long mhh_halo_buffer_elems(const mhh_grid* g, int nf)
{
    return (unsigned long long)nf * g->kcells * g->jgc * g->icells;
}

// =======================================================================================================
// Slab pressure solver (pres_2, pres_4). Layouts, all complex interleaved, nxh = itot/2+1, nxb = ceil(nxh/npy):
//   specx [k][jl][kx]            after the local x transform (jl in this rank's jmax rows)
//   xbuf  [q][k][jl][kxl]        all-to-all buffer, q = destination / source rank, kx = q*nxb + kxl (zero padded)
//   specy [k][kxl][j]            after the exchange, j over the full jtot, unit stride for the y transform
// =======================================================================================================
struct mhh_pres_slab_plan
{
    int order = 2, dtype = 0, itot = 0, jtot = 0, ktot = 0, jmax = 0, npy = 1, rank = 0, nxh = 0, nxb = 0;
    size_t esz = 8;
    void* bmati = nullptr; void* bmatj = nullptr; void* a = nullptr; void* c = nullptr; void* dz = nullptr; void* rhoref = nullptr;
    void* m[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // pres_4: the interior rows of the seven bands
    void* packed = nullptr; void* specx = nullptr; void* specy = nullptr; void* work = nullptr;
    // the transforms over ONE k-slice of ktot / nchunks levels (mhh_pres_slab_set_chunks; one slice = all levels): slice c of the
    // all-to-all can travel while slice c+1 is transformed
    int nchunks = 1;
    rocfft_plan fx = nullptr, bx = nullptr, fy = nullptr, by = nullptr;
    rocfft_execution_info info = nullptr;
    void* wb = nullptr; size_t wbs = 0, wb_cap = 0;
    // the x stages with the transforms in LDS (pres_lds.h, pres_lds_slab.h): twiddles exp(-2 pi i m / itot); null = not available
    void* tx_lds = nullptr; void* ty_lds = nullptr;
};

template<class TF>
static int slab_tables(mhh_pres_slab_plan* P, const mhh_grid* g, const void* hdz, const void* hdzhi, const void* hrho, const void* hrhoh)
{
    // Pres_2::set_values, src/pres_2.cxx:125-153
    const int itot = g->itot, jtot = g->jtot, kmax = g->kmax, kgc = g->kgc;
    const TF dx = TF(g->dx), dy = TF(g->dy);
    const TF dxidxi = 1./(dx*dx), dyidyi = 1./(dy*dy);
    const TF pi = std::acos(-1.);
    std::vector<TF> bi(itot), bj(jtot), a(kmax), c(kmax), dzk(kmax), rk(kmax);
    for (int j=0; j<jtot/2+1; ++j) bj[j] = 2. * (std::cos(2.*pi*(TF)j/(TF)jtot)-1.) * dyidyi;
    for (int j=jtot/2+1; j<jtot; ++j) bj[j] = bj[jtot-j];
    for (int i=0; i<itot/2+1; ++i) bi[i] = 2. * (std::cos(2.*pi*(TF)i/(TF)itot)-1.) * dxidxi;
    for (int i=itot/2+1; i<itot; ++i) bi[i] = bi[itot-i];
    const TF* dz = cp<TF>(hdz); const TF* dzhi = cp<TF>(hdzhi); const TF* rhoh = cp<TF>(hrhoh); const TF* rho = cp<TF>(hrho);
    for (int k=0; k<kmax; ++k)
    {
        a[k] = dz[k+kgc] * rhoh[k+kgc  ]*dzhi[k+kgc  ];
        c[k] = dz[k+kgc] * rhoh[k+kgc+1]*dzhi[k+kgc+1];
        dzk[k] = dz[k+kgc]; rk[k] = rho[k+kgc];
    }
    if (int e = upload(&P->bmati, bi)) return e;
    if (int e = upload(&P->bmatj, bj)) return e;
    if (int e = upload(&P->a, a)) return e;
    if (int e = upload(&P->c, c)) return e;
    if (int e = upload(&P->dz, dzk)) return e;
    return upload(&P->rhoref, rk);
}
// Pres_4::set_values, src/pres_4.cxx:179-252: the single-GPU plan's own host tables (pres4_bands.h)
template<class TF>
static int slab_tables4(mhh_pres_slab_plan* P, const mhh_grid* g, const void* hdzi4, const void* hdzhi4)
{
    std::vector<TF> bi, bj, m[7];
    host_bmat<TF>(4, g, bi, bj);
    host_pres4_bands<TF>(g, cp<TF>(hdzi4), cp<TF>(hdzhi4), m);
    if (int e = upload(&P->bmati, bi)) return e;
    if (int e = upload(&P->bmatj, bj)) return e;
    for (int n=0; n<7; ++n) if (int e = upload(&P->m[n], m[n])) return e;
    return MHH_OK;
}

static int plan1d(rocfft_plan* plan, rocfft_transform_type type, rocfft_result_placement place, int dtype, size_t n, size_t batch,
                  rocfft_array_type in_t, rocfft_array_type out_t, size_t in_dist, size_t out_dist, size_t* wbs)
{
    const size_t len[1] = {n}, one[1] = {1}, off[1] = {0};
    rocfft_plan_description d = nullptr;
    MHH_FFT_TRY(rocfft_plan_description_create(&d));
    MHH_FFT_TRY(rocfft_plan_description_set_data_layout(d, in_t, out_t, off, off, 1, one, in_dist, 1, one, out_dist));
    MHH_FFT_TRY(rocfft_plan_create(plan, place, type, dtype == MHH_F64 ? rocfft_precision_double : rocfft_precision_single, 1, len, batch, d));
    MHH_FFT_TRY(rocfft_plan_description_destroy(d));
    size_t w = 0;
    MHH_FFT_TRY(rocfft_plan_get_work_buffer_size(*plan, &w));
    if (w > *wbs) *wbs = w;
    return MHH_OK;
}

// the four transforms of the solve over one k-slice of ktot / nchunks levels, in place of the ones the plan has (which live until
// the new ones exist: rocFFT shares the tables of equal lengths between live plans; a failure leaves the plan as it was). *wbs grows
// to the largest work area they ask for
static int slab_fft_plans(mhh_pres_slab_plan* P, int nchunks, size_t* wbs)
{
    const int kc = P->ktot / nchunks;
    const rocfft_array_type R = rocfft_array_type_real, H = rocfft_array_type_hermitian_interleaved, Cx = rocfft_array_type_complex_interleaved;
    const size_t bx = (size_t)P->jmax*kc, by = (size_t)P->nxb*kc;
    rocfft_plan n[4] = {nullptr, nullptr, nullptr, nullptr};
    int e = plan1d(&n[0], rocfft_transform_type_real_forward, rocfft_placement_notinplace, P->dtype, P->itot, bx, R, H, P->itot, P->nxh, wbs);
    if (!e) e = plan1d(&n[1], rocfft_transform_type_real_inverse, rocfft_placement_notinplace, P->dtype, P->itot, bx, H, R, P->nxh, P->itot, wbs);
    if (!e) e = plan1d(&n[2], rocfft_transform_type_complex_forward, rocfft_placement_inplace, P->dtype, P->jtot, by, Cx, Cx, P->jtot, P->jtot, wbs);
    if (!e) e = plan1d(&n[3], rocfft_transform_type_complex_inverse, rocfft_placement_inplace, P->dtype, P->jtot, by, Cx, Cx, P->jtot, P->jtot, wbs);
    if (!e) { std::swap(n[0], P->fx); std::swap(n[1], P->bx); std::swap(n[2], P->fy); std::swap(n[3], P->by); P->nchunks = nchunks; }
    for (rocfft_plan p : n) if (p) rocfft_plan_destroy(p);
    return e;
}

MHH_API void mhh_pres_slab_plan_destroy(mhh_pres_slab_plan* P)
{
    if (P && P->tx_lds) { (void)hipFree(P->tx_lds); P->tx_lds = nullptr; }
    if (P && P->ty_lds) { (void)hipFree(P->ty_lds); P->ty_lds = nullptr; }
    if (!P) return;
    for (rocfft_plan p : {P->fx, P->bx, P->fy, P->by}) if (p) rocfft_plan_destroy(p);
    if (P->info) rocfft_execution_info_destroy(P->info);
    for (void* b : {P->bmati, P->bmatj, P->a, P->c, P->dz, P->rhoref, P->packed, P->specx, P->specy, P->work, P->wb}) if (b) (void)hipFree(b);
    for (void* b : P->m) if (b) (void)hipFree(b);
    delete P;
}

static int slab_factor(mhh_pres_slab_plan* P);     // tdma_slab_factor_kernel / hdma_slab_factor_kernel launch, defined with the kernels
MHH_API int mhh_pres_slab_plan_create_order(const mhh_grid* g, int order, const void* host_dz, const void* host_dzhi, const void* host_dzi4, const void* host_dzhi4,
                                            const void* host_rhoref, const void* host_rhorefh, mhh_pres_slab_plan** out)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(out != nullptr, "out");
    MHH_REQUIRE(order == 2 || order == 4, "order must be 2 or 4");
    MHH_REQUIRE(g->npy >= 1 && g->jtot % g->npy == 0 && g->jmax == g->jtot / g->npy && g->imax == g->itot, "slab grid: jmax = jtot/npy, imax = itot");
    MHH_REQUIRE(g->mpicoordy >= 0 && g->mpicoordy < g->npy, "mpicoordy");
    if (order == 2)
    {
        MHH_REQUIRE(host_dz && host_dzhi && host_rhoref && host_rhorefh, "null pointer");
        MHH_REQUIRE(g->jtot > 1 && g->kgc >= 1 && g->igc >= 1 && g->jgc >= 1, "pres_2 slab needs a 3-D grid with 1 ghost cell");
    }
    else
    {
        MHH_REQUIRE(host_dzi4 && host_dzhi4, "null pointer");
        MHH_REQUIRE(g->jtot > 1 && g->kgc >= 2 && g->igc >= 2 && g->jgc >= 2 && g->kmax >= 4, "pres_4 slab needs a 3-D grid with 2 ghost cells and kmax >= 4");
    }
    mhh_pres_slab_plan* P = new mhh_pres_slab_plan();
    P->order = order; P->dtype = g->dtype; P->itot = g->itot; P->jtot = g->jtot; P->ktot = g->ktot; P->jmax = g->jmax; P->npy = g->npy; P->rank = g->mpicoordy;
    P->nxh = g->itot/2 + 1; P->nxb = (P->nxh + g->npy - 1) / g->npy; P->esz = (g->dtype == MHH_F64) ? 8 : 4;
    int e = (order == 4) ? ((g->dtype == MHH_F64) ? slab_tables4<double>(P, g, host_dzi4, host_dzhi4) : slab_tables4<float>(P, g, host_dzi4, host_dzhi4))
                         : ((g->dtype == MHH_F64) ? slab_tables<double>(P, g, host_dz, host_dzhi, host_rhoref, host_rhorefh)
                                                  : slab_tables<float>(P, g, host_dz, host_dzhi, host_rhoref, host_rhorefh));
    const size_t nreal = (size_t)g->itot*g->jmax*g->ktot, nx = (size_t)P->nxh*g->jmax*g->ktot, ny = (size_t)P->nxb*g->jtot*g->ktot;
    // the factors of every column, computed below: pres_2 the pivots w2 and the eliminated upper diagonal w3 (kmax levels each),
    // pres_4 the seven LU bands of the kmax+4 rows
    const size_t nwork = (order == 2) ? 2*ny : (size_t)7*(g->ktot + 4)*P->nxb*g->jtot;
    auto alloc = [&](void** p, size_t bytes) { if (e) return; hipError_t h = hipMalloc(p, bytes); if (h != hipSuccess) { set_error("hipMalloc: %s", hipGetErrorString(h)); e = MHH_ENOMEM; } };
    alloc(&P->packed, nreal*P->esz); alloc(&P->specx, nx*2*P->esz); alloc(&P->specy, ny*2*P->esz); alloc(&P->work, nwork*P->esz);
    if (!e)
    {
        fft_acquire();
        e = slab_fft_plans(P, 1, &P->wbs);
        if (!e && rocfft_execution_info_create(&P->info) != rocfft_status_success) { set_error("FFT error: execution_info_create"); e = MHH_EFFT; }
        if (!e && P->wbs)
        {
            alloc(&P->wb, P->wbs); P->wb_cap = P->wbs;
            if (!e && rocfft_execution_info_set_work_buffer(P->info, P->wb, P->wbs) != rocfft_status_success) { set_error("FFT error: set_work_buffer"); e = MHH_EFFT; }
        }
    }
    if (!e) e = slab_factor(P);
    if (!e && order == 2 && lds_slab_usable(g)) { e = lds_twiddles(g->itot, g->dtype, &P->tx_lds); if (!e) e = lds_twiddles(g->jtot, g->dtype, &P->ty_lds); }      // the transforms in LDS
    if (e) { mhh_pres_slab_plan_destroy(P); return e; }
    *out = P;
    return MHH_OK;
}
MHH_API int mhh_pres_slab_plan_create(const mhh_grid* g, const void* host_dz, const void* host_dzhi, const void* host_rhoref, const void* host_rhorefh,
                                      mhh_pres_slab_plan** out)
{
    return mhh_pres_slab_plan_create_order(g, 2, host_dz, host_dzhi, nullptr, nullptr, host_rhoref, host_rhorefh, out);
}
MHH_API int mhh_pres_slab_order(const mhh_pres_slab_plan* P) { return P ? P->order : 0; }
MHH_API unsigned long long mhh_pres_slab_xbuf_elems(const mhh_pres_slab_plan* P)   // complex elements of one all-to-all buffer
{
    return (unsigned long long)P->npy * P->ktot * P->jmax * P->nxb;
}
MHH_API void* mhh_pres_slab_packed(mhh_pres_slab_plan* P) { return P->packed; }

// specx [k][jl][kx] -> xbuf [q][k][jl][kxl] (FWD) and back (the reverse direction drops the zero padding)
template<class TF, bool FWD>
__global__ void __launch_bounds__(256) xbuf_x_kernel(C2<TF>* __restrict__ specx, C2<TF>* __restrict__ xbuf, int nxh, int nxb, int jmax, int ktot, int npy)
{
    const int kx = blockIdx.x*256 + threadIdx.x;          // 0 .. npy*nxb-1
    const int jl = blockIdx.y, k = blockIdx.z;
    if (kx >= npy*nxb) return;
    const int q = kx / nxb, kxl = kx - q*nxb;
    const size_t xb = (((size_t)q*ktot + k)*jmax + jl)*nxb + kxl;
    const size_t sx = ((size_t)k*jmax + jl)*nxh + kx;
    if (FWD) xbuf[xb] = (kx < nxh) ? specx[sx] : C2<TF>{0, 0};
    else if (kx < nxh) specx[sx] = xbuf[xb];
}
// xbuf [r][k][jl][kxl] <-> specy [k][kxl][j = r*jmax + jl]: per (k, r) a 2-D transpose of a (jmax x nxb) matrix of complex
// numbers, done through an LDS tile of 64 (j) x 32 (kxl) so that both the global reads and the global writes are
// contiguous runs (512 B rows on the xbuf side, 1 KB rows on the specy side). The tile rows are padded by one element:
// a transposed ds_read_b128 then touches 16 different 4-bank groups per lane group (no conflicts).
template<class TF, bool FWD>
__global__ void __launch_bounds__(256) xbuf_y_kernel(C2<TF>* __restrict__ specy, C2<TF>* __restrict__ xbuf, int nxb, int jmax, int jtot, int ktot)
{
    constexpr int TJ = 64, TX = 32;
    __shared__ C2<TF> tile[TJ][TX+1];
    const int ntx = (nxb + TX-1)/TX, njl = (jmax + TJ-1)/TJ;
    int b = blockIdx.x;
    const int txi = b % ntx; b /= ntx;
    const int jli = b % njl; const int r = b / njl;
    const int k = blockIdx.y;
    const int kx0 = txi*TX, jl0 = jli*TJ;
    const int t = threadIdx.x;
    const size_t xb0 = ((size_t)r*ktot + k)*jmax*nxb;            // start of the (r,k) matrix [jl][kxl]
    const size_t sy0 = (size_t)k*nxb*jtot + (size_t)r*jmax;      // specy element (k, kxl=0, j=r*jmax)
    if (FWD)
    {
        // all eight loads of a thread are requested before the first is used (clamped addresses, no branch between them): as
        // load - store pairs under a condition they were eight memory round trips in a row
        C2<TF> v[TJ*TX/256];
#pragma unroll
        for (int p = 0; p < TJ*TX/256; ++p)                      // 8 passes: 8 rows x 32 columns each
        {
            const int row = p*8 + t/32, cx = t % 32;
            const int jl = jl0 + row, kxl = kx0 + cx;
            const bool in = (jl < jmax && kxl < nxb);
            v[p] = xbuf[xb0 + (in ? (size_t)jl*nxb + kxl : (size_t)0)];
        }
#pragma unroll
        for (int p = 0; p < TJ*TX/256; ++p)
        {
            const int row = p*8 + t/32, cx = t % 32;
            if (jl0 + row < jmax && kx0 + cx < nxb) tile[row][cx] = v[p];
        }
        __syncthreads();
        for (int p = 0; p < TJ*TX/256; ++p)                      // 8 passes: 4 columns x 64 rows each
        {
            const int cx = p*4 + t/64, row = t % 64;
            const int jl = jl0 + row, kxl = kx0 + cx;
            if (jl < jmax && kxl < nxb) specy[sy0 + (size_t)kxl*jtot + jl] = tile[row][cx];
        }
    }
    else
    {
        C2<TF> v[TJ*TX/256];
#pragma unroll
        for (int p = 0; p < TJ*TX/256; ++p)
        {
            const int cx = p*4 + t/64, row = t % 64;
            const int jl = jl0 + row, kxl = kx0 + cx;
            const bool in = (jl < jmax && kxl < nxb);
            v[p] = specy[sy0 + (in ? (size_t)kxl*jtot + jl : (size_t)0)];
        }
#pragma unroll
        for (int p = 0; p < TJ*TX/256; ++p)
        {
            const int cx = p*4 + t/64, row = t % 64;
            if (jl0 + row < jmax && kx0 + cx < nxb) tile[row][cx] = v[p];
        }
        __syncthreads();
        for (int p = 0; p < TJ*TX/256; ++p)
        {
            const int row = p*8 + t/32, cx = t % 32;
            const int jl = jl0 + row, kxl = kx0 + cx;
            if (jl < jmax && kxl < nxb) xbuf[xb0 + (size_t)jl*nxb + kxl] = tile[row][cx];
        }
    }
}

// Thomas solve of the slab stage (src/pres_2.cxx:289-330 matrix, :202-263 tdma) on the rank's (x-block, all y) columns.
// A rank has only nxb*jtot columns (33 x 512 at 512^3 on 8 GPUs: half a wave per SIMD), so the sweep is latency-bound
// and organised for that:
//   * the pivots w2 and the eliminated upper diagonal w3 depend on the grid and (kx, ky) only: computed ONCE at plan
//     creation (tdma_slab_factor_kernel, the reference's recurrence) and kept, 2 x nxb*jtot*kmax values;
//   * one thread per (ky, re|im) component -- twice the parallelism, lanes still read consecutive 8-byte words;
//   * the right-hand side and pivots of the next 16 levels are loaded while the 16 current levels run through the
//     recurrence (only a multiply-subtract and the division by the pivot are left on the dependent chain).
template<class TF>
__global__ void __launch_bounds__(64) tdma_slab_factor_kernel(TF* __restrict__ W2, TF* __restrict__ W3,
                                                              const TF* __restrict__ bmati, const TF* __restrict__ bmatj,
                                                              const TF* __restrict__ a, const TF* __restrict__ c, const TF* __restrict__ dz, const TF* __restrict__ rho,
                                                              int nxh, int nxb, int kx0, int jtot, int kmax)
{
    const int ky = blockIdx.x*64 + threadIdx.x, kxl = blockIdx.y;
    const int kx = kx0 + kxl;
    if (ky >= jtot || kx >= nxh) return;
    const size_t kk = (size_t)nxb*jtot, col = (size_t)kxl*jtot + ky;
    const TF bm = bmati[kx] + bmatj[ky];
    const bool mean = (kx == 0 && ky == 0);
    TF w2;
    {
        const TF dz2 = dz[0]*dz[0];
        TF b = dz2 * rho[0]*bm - (a[0]+c[0]);
        b += a[0];
        if (kmax == 1) { if (mean) b -= c[0]; else b += c[0]; }
        w2 = b;
        W2[col] = w2; W3[col] = TF(0);
    }
    for (int k=1; k<kmax; ++k)
    {
        const TF dz2 = dz[k]*dz[k];
        TF b = dz2 * rho[k]*bm - (a[k]+c[k]);
        if (k == kmax-1) { if (mean) b -= c[k]; else b += c[k]; }
        const TF w3 = c[k-1] / w2;
        w2 = b - a[k]*w3;
        W2[col + (size_t)k*kk] = w2; W3[col + (size_t)k*kk] = w3;
    }
}
template<class TF>
__global__ void __launch_bounds__(128) tdma_slab_kernel(TF* __restrict__ p, const TF* __restrict__ W2, const TF* __restrict__ W3,
                                                        const TF* __restrict__ a, const TF* __restrict__ dz,
                                                        int nxh, int nxb, int kx0, int jtot, int kmax)
{
#ifndef MHH_SLAB_U
#define MHH_SLAB_U 16          // levels in flight per thread (512^3 / 8: y-stage 0.44 ms with 8, 0.41 with 16, 0.40 with 32)
#endif
    constexpr int U = MHH_SLAB_U;
    const int t = blockIdx.x*128 + threadIdx.x;           // 0 .. 2*jtot-1
    const int ky = t >> 1, comp = t & 1, kxl = blockIdx.y;
    const int kx = kx0 + kxl;                              // swapped indices: this rank owns a block of x modes, all y modes
    if (ky >= jtot || kx >= nxh) return;
    const size_t kk = (size_t)nxb*jtot, col = (size_t)kxl*jtot + ky;
    TF* __restrict__ q = p + 2*col + comp;                 // component stream, stride 2*kk per level
    const TF* __restrict__ w2 = W2 + col; const TF* __restrict__ w3 = W3 + col;
    TF pp;
    {
        TF v = dz[0]*dz[0] * q[0];
        v /= w2[0];
        q[0] = v; pp = v;
    }
    // forward sweep, levels 1 .. kmax-1 in blocks of U with the next block's operands in flight
    TF qc[U], wc[U];
#pragma unroll
    for (int u=0; u<U; ++u) { const int k = 1 + u; const bool ok = k < kmax; qc[u] = ok ? q[2*(size_t)k*kk] : TF(0); wc[u] = ok ? w2[(size_t)k*kk] : TF(1); }
    for (int k0=1; k0<kmax; k0+=U)
    {
        TF qn[U], wn[U];
#pragma unroll
        for (int u=0; u<U; ++u) { const int k = k0 + U + u; const bool ok = k < kmax; qn[u] = ok ? q[2*(size_t)k*kk] : TF(0); wn[u] = ok ? w2[(size_t)k*kk] : TF(1); }
#pragma unroll
        for (int u=0; u<U; ++u)
        {
            const int k = k0 + u;
            if (k < kmax)
            {
                TF v = dz[k]*dz[k] * qc[u];
                v -= a[k]*pp;
                v /= wc[u];
                q[2*(size_t)k*kk] = v; pp = v;
            }
        }
#pragma unroll
        for (int u=0; u<U; ++u) { qc[u] = qn[u]; wc[u] = wn[u]; }
    }
    // backward sweep, levels kmax-2 .. 0
#pragma unroll
    for (int u=0; u<U; ++u) { const int k = kmax-2 - u; const bool ok = k >= 0; qc[u] = ok ? q[2*(size_t)k*kk] : TF(0); wc[u] = ok ? w3[(size_t)(k+1)*kk] : TF(0); }
    for (int k0=kmax-2; k0>=0; k0-=U)
    {
        TF qn[U], wn[U];
#pragma unroll
        for (int u=0; u<U; ++u) { const int k = k0 - U - u; const bool ok = k >= 0; qn[u] = ok ? q[2*(size_t)k*kk] : TF(0); wn[u] = ok ? w3[(size_t)(k+1)*kk] : TF(0); }
#pragma unroll
        for (int u=0; u<U; ++u)
        {
            const int k = k0 - u;
            if (k >= 0)
            {
                TF v = qc[u];
                v -= wc[u]*pp;
                q[2*(size_t)k*kk] = v; pp = v;
            }
        }
#pragma unroll
        for (int u=0; u<U; ++u) { qc[u] = qn[u]; wc[u] = wn[u]; }
    }
}

// The 7-band solve of pres_4 (src/pres_4.cxx:358-470 matrix, :574-730 hdma) on the rank's (x-block, all y) columns. Latency-bound
// like the Thomas sweep above (33 x 256 columns per rank at moser600 on 8 GPUs: a quarter of a wave per SIMD, 260 dependent rows per
// sweep), and organised the same way:
//   * the LU factors depend on the grid and (kx, ky) only: computed ONCE at plan creation by the single-GPU plan's own column
//     factorisation (hdma_factor_column, pres4_bands.h) in the slab column order col = kxl*jtot + ky, band n (0..6), row r at
//     W[(n*(kmax+4) + r)*ncol + col] -- 7*(kmax+4)*nxb*jtot values. The pivots (band 3) are kept as reciprocals (as the LDS
//     form's pres4_lds_factor_kernel does), so that no division is left in the sweeps;
//   * one thread per (ky, re|im) component, in place on specy [k][kxl][ky] (row r of the system = level r-2; the two boundary rows
//     on either side carry a zero right-hand side and live in registers);
//   * the right-hand side and the factors of the next U levels are loaded while the U current levels run through the
//     recurrence, whose terms are ordered so that only one multiply-subtract (and the multiply by the reciprocal pivot on the way
//     back) waits for the row before.
template<class TF>
__global__ void __launch_bounds__(64) hdma_slab_factor_kernel(TF* __restrict__ W, const TF* __restrict__ bmati, const TF* __restrict__ bmatj,
                                                              const TF* __restrict__ M1, const TF* __restrict__ M2, const TF* __restrict__ M3, const TF* __restrict__ M4,
                                                              const TF* __restrict__ M5, const TF* __restrict__ M6, const TF* __restrict__ M7,
                                                              int nxh, int nxb, int kx0, int jtot, int kmax)
{
    const int ky = blockIdx.x*64 + threadIdx.x, kxl = blockIdx.y;
    const int kx = kx0 + kxl;
    if (ky >= jtot || kx >= nxh) return;
    const size_t ncol = (size_t)nxb*jtot, col = (size_t)kxl*jtot + ky, bstride = (size_t)(kmax+4)*ncol;
    TF* __restrict__ Wc = W + col;
    hdma_factor_column(Wc, ncol, bstride, bmati[kx], bmatj[ky], kx == 0 && ky == 0, M1, M2, M3, M4, M5, M6, M7, kmax);
    for (int r=0; r<kmax+4; ++r) Wc[3*bstride + (size_t)r*ncol] = TF(1.) / Wc[3*bstride + (size_t)r*ncol];
}
template<class TF>
__global__ void __launch_bounds__(128) hdma_slab_kernel(TF* __restrict__ p, const TF* __restrict__ W, int nxh, int nxb, int kx0, int jtot, int kmax)
{
#ifndef MHH_SLAB4_U
#define MHH_SLAB4_U 8          // levels in flight per thread
#endif
    constexpr int U = MHH_SLAB4_U;
    const int t = blockIdx.x*128 + threadIdx.x;           // 0 .. 2*jtot-1
    const int ky = t >> 1, comp = t & 1, kxl = blockIdx.y;
    const int kx = kx0 + kxl;
    if (ky >= jtot || kx >= nxh) return;
    const size_t ncol = (size_t)nxb*jtot, col = (size_t)kxl*jtot + ky, bs = (size_t)(kmax+4)*ncol;
    TF* __restrict__ q = p + 2*col + comp;                 // level l of this component at q[2*l*ncol]
    const TF* __restrict__ m1 = W + col;        const TF* __restrict__ m2 = m1 + bs;   const TF* __restrict__ m3 = m1 + 2*bs;
    const TF* __restrict__ r4 = m1 + 3*bs;      const TF* __restrict__ m5 = m1 + 4*bs; const TF* __restrict__ m6 = m1 + 5*bs;
    const TF* __restrict__ m7 = m1 + 6*bs;
#define A(arr, r) arr[(size_t)(r)*ncol]
    // the factors of the two top rows (kmax+2, kmax+3), needed between the sweeps
    const int rt = kmax+2;
    const TF t1a = A(m1,rt), t2a = A(m2,rt), t3a = A(m3,rt), t1b = A(m1,rt+1), t2b = A(m2,rt+1), t3b = A(m3,rt+1);
    const TF r4a = A(r4,rt), r4b = A(r4,rt+1), t5a = A(m5,rt);
    // L y = q: y_r = q_r - m1_r y_{r-3} - m2_r y_{r-2} - m3_r y_{r-1}; rows 0 and 1 give y = 0
    TF a1 = TF(0), a2 = TF(0), a3 = TF(0);                 // y_{r-1}, y_{r-2}, y_{r-3}
    {
        TF qc[U], c1[U], c2[U], c3[U];
#pragma unroll
        for (int u=0; u<U; ++u) { const int l = u; const bool ok = l < kmax; const int r = ok ? l+2 : 0;
                                  qc[u] = ok ? q[2*(size_t)l*ncol] : TF(0); c1[u] = A(m1,r); c2[u] = A(m2,r); c3[u] = A(m3,r); }
        for (int l0=0; l0<kmax; l0+=U)
        {
            TF qn[U], n1[U], n2[U], n3[U];
#pragma unroll
            for (int u=0; u<U; ++u) { const int l = l0 + U + u; const bool ok = l < kmax; const int r = ok ? l+2 : 0;
                                      qn[u] = ok ? q[2*(size_t)l*ncol] : TF(0); n1[u] = A(m1,r); n2[u] = A(m2,r); n3[u] = A(m3,r); }
#pragma unroll
            for (int u=0; u<U; ++u)
            {
                const int l = l0 + u;
                if (l < kmax)
                {
                    TF v = qc[u] - c1[u]*a3;
                    v -= c2[u]*a2;
                    v -= c3[u]*a1;
                    q[2*(size_t)l*ncol] = v;
                    a3 = a2; a2 = a1; a1 = v;
                }
            }
#pragma unroll
            for (int u=0; u<U; ++u) { qc[u] = qn[u]; c1[u] = n1[u]; c2[u] = n2[u]; c3[u] = n3[u]; }
        }
    }
    TF ya = TF(0) - t1a*a3; ya -= t2a*a2; ya -= t3a*a1;    // row kmax+2
    TF yb = TF(0) - t1b*a2; yb -= t2b*a1; yb -= t3b*ya;    // row kmax+3
    // U x = y: x_r = (y_r - m7_r x_{r+3} - m6_r x_{r+2} - m5_r x_{r+1}) / m4_r, from the top
    TF b2 = yb * r4b;                                      // x_{kmax+3}
    TF b1 = (ya - t5a*b2) * r4a;                           // x_{kmax+2}
    TF b3 = TF(0);                                         // (no row kmax+4)
    {
        TF qc[U], c5[U], c6[U], c7[U], c4[U];
#pragma unroll
        for (int u=0; u<U; ++u) { const int l = kmax-1 - u; const bool ok = l >= 0; const int r = ok ? l+2 : 0;
                                  qc[u] = ok ? q[2*(size_t)l*ncol] : TF(0); c5[u] = A(m5,r); c6[u] = A(m6,r); c7[u] = A(m7,r); c4[u] = A(r4,r); }
        for (int l0=kmax-1; l0>=0; l0-=U)
        {
            TF qn[U], n5[U], n6[U], n7[U], n4[U];
#pragma unroll
            for (int u=0; u<U; ++u) { const int l = l0 - U - u; const bool ok = l >= 0; const int r = ok ? l+2 : 0;
                                      qn[u] = ok ? q[2*(size_t)l*ncol] : TF(0); n5[u] = A(m5,r); n6[u] = A(m6,r); n7[u] = A(m7,r); n4[u] = A(r4,r); }
#pragma unroll
            for (int u=0; u<U; ++u)
            {
                const int l = l0 - u;
                if (l >= 0)
                {
                    TF v = qc[u] - c7[u]*b3;
                    v -= c6[u]*b2;
                    v -= c5[u]*b1;
                    v *= c4[u];
                    q[2*(size_t)l*ncol] = v;
                    b3 = b2; b2 = b1; b1 = v;
                }
            }
#pragma unroll
            for (int u=0; u<U; ++u) { qc[u] = qn[u]; c5[u] = n5[u]; c6[u] = n6[u]; c7[u] = n7[u]; c4[u] = n4[u]; }
        }
    }
#undef A
}

// the launches of the factor and sweep kernels of the plan's order on TF
template<class TF>
static void slab_factor_launch(mhh_pres_slab_plan* P)
{
    dim3 gf((P->jtot + 63)/64, P->nxb);
    const size_t ny = (size_t)P->nxb*P->jtot*P->ktot;
    if (P->order == 4)
        hipLaunchKernelGGL(hdma_slab_factor_kernel<TF>, gf, dim3(64), 0, 0, mp<TF>(P->work), cp<TF>(P->bmati), cp<TF>(P->bmatj),
                           cp<TF>(P->m[0]), cp<TF>(P->m[1]), cp<TF>(P->m[2]), cp<TF>(P->m[3]), cp<TF>(P->m[4]), cp<TF>(P->m[5]), cp<TF>(P->m[6]),
                           P->nxh, P->nxb, P->rank*P->nxb, P->jtot, P->ktot);
    else
        hipLaunchKernelGGL(tdma_slab_factor_kernel<TF>, gf, dim3(64), 0, 0, mp<TF>(P->work), mp<TF>(P->work) + ny, cp<TF>(P->bmati), cp<TF>(P->bmatj),
                           cp<TF>(P->a), cp<TF>(P->c), cp<TF>(P->dz), cp<TF>(P->rhoref), P->nxh, P->nxb, P->rank*P->nxb, P->jtot, P->ktot);
}
template<class TF>
static void slab_solve_launch(mhh_pres_slab_plan* P, hipStream_t st)
{
    const size_t ny = (size_t)P->nxb*P->jtot*P->ktot;
    dim3 gs((2*P->jtot + 127)/128, P->nxb);
    if (P->order == 4)
        hipLaunchKernelGGL(hdma_slab_kernel<TF>, gs, dim3(128), 0, st, mp<TF>(P->specy), cp<TF>(P->work), P->nxh, P->nxb, P->rank*P->nxb, P->jtot, P->ktot);
    else
        hipLaunchKernelGGL(tdma_slab_kernel<TF>, gs, dim3(128), 0, st, mp<TF>(P->specy), cp<TF>(P->work), cp<TF>(P->work) + ny,
                           cp<TF>(P->a), cp<TF>(P->dz), P->nxh, P->nxb, P->rank*P->nxb, P->jtot, P->ktot);
}
static int slab_factor(mhh_pres_slab_plan* P)
{
#define CALL(TF) slab_factor_launch<TF>(P)
    MHH_DISPATCH(P, CALL);
#undef CALL
    hipError_t h = hipGetLastError(); if (h == hipSuccess) h = hipStreamSynchronize(0);
    if (h != hipSuccess) { set_error("%s: %s", P->order == 4 ? "hdma_slab_factor" : "tdma_slab_factor", hipGetErrorString(h)); return MHH_EHIP; }
    return MHH_OK;
}
// the k-sweeps of every column of the rank's slab on specy: Thomas (pres_2) or the factored 7-band substitution (pres_4)
static int slab_column_solve(mhh_pres_slab_plan* P, hipStream_t st)
{
#define CALL(TF) slab_solve_launch<TF>(P, st)
    MHH_DISPATCH(P, CALL);
#undef CALL
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// packed real [k][jl][i] -> ghosted p: interior rows + x halo (wrap) + the mirrored vertical ghost levels (src/pres_2.cxx:333-362:
// the bottom one; src/pres_4.cxx:481-528: two at the bottom, two at the top); the y halo is the caller's exchange.
// blockIdx.z = kmax + 1 (pres_2) or kmax + 4 (pres_4) levels.
template<class TF>
__global__ void __launch_bounds__(256) unpack_slab_kernel(TF* __restrict__ p, const TF* __restrict__ packed, int order, int itot, int jtot, int jmax, int kmax,
                                                          int igc, int jgc, int kgc, int icells, int jcells)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    const int jl = blockIdx.y, kz = blockIdx.z;
    if (i >= icells) return;
    int kd, ks;
    if (kz < kmax)       { kd = kz + kgc;      ks = kz; }
    else if (order == 2) { kd = kgc - 1;       ks = 0; }          // p[kstart-1] = p[kstart]
    else
    {
        const int gidx = kz - kmax;                                 // 0..3
        if (gidx == 0)      { kd = kgc - 1;        ks = 0; }        // p[kstart-1] = p[kstart]
        else if (gidx == 1) { kd = kgc - 2;        ks = 1; }        // p[kstart-2] = p[kstart+1]
        else if (gidx == 2) { kd = kgc + kmax;     ks = kmax-1; }   // p[kend]     = p[kend-1]
        else                { kd = kgc + kmax + 1; ks = kmax-2; }   // p[kend+1]   = p[kend-2]
    }
    int is = (i - igc) % itot; if (is < 0) is += itot;
    const TF val = packed[(size_t)is + (size_t)jl*itot + (size_t)ks*itot*jmax] / jtot / itot;
    p[(size_t)i + (size_t)(jl + jgc)*icells + (size_t)kd*icells*jcells] = val;
}

// unpack and Pres_2::output in one pass on a slab (as unpack_out2_kernel of k_pres.hip): p of the rank's own rows, and on
// interior cells ut, wt and -- for every row but the southernmost, whose p[j-1] lives on the south neighbour -- vt, with the
// neighbours re-normalised from the packed solution (the stored values). The southernmost row of vt follows the one-row
// halo exchange of p (pres_out_south_row_kernel).
template<bool POW2, class TF>
__global__ void __launch_bounds__(256) unpack_out_slab_kernel(TF* __restrict__ p, const TF* __restrict__ packed,
                                                              TF* __restrict__ ut, TF* __restrict__ vt, TF* __restrict__ wt, const TF* __restrict__ dzhi,
                                                              TF dxi, TF dyi, int itot, int jtot, int jmax, int kmax, int igc, int jgc, int kgc, int icells, int jcells)
{
    const int i = blockIdx.x*256 + threadIdx.x;
    const int jl = blockIdx.y, kz = blockIdx.z;
    if (i >= icells) return;
    const int kd = (kz < kmax) ? kz + kgc : kgc - 1;
    const int ks = (kz < kmax) ? kz : 0;
    int is = (i - igc) % itot; if (is < 0) is += itot;
    const size_t ijm = (size_t)itot*jmax;
    const TF ri = TF(1)/TF(itot), rj = TF(1)/TF(jtot);
    const TF pc = fft_norm<POW2>(packed[(size_t)is + (size_t)jl*itot + (size_t)ks*ijm], itot, jtot, ri, rj);
    const size_t c = (size_t)i + (size_t)(jl + jgc)*icells + (size_t)kd*icells*jcells;
    p[c] = pc;
    if (kz < kmax && i >= igc && i < igc + itot)
    {
        const int iw = (is == 0) ? itot-1 : is-1;
        const TF pw = fft_norm<POW2>(packed[(size_t)iw + (size_t)jl*itot + (size_t)ks*ijm], itot, jtot, ri, rj);
        const TF pb = (ks == 0) ? pc : fft_norm<POW2>(packed[(size_t)is + (size_t)jl*itot + (size_t)(ks-1)*ijm], itot, jtot, ri, rj);
        ut[c] -= (pc - pw) * dxi;
        if (jl > 0)
        {
            const TF ps = fft_norm<POW2>(packed[(size_t)is + (size_t)(jl-1)*itot + (size_t)ks*ijm], itot, jtot, ri, rj);
            vt[c] -= (pc - ps) * dyi;
        }
        wt[c] -= (pc - pb) * dzhi[kd];
    }
}
template<class TF>
__global__ void __launch_bounds__(256) pres_out_south_row_kernel(TF* __restrict__ vt, const TF* __restrict__ p, TF dyi, int istart, int iend, int jstart, int kstart, int icells, int ijcells)
{
    const int i = istart + blockIdx.x*256 + threadIdx.x;
    if (i >= iend) return;
    const size_t c = (size_t)i + (size_t)jstart*icells + (size_t)(kstart + blockIdx.y)*ijcells;
    vt[c] -= (p[c] - p[c-icells]) * dyi;
}

static int slab_match(const mhh_pres_slab_plan* P, const mhh_grid* g)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(P && P->dtype == g->dtype && P->itot == g->itot && P->jtot == g->jtot && P->ktot == g->ktot && P->jmax == g->jmax && P->npy == g->npy && P->rank == g->mpicoordy, "plan/grid mismatch");
    return MHH_OK;
}

// =======================================================================================================
// The solve works in nchunks k-slices (src/fft.cxx:451-583 transforms the planes of a field one k-slice at a time too; one slice =
// all levels): the buffers of the all-to-alls are laid out [slice][peer][k in slice][jl][kxl], so that slice c is ONE equal-split
// all-to-all of its own, which the host issues on a second stream while slice c+1 is being transformed (microhh_amd/model.py:
// HotPath.pres). Every plane goes through the same transform kernels whatever the slice count; the column solves need all slices.
// =======================================================================================================
MHH_API int mhh_pres_slab_set_chunks(mhh_pres_slab_plan* P, int nchunks)
{
    MHH_REQUIRE(P && nchunks >= 1 && P->ktot % nchunks == 0, "the number of k-slices must divide ktot");
    if (nchunks == P->nchunks) return MHH_OK;
    size_t wbs = P->wbs;
    int e = slab_fft_plans(P, nchunks, &wbs);
    if (!e && wbs > P->wb_cap)
    {
        MHH_HIP_TRY(hipStreamSynchronize(0));          // (the work buffer may still be in use by a solve in flight on the default stream)
        if (P->wb) (void)hipFree(P->wb);
        MHH_HIP_TRY(hipMalloc(&P->wb, wbs)); P->wb_cap = wbs;
        MHH_FFT_TRY(rocfft_execution_info_set_work_buffer(P->info, P->wb, wbs));
    }
    P->wbs = wbs;
    return e;
}
MHH_API int mhh_pres_slab_chunks(const mhh_pres_slab_plan* P) { return P ? P->nchunks : 0; }

namespace
{
struct Slice { int kc; size_t xseg, sx, sy, pk; };      // levels per slice; element offsets of slice c in xbuf / specx / specy / packed
inline Slice slice_of(const mhh_pres_slab_plan* P, int c)
{
    const int kc = P->ktot / P->nchunks;
    return Slice{kc, (size_t)c*P->npy*kc*P->jmax*P->nxb, (size_t)c*kc*P->jmax*P->nxh, (size_t)c*kc*P->nxb*P->jtot, (size_t)c*kc*P->jmax*P->itot};
}
inline int chunk_ok(const mhh_pres_slab_plan* P, const mhh_grid* g, int c)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(c >= 0 && c < P->nchunks, "k-slice index (mhh_pres_slab_set_chunks sets their number)");
    return MHH_OK;
}
// the calls without a slice index work all levels at once: slice 0 of a plan that has one slice
const char* const ONE_SLICE = "this plan works in k-slices: call mhh_pres_slab_set_chunks(plan, 1) first, or the per-slice entry points";

// one transform of slice-sized batch on `st`
inline int slab_fft(mhh_pres_slab_plan* P, rocfft_plan plan, void* in, void* out, hipStream_t st)
{
    MHH_FFT_TRY(rocfft_execution_info_set_stream(P->info, st));
    void* i[1] = {in}; void* o[1] = {out};
    MHH_FFT_TRY(rocfft_execute(plan, i, out ? o : nullptr, P->info));
    return MHH_OK;
}
// specx of the slice <-> its segment of an all-to-all buffer; the same for specy
template<class TF, bool FWD>
int xbuf_x(mhh_pres_slab_plan* P, const Slice& sl, void* xbuf, hipStream_t st)
{
    hipLaunchKernelGGL((xbuf_x_kernel<TF, FWD>), dim3((P->npy*P->nxb + 255)/256, P->jmax, sl.kc), dim3(256), 0, st,
                       (C2<TF>*)P->specx + sl.sx, (C2<TF>*)xbuf + sl.xseg, P->nxh, P->nxb, P->jmax, sl.kc, P->npy);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
template<class TF, bool FWD>
int xbuf_y(mhh_pres_slab_plan* P, const Slice& sl, void* xbuf, hipStream_t st)
{
    hipLaunchKernelGGL((xbuf_y_kernel<TF, FWD>), dim3((unsigned)(((P->nxb + 31)/32) * ((P->jmax + 63)/64) * P->npy), sl.kc), dim3(256), 0, st,
                       (C2<TF>*)P->specy + sl.sy, (C2<TF>*)xbuf + sl.xseg, P->nxb, P->jmax, P->jtot, sl.kc);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// ---- the stages of the solve on one slice ----
// x transform of the packed divergence + pack into the slice's segment of sendbuf
int stage_fwd_x(mhh_pres_slab_plan* P, const Slice& sl, void* p_packed, void* sendbuf, hipStream_t st)
{
    if (!p_packed) p_packed = P->packed;
    if (int e = slab_fft(P, P->fx, static_cast<char*>(p_packed) + sl.pk*P->esz, static_cast<char*>(P->specx) + sl.sx*2*P->esz, st)) return e;
#define CALL(TF) xbuf_x<TF, true>(P, sl, sendbuf, st)
    return MHH_DISPATCH(P, CALL);
#undef CALL
}
// after the slice's forward all-to-all: reorder into [k][kxl][j] and forward y transform
int stage_fwd_y(mhh_pres_slab_plan* P, const Slice& sl, void* recvbuf, hipStream_t st)
{
#define CALL(TF) xbuf_y<TF, true>(P, sl, recvbuf, st)
    if (int e = MHH_DISPATCH(P, CALL)) return e;
#undef CALL
    return slab_fft(P, P->fy, static_cast<char*>(P->specy) + sl.sy*2*P->esz, nullptr, st);
}
// (all slices in: slab_column_solve)  inverse y transform + reorder into the slice's segment of sendbuf
int stage_bwd_y(mhh_pres_slab_plan* P, const Slice& sl, void* sendbuf, hipStream_t st)
{
    if (int e = slab_fft(P, P->by, static_cast<char*>(P->specy) + sl.sy*2*P->esz, nullptr, st)) return e;
#define CALL(TF) xbuf_y<TF, false>(P, sl, sendbuf, st)
    return MHH_DISPATCH(P, CALL);
#undef CALL
}
// after the slice's backward all-to-all: back into [k][jl][kx] and inverse x transform into the packed solution
int stage_bwd_x(mhh_pres_slab_plan* P, const Slice& sl, void* recvbuf, hipStream_t st)
{
#define CALL(TF) xbuf_x<TF, false>(P, sl, recvbuf, st)
    if (int e = MHH_DISPATCH(P, CALL)) return e;
#undef CALL
    return slab_fft(P, P->bx, static_cast<char*>(P->specx) + sl.sx*2*P->esz, static_cast<char*>(P->packed) + sl.pk*P->esz, st);
}
// all slices back: the packed solution into p (unpack_slab_kernel) ...
template<class TF>
int unpack(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, hipStream_t st)
{
    hipLaunchKernelGGL(unpack_slab_kernel<TF>, dim3((g->icells + 255)/256, g->jmax, g->kmax + (P->order == 2 ? 1 : 4)), dim3(256), 0, st, mp<TF>(f->p), cp<TF>(P->packed),
                       P->order, g->itot, g->jtot, g->jmax, g->kmax, g->igc, g->jgc, g->kgc, g->icells, g->jcells);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
int stage_unpack(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, hipStream_t st)
{
#define CALL(TF) unpack<TF>(P, g, f, st)
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
// ... or into p with Pres_2::output applied in the same kernel (unpack_out_slab_kernel)
template<bool POW2, class TF>
int unpack_output(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, hipStream_t st)
{
    const GridDev<TF> gd = make_grid<TF>(g);
    hipLaunchKernelGGL((unpack_out_slab_kernel<POW2, TF>), dim3((g->icells + 255)/256, g->jmax, g->kmax + 1), dim3(256), 0, st, mp<TF>(f->p), cp<TF>(P->packed),
                       mp<TF>(f->ut), mp<TF>(f->vt), mp<TF>(f->wt), gd.dzhi, gd.dxi_t, gd.dyi_t, g->itot, g->jtot, g->jmax, g->kmax, g->igc, g->jgc, g->kgc, g->icells, g->jcells);
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}
int stage_unpack_output(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, hipStream_t st)
{
    const bool pow2 = is_pow2(g->itot) && is_pow2(g->jtot);
#define CALL(TF) (pow2 ? unpack_output<true, TF>(P, g, f, st) : unpack_output<false, TF>(P, g, f, st))
    return MHH_DISPATCH(g, CALL);
#undef CALL
}
}

// ---- per slice c ----
MHH_API int mhh_pres_fwd_x_pack_chunk(mhh_pres_slab_plan* P, const mhh_grid* g, void* p_packed, void* sendbuf, int c, void* stream)
{
    if (int e = chunk_ok(P, g, c)) return e;
    MHH_REQUIRE(sendbuf != nullptr, "sendbuf");
    return stage_fwd_x(P, slice_of(P, c), p_packed, sendbuf, as_stream(stream));
}
MHH_API int mhh_pres_fwd_y_chunk(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, int c, void* stream)
{
    if (int e = chunk_ok(P, g, c)) return e;
    MHH_REQUIRE(recvbuf != nullptr, "recvbuf");
    return stage_fwd_y(P, slice_of(P, c), recvbuf, as_stream(stream));
}
// all slices in: the tridiagonal (pres_2) or 7-band (pres_4) solves over k
MHH_API int mhh_pres_solve_y(mhh_pres_slab_plan* P, const mhh_grid* g, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    return slab_column_solve(P, as_stream(stream));
}
MHH_API int mhh_pres_bwd_y_chunk(mhh_pres_slab_plan* P, const mhh_grid* g, void* sendbuf, int c, void* stream)
{
    if (int e = chunk_ok(P, g, c)) return e;
    MHH_REQUIRE(sendbuf != nullptr, "sendbuf");
    return stage_bwd_y(P, slice_of(P, c), sendbuf, as_stream(stream));
}
MHH_API int mhh_pres_bwd_x_chunk(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, int c, void* stream)
{
    if (int e = chunk_ok(P, g, c)) return e;
    MHH_REQUIRE(recvbuf != nullptr, "recvbuf");
    return stage_bwd_x(P, slice_of(P, c), recvbuf, as_stream(stream));
}
// all slices back
MHH_API int mhh_pres_unpack_slab(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(f && f->p, "buffers");
    return stage_unpack(P, g, f, as_stream(stream));
}
// the caller then exchanges the one-row halo of p and finishes vt on the southernmost row with mhh_pres_output_south_row
MHH_API int mhh_pres_unpack_output_slab(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "Pres_2::output only: a pres_4 plan takes mhh_pres_unpack_slab, the halo of p and mhh_pres_output_order(g, 4)");
    MHH_REQUIRE(f && f->p && f->ut && f->vt && f->wt, "buffers");
    return stage_unpack_output(P, g, f, as_stream(stream));
}

// ---- all levels at once: the stages above on slice 0 of a one-slice plan ----
// stage 1: x transform of the packed divergence + pack for the forward all-to-all
MHH_API int mhh_pres_fwd_x_pack(mhh_pres_slab_plan* P, const mhh_grid* g, void* p_packed, void* sendbuf, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(sendbuf != nullptr, "sendbuf");
    MHH_REQUIRE(P->nchunks == 1, ONE_SLICE);
    return stage_fwd_x(P, slice_of(P, 0), p_packed, sendbuf, as_stream(stream));
}
// stage 2: after the forward all-to-all: y transform, tridiagonal (pres_2) or 7-band (pres_4) solves, inverse y transform, pack for the way back
MHH_API int mhh_pres_fwd_y_solve_bwd_y(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, void* sendbuf, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(recvbuf && sendbuf, "buffers");
    MHH_REQUIRE(P->nchunks == 1, ONE_SLICE);
    hipStream_t st = as_stream(stream);
    if (int e = stage_fwd_y(P, slice_of(P, 0), recvbuf, st)) return e;
    if (int e = slab_column_solve(P, st)) return e;
    return stage_bwd_y(P, slice_of(P, 0), sendbuf, st);
}
// stage 3: after the backward all-to-all: inverse x transform, normalise, write p (interior rows, x halo, vertical ghost levels)
MHH_API int mhh_pres_bwd_x_unpack(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, const mhh_fields* f, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(recvbuf && f && f->p, "buffers");
    MHH_REQUIRE(P->nchunks == 1, ONE_SLICE);
    if (int e = stage_bwd_x(P, slice_of(P, 0), recvbuf, as_stream(stream))) return e;
    return stage_unpack(P, g, f, as_stream(stream));
}
// stage 3, fused form: inverse x transform, then unpack + Pres_2::output in one kernel for everything but vt on the southernmost
// row; the caller exchanges the one-row halo of p and finishes with mhh_pres_output_south_row.
MHH_API int mhh_pres_bwd_x_unpack_output(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, const mhh_fields* f, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "Pres_2::output only: a pres_4 plan takes mhh_pres_bwd_x_unpack, the halo of p and mhh_pres_output_order(g, 4)");
    MHH_REQUIRE(recvbuf && f && f->p && f->ut && f->vt && f->wt, "buffers");
    MHH_REQUIRE(P->nchunks == 1, ONE_SLICE);
    if (int e = stage_bwd_x(P, slice_of(P, 0), recvbuf, as_stream(stream))) return e;
    return stage_unpack_output(P, g, f, as_stream(stream));
}
MHH_API int mhh_pres_output_south_row(const mhh_grid* g, const mhh_fields* f, void* stream)
{
    if (int e = check_grid(g)) return e;
    MHH_REQUIRE(f && f->p && f->vt && g->jgc >= 1, "null field");
    dim3 grid((g->imax + 255)/256, g->kmax);
#define CALL(TF) [&]{ const GridDev<TF> gd = make_grid<TF>(g); \
        hipLaunchKernelGGL(pres_out_south_row_kernel<TF>, grid, dim3(256), 0, as_stream(stream), mp<TF>(f->vt), cp<TF>(f->p), gd.dyi_t, g->istart, g->iend, g->jstart, g->kstart, g->icells, g->ijcells); return (int)MHH_OK; }()
    if (int e = MHH_DISPATCH(g, CALL)) return e;
#undef CALL
    MHH_LAUNCH_CHECK();
    return MHH_OK;
}

// ---- the x stages with the transforms in LDS (pres_lds.h): input + x transform WRITING the send buffer of the x -> y transpose,
// x transform + p + output READING the receive buffer of the y -> x transpose -- two kernels and four array passes per rank where
// the staged form has input | x r2c | pack and unpack | x c2r | unpack + output (six kernels, eleven passes). The y stage between
// the transposes is unchanged. c = k-slice (0 with unsliced transposes): the kernels work the levels of that slice only.
MHH_API int mhh_pres_slab_has_lds(const mhh_pres_slab_plan* P)
{
    // MHH_PRES_SLAB_LDS=0: the staged x stages (A/B runs, tests of both forms)
    return (P && P->order == 2 && P->tx_lds && !env_is("MHH_PRES_SLAB_LDS", "0")) ? 1 : 0;
}
MHH_API int mhh_pres_slab_lds_fwd(mhh_pres_slab_plan* P, const mhh_grid* g, const mhh_fields* f, double dt, void* sendbuf, int c, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "the LDS x stages implement pres_2 only");
    MHH_REQUIRE(P->tx_lds != nullptr, "this plan has no LDS form of the x stages (power-of-two itot, jmax a multiple of 8)");
    MHH_REQUIRE(f && f->u && f->v && f->w && f->ut && f->vt && f->wt && f->rhoref && f->rhorefh && sendbuf, "null field");
    MHH_REQUIRE(dt > 0. && c >= 0 && c < P->nchunks, "dt, k-slice");
    const int ks = P->ktot / P->nchunks;
    return lds_slab_stage_in(g, f, dt, sendbuf, P->tx_lds, P->nxb, P->npy, ks, c*ks, (c+1)*ks, as_stream(stream));
}
MHH_API int mhh_pres_slab_lds_bwd(mhh_pres_slab_plan* P, const mhh_grid* g, const void* recvbuf, const mhh_fields* f, int c, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "the LDS x stages implement pres_2 only");
    MHH_REQUIRE(P->tx_lds != nullptr, "this plan has no LDS form of the x stages (power-of-two itot, jmax a multiple of 8)");
    MHH_REQUIRE(f && f->p && f->ut && f->vt && f->wt && recvbuf, "null field");
    MHH_REQUIRE(c >= 0 && c < P->nchunks, "k-slice");
    const int ks = P->ktot / P->nchunks;
    return lds_slab_stage_out(g, f, recvbuf, P->tx_lds, P->nxb, P->npy, ks, c*ks, (c+1)*ks, as_stream(stream));
}
// The y stage of the LDS form: the transform along y of k-slice c from the receive buffer into the plan's [k][kxl][ky] array
// (mhh_pres_slab_lds_fwd_y), the Thomas sweeps over all levels (mhh_pres_solve_y), the transform back into the send buffer
// (mhh_pres_slab_lds_bwd_y). The buffers of this form are laid out [slice][peer][k][kxl][row] (rows fastest), NOT as the staged form's.
MHH_API int mhh_pres_slab_lds_fwd_y(mhh_pres_slab_plan* P, const mhh_grid* g, void* recvbuf, int c, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "the LDS x stages implement pres_2 only");
    MHH_REQUIRE(P->ty_lds != nullptr && recvbuf && c >= 0 && c < P->nchunks, "LDS form, buffer, k-slice");
    const int ks = P->ktot / P->nchunks;
    return lds_slab_yfft(g, true, recvbuf, P->specy, P->ty_lds, P->nxb, P->npy, ks, c*ks, (c+1)*ks, as_stream(stream));
}
MHH_API int mhh_pres_slab_lds_bwd_y(mhh_pres_slab_plan* P, const mhh_grid* g, void* sendbuf, int c, void* stream)
{
    if (int e = slab_match(P, g)) return e;
    MHH_REQUIRE(P->order == 2, "the LDS x stages implement pres_2 only");
    MHH_REQUIRE(P->ty_lds != nullptr && sendbuf && c >= 0 && c < P->nchunks, "LDS form, buffer, k-slice");
    const int ks = P->ktot / P->nchunks;
    return lds_slab_yfft(g, false, sendbuf, P->specy, P->ty_lds, P->nxb, P->npy, ks, c*ks, (c+1)*ks, as_stream(stream));
}
