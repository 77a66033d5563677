// pres_lds_slab.h -- what the pressure solvers of k_pres.hip (single GPU) and k_slab.hip (slab-decomposed) share: the complex
// number type of their spectral arrays, the rocFFT error check, the host-to-device table upload, and the x / y stages of
// Pres_2::exec with the transforms in LDS (pres_lds.h) for a slab rank, defined in k_pres.hip (where the kernels are
// instantiated). Internal to the library.
#pragma once
#include <vector>
#include <rocfft/rocfft.h>
#include "k_common.h"

// naturally aligned (16 bytes in fp64): one ds_read_b128 / global_load_dwordx4 per number instead of two 8-byte halves
template<class TF> struct alignas(2*sizeof(TF)) C2 { TF x, y; };

#define MHH_FFT_TRY(expr) do { rocfft_status s_ = (expr); if (s_ != rocfft_status_success) { \
    mhh::set_error("FFT error: %s returned %d (%s:%d)", #expr, (int)s_, __FILE__, __LINE__); return MHH_EFFT; } } while (0)

namespace mhh
{
// a host table into a new device allocation (the caller frees it)
template<class TF>
inline int upload(void** dst, const std::vector<TF>& v)
{
    MHH_HIP_TRY(hipMalloc(dst, v.size()*sizeof(TF)));
    MHH_HIP_TRY(hipMemcpy(*dst, v.data(), v.size()*sizeof(TF), hipMemcpyHostToDevice));
    return MHH_OK;
}
// exp(-2 pi i m / n), m < n, in the grid's precision on the device (the caller frees it): the twiddles of the LDS transforms
int lds_twiddles(int n, int dtype, void** t);
// 1 if a rank of this grid can run the x and y stages in LDS: power-of-two itot and jtot with instantiations, rows in whole strips of eight
int lds_slab_usable(const mhh_grid* g);
int lds_slab_yfft(const mhh_grid* g, bool fwd, void* xbuf, void* specy, const void* ty, int nxb, int npy, int ks, int kbeg, int kend, hipStream_t st);
int lds_slab_stage_in(const mhh_grid* g, const mhh_fields* f, double dt, void* xbuf, const void* tx, int nxb, int npy, int ks, int kbeg, int kend, hipStream_t st);
int lds_slab_stage_out(const mhh_grid* g, const mhh_fields* f, const void* xbuf, const void* tx, int nxb, int npy, int ks, int kbeg, int kend, hipStream_t st);
}
