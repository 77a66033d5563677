/* TEST-ONLY: lets tests/test_integration_compile.py and tests/cpp/ref_pres_shim.cpp parse the reference headers that include
 * <fftw3.h> (include/fft.h:26). It declares the plan types those headers name and nothing else: no function, no transform.
 * The shim, which runs the reference's pressure solver, supplies FFT::exec_forward / exec_backward itself (the oracle's DFT);
 * src/fft.cxx is never built. */
#ifndef MHH_TEST_FFTW3_SYNTAX_STUB
#define MHH_TEST_FFTW3_SYNTAX_STUB
typedef struct mhh_stub_fftw_plan_s*  fftw_plan;
typedef struct mhh_stub_fftwf_plan_s* fftwf_plan;
#endif
