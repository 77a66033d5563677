// tests/cpp/ref_shim.h -- TEST infrastructure: what the ref_*_shim.cpp translation units share. tests/refshim.py compiles them with
// -fvisibility=hidden, so every entry point is marked REF_API.
#ifndef MHH_TESTS_REF_SHIM_H
#define MHH_TESTS_REF_SHIM_H

// the index ranges and strides of a grid, as the reference's kernels take them; mirrored by refshim.Dims
struct Dims { int istart, iend, jstart, jend, kstart, kend, icells, ijcells, kcells; };

#define REF_API extern "C" __attribute__((visibility("default")))

#endif
