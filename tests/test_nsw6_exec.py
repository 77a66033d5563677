"""Microphys_nsw6::exec and its sedimentation CFL number (csrc/microphys_nsw6.h) against the reference.

The reference is the reference's own source behind tests/cpp/ref_nsw6_shim.cpp where that tree exists, tests/golden/nsw6_ref.npz
elsewhere (tests/nsw6_ref.py). With the shim built on this host the NSW6_POW form of the emulation build agrees bit for bit, through
pow, exp, log, sqrt and the host's tgamma: conversion alone, each species' sedimentation alone and everything together, from
non-zero tendencies, with ql and qi given and with both null, the three surface rates and the CFL number. NSW6_SQRT differs from
NSW6_POW by rounding alone: SQRT_BOUND is 8 times the difference measured on the emulation build, relative to each array's largest
value. On the MI355X both forms are held against the golden file: BOUND is 8 times the largest difference measured there
(profiles/microphys_nsw6.md). With ql and qi null the branches of conversion compare computed values with thresholds; cells whose
REFERENCE value lies within a relative 1e-12 (fp64) / 1e-5 (fp32) of one are left out; the recording step asserts that the seeded
inputs put none there, so the lists in the golden file are empty.
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import moist_ref as M
import nsw6_ref as R
from backends import be  # noqa: F401
from microhh_amd import capi

CASES = [(s, gc) for s in R.SHAPES for gc in R.GCS]
IDS = ["%dx%dx%d-gc%d%d%d" % (s + gc) for s, gc in CASES]
SHAPE_IDS = ["%dx%dx%d" % s for s in R.SHAPES]
# 8 x the largest difference of either form measured on the MI355X against the golden file, relative to the array's maximum
# (profiles/microphys_nsw6.md: 2.18e-15 in fp64 on qgt in the form NSW6_SQRT, 1.44e-15 in NSW6_POW; 5.37e-7 in fp32 on qst in both; the
# CFL number differs by 2.6e-7 in fp32)
BOUND = {np.float64: 8*2.18e-15, np.float32: 8*5.37e-7}
# 8 x the largest difference between the two forms measured on the emulation build (profiles/microphys_nsw6.md: 2.58e-15 in fp64,
# 2.74e-6 in fp32, both on qst; the CFL number differs by 1.1e-7 in fp32)
SQRT_BOUND = {np.float64: 8*2.58e-15, np.float32: 8*2.74e-6}
ALL_OUT = R.OUT + R.BOT


def interior2(g):
    return (slice(g.jstart, g.jend), slice(g.istart, g.iend))


def check_outside(x, out):
    """Nothing outside the interior is written, and no field anywhere: the sentinel of the horizontal ghost cells, the ghost levels,
    the rim of the surface rates."""
    g = x.g
    for n in R.SPECIES + ("thl", "qt", "ql", "qi"):
        assert cm.same_bits(out[n], x.h[n]), n
    mask = np.ones(g.shape3, dtype=bool); mask[g.interior] = False
    for n in R.OUT:
        assert cm.same_bits(out[n][mask], x.h[n][mask]), n
    rim = np.ones(g.shape2, dtype=bool); rim[interior2(g)] = False
    for n in R.BOT:
        assert cm.same_bits(out[n][rim], x.h[n][rim]), n


def test_golden_file_matches_the_cases():
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/nsw6_ref.npz"
    for shape in R.SHAPES:
        assert str(z["digest/%s" % R.ice_case(shape).key]) == R.ice_case(shape).digest(), "the seeded inputs differ from the recorded ones"
    for k in z.files:
        if k.endswith("excluded"):
            assert z[k].size == 0


def test_inputs_cover_the_branches():
    """On the inputs themselves (float64 transcription of the scheme in nsw6_ref.diagnose)."""
    both = lambda m: m.any() and (~m).any()
    c = R.ice_case((70, 9, 10))
    d = R.diagnose(c, c.dt["hi"])
    busy = d["busy"]
    assert both(d["T"] >= R.T0) and (d["T"] < 233.15).any()
    for name, m in d["has"].items():
        assert both(m[busy]) if name != "vapor" else both(m), name
    assert both(busy)                                                           # cells with nothing
    i = (slice(1, -1),)
    assert both(c.qr[i][d["has"]["rain"]] >= 1e-4) and both(c.qs[i][d["has"]["snow"]] >= 1e-4)
    assert both(d["S_i"][busy] <= 1.) and (d["has"]["rain"] & (d["S_w"] < 1.)).any()
    assert both(c.qs[i][d["has"]["snow"]] > 6e-4)
    for name, f in d["factor"].items():
        assert (f[busy] < 1.).any(), "limit factor of q%s" % name
    # liquid-only, mixed and ice-only cloud
    assert (d["has"]["liq"] & ~d["has"]["ice"]).any() and (d["has"]["liq"] & d["has"]["ice"]).any() and (~d["has"]["liq"] & d["has"]["ice"]).any()
    # the clamps of the terminal velocity: 10 m/s here, 0.1 m/s under the dense levels of (20, 1, 12)
    assert any((v > 10.).any() for v in d["V"].values())
    dense = R.diagnose(R.ice_case((20, 1, 12)), 1.)
    assert any(((v > 0) & (v < 0.1)).any() for v in dense["V"].values())
    for shape in R.SHAPES:
        c = R.ice_case(shape)
        for n in R.SPECIES:
            wet = getattr(c, n)[i] > 1e-12
            if shape == (70, 9, 10):
                assert (wet[-1] & ~wet[:-1].any(axis=0)).any() and (wet[0] & ~wet[1:].any(axis=0)).any(), n     # top only, bottom only
        assert R.ref("cfl/%dx%dx%d/hi/f64" % shape)[0] > 1.                                                    # a gather over several levels


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES, ids=IDS)
def test_exec_is_the_references(be, shape, gc, dtype):  # noqa: F811
    """Every part alone and all together, with ql and qi given and with both null. With the shim on this host: NSW6_POW from non-zero
    tendencies, both steps, bit for bit. Elsewhere both forms on the runs of the golden file (from zero tendencies) within BOUND."""
    g = R.grid_of(shape, gc, dtype)
    c = R.ice_case(shape)
    if R.exact_here(be):
        for mode in R.MODES:
            for name, mask in R.MASKS.items():
                for dtname in (R.CFLS if mask != R.CONV else ("hi",)):
                    x = R.Dev(be, shape, gc, dtype)
                    got = x.exec(mask, c.dt[dtname], mode, R.POW)
                    want = R.ref_exec(shape, dtype, mask, dtname, mode, gc=gc)
                    check_outside(x, got)
                    for n in ALL_OUT:
                        assert cm.same_bits(got[n], want[n]), (mode, name, dtname, n, M.rel(got[n], want[n]))
                        if n in R.WRITES[mask]:
                            assert not cm.same_bits(got[n], x.h[n]), (name, n, "the part wrote nothing")
                        else:
                            assert cm.same_bits(got[n], x.h[n]), (name, n, "not this part's to write")
                    assert x.count() == 0
        return
    for s, name, mask, dtname, mode in R.golden_runs():
        if s != shape:
            continue
        key = R.run_key(shape, name, dtname, mode, dtype)
        excluded = R.ref(key + "excluded", be) if mode == "sat" else np.zeros(0, dtype=np.int32)
        assert excluded.size == 0
        for impl in (R.POW, R.SQRT):
            x = R.Dev(be, shape, gc, dtype, zero_tend=True)
            got = x.exec(mask, c.dt[dtname], mode, impl)
            check_outside(x, got)
            for n in R.stored(shape, mask, mode):
                want = R.ref(key + n, be)
                have = R.pick(shape, got[n][interior2(g)] if n in R.BOT else got[n][g.interior])
                e = M.rel(have, want)
                print("nsw6 exec %s gc%d%d%d %s impl %d %s: rel %.3e" % (key, gc[0], gc[1], gc[2], be.name, impl, n, e))
                assert np.max(np.abs(want)) > 0, (name, n)
                assert e <= BOUND[dtype], (name, dtname, mode, impl, n, e)
            assert x.count() == 0


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_sqrt_form_is_the_pow_form_up_to_rounding(shape, dtype):
    """On the emulation build: everything at once in both modes, from non-zero tendencies, and the CFL number."""
    emul = B.get("emul")
    c = R.ice_case(shape)
    for mode in R.MODES:
        out = {}
        for impl in (None, R.POW, R.SQRT):
            x = R.Dev(emul, shape, (3, 3, 1), dtype, zero_tend=True)
            out[impl] = x.exec(R.ALL, c.dt["hi"], mode, impl)
            check_outside(x, out[impl])
        for n in ALL_OUT:
            assert cm.same_bits(out[None][n], out[capi_default()][n]), n
            i = interior2(x.g) if n in R.BOT else x.g.interior
            e = M.rel(out[R.SQRT][n][i], out[R.POW][n][i])
            print("nsw6 sqrt vs pow %s %s %s %s: rel %.3e" % (c.key, mode, R.tag(dtype), n, e))
            assert e <= SQRT_BOUND[dtype], (mode, n, e)
    x = R.Dev(emul, shape, (1, 1, 1), dtype)
    a, b = x.cfl(c.dt["hi"], R.POW), x.cfl(c.dt["hi"], R.SQRT)
    print("nsw6 sqrt vs pow %s cfl %s: rel %.3e" % (c.key, R.tag(dtype), abs(a - b)/a))
    assert abs(a - b) <= SQRT_BOUND[dtype]*a


def capi_default():
    """MHH_NSW6_IMPL_DEFAULT of include/mhh_hip.h."""
    return R.SQRT


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_sedimentation_conserves_and_idle_cells_keep_their_bits(be, shape, dtype):  # noqa: F811
    """Sedimentation alone from zero tendencies: the flux form telescopes and the flux at kend is zero, so per column and species
    sum_k rho dz qct == -r_bot within ktot x eps x the largest term, and the rates are non-negative. Conversion alone: a cell without
    condensate keeps the bits of its five tendencies."""
    c = R.ice_case(shape)
    x = R.Dev(be, shape, (3, 3, 1), dtype, zero_tend=True)
    got = x.exec(R.SEDI_R | R.SEDI_S | R.SEDI_G, c.dt["hi"], "given")
    g = x.g
    eps = np.finfo(dtype).eps
    rdz = (x.h["rho"].astype(np.float64)*g.dz.astype(np.float64))[g.kstart:g.kend, None, None]
    for s in range(3):
        rate = got[R.BOT[s]][interior2(g)].astype(np.float64)
        terms = rdz*got[R.OUT[s]][g.interior].astype(np.float64)
        assert (rate >= 0).all() and rate.max() > 0
        bound = g.kmax*eps*np.maximum(np.abs(terms).max(axis=0), np.abs(rate))
        assert (np.abs(terms.sum(axis=0) + rate) <= bound).all(), R.SPECIES[s]
    y = R.Dev(be, shape, (3, 3, 1), dtype)
    got = y.exec(R.CONV, c.dt["hi"], "given")
    i = g.interior
    idle = ~((y.h["ql"][i] > 1e-7) | (y.h["qi"][i] > 1e-7) | (y.h["qr"][i] > 1e-12) | (y.h["qs"][i] > 1e-12) | (y.h["qg"][i] > 1e-12))
    assert 0.02 < idle.mean() < 0.9
    for n in R.OUT:
        assert cm.same_bits(got[n][i][idle], y.h[n][i][idle]), n
        assert (got[n][i][~idle] != y.h[n][i][~idle]).mean() > 0.2, n


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES, ids=IDS)
def test_sedimentation_cfl(be, shape, gc, dtype):  # noqa: F811
    """The largest of the three calc_cfl_ss08 for both steps and both forms, and its floor of 1e-5 on fields without precipitation."""
    c = R.ice_case(shape)
    x = R.Dev(be, shape, gc, dtype)
    for dtname in R.CFLS:
        want = float(R.ref("cfl/%dx%dx%d/%s/%s" % (shape + (dtname, R.tag(dtype))), be)[0])
        for impl in (R.POW, R.SQRT):
            got = x.cfl(c.dt[dtname], impl)
            print("nsw6 cfl %s %s %s impl %d: got %.17g want %.17g rel %.3e" % (c.key, dtname, be.name, impl, got, want, abs(got - want)/want))
            if R.exact_here(be) and impl == R.POW:
                assert got == want
            else:
                assert abs(got - want) <= max(BOUND[dtype], SQRT_BOUND[dtype])*want
        assert x.cfl(c.dt[dtname]) == x.cfl(c.dt[dtname], capi_default())
        assert 0.5*R.CFLS[dtname] < want < 2.*R.CFLS[dtname]
    h = c.inputs(x.g)
    for n in R.SPECIES:
        h[n][:] = 0
    dry = R.Dev(be, shape, gc, dtype, host=h)
    assert dry.cfl(1.0) == 1e-5


def test_refusals_name_their_reason(be):  # noqa: F811
    x = R.Dev(be, (20, 1, 12), (1, 1, 1), np.float64)
    a = x.args("given")
    p = capi.MhhMicroParams(R.NC0, 10., R.ALL)
    lib = be.lib
    assert lib.mhh_micro_nsw6_exec_impl(x.G, 7, C.byref(p), *a) != 0 and b"impl" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(p), None, *a[1:]) != 0 and b"null field" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(p), *a[:3], None, *a[4:]) != 0 and b"conversion needs" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(p), *a[:5], None, *a[6:]) != 0 and b"both given or both null" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(p), *a[:18], None, None, be.stream) != 0 and b"scratch" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(capi.MhhMicroParams(R.NC0, 10., 16)), *a) != 0 and b"processes" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(capi.MhhMicroParams(R.NC0, 0., R.ALL)), *a) != 0 and b"dt" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_exec(x.G, C.byref(capi.MhhMicroParams(0., 10., R.ALL)), *a) != 0 and b"Nc0" in lib.mhh_last_error()
    assert lib.mhh_micro_nsw6_cfl(x.G, *a[:3], a[15], 1., None, None, be.stream) != 0 and b"work" in lib.mhh_last_error()
    g0 = R.grid_of((20, 1, 12), (1, 1, 1), np.float64)
    G0 = be.grid(g0)
    G0.contents.dtype = 5
    assert lib.mhh_micro_nsw6_exec(G0, C.byref(p), *a) != 0 and b"dtype" in lib.mhh_last_error()
    # conversion alone: no scratch and no surface rates needed
    p = capi.MhhMicroParams(R.NC0, 10., R.CONV)
    B.ok(be, lib.mhh_micro_nsw6_exec(x.G, C.byref(p), *a[:12], None, None, None, *a[15:18], None, None, be.stream))
    be.sync()
