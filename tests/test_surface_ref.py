"""The surface layer (csrc/surface_layer.h) against the reference's own templates.

Reference: tests/cpp/ref_surface_shim.cpp compiled against the reference's headers where that tree exists, otherwise
tests/golden/surface_ref.npz (tests/surface_ref.py). Record the golden file with
    MHH_RECORD_SURFACE_GOLDEN=1 python -m pytest tests/test_surface_ref.py
GPU tests read only the golden file.

Exact (bit for bit, both backends): nobuk and obuk from a given dutot -- products, quotients and the float interpolation only --,
ugradbot, vgradbot, and sgradbot of a Dirichlet scalar. sgradbot of a FLUX scalar is (var - varbot)/zsl with varbot from fh, so it
is exact only where fh is: it is compared with the toleranced outputs.
Toleranced: everything that passes through pow / log / exp. On emul with the shim compiled on the same host these are bit for bit
too (same C library, no contraction); elsewhere max|got - ref| / max|ref| per array stays under BOUND.
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import surface_ref as S
from backends import be  # noqa: F401
from common import same_bits as same
from microhh_amd import capi

# Largest relative difference per dtype over every case and every output that passes through pow / log / exp (dutot, ustar, ufluxbot,
# vfluxbot, sfluxbot / sbot, dudz, dvdz, dbdz) on the first MI355X run, profiles/surface_parity.md, times 8 (three bits: the device
# library's pow / log / exp errors depend on the argument and the seeds sample few).
# fp64: 5.804e-16 (dbdz, flux 16x6x8) -> 4.64e-15;  fp32: 5.149e-7 (dbdz, dirichlet 20x1x12) -> 4.12e-6.
BOUND = {np.dtype(np.float64): 8*5.804e-16, np.dtype(np.float32): 8*5.149e-7}
CEILING = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}     # beyond this a difference is not rounding

RECORD = S.RECORD
CASES = [pytest.param(c, s, id=i) for (c, s), i in zip(S.CASES, S.CASE_IDS)]
_ref, _dev = {}, {}


def table_of(case, want_shim):
    if want_shim:
        return S.lut(S.shim().ref_surface_lut, case.g, case.mbcbot, case.thermobc)
    return None


def reference(case, use_shim):
    """(inputs, outputs) of the reference for a case, computed once: the shim where asked for (and possible), else the golden file."""
    key = (case.id, use_shim)
    if key not in _ref:
        if use_shim:
            inp = case.inputs()
            _ref[key] = (inp, S.ref_exec(case, inp, case.state(), table_of(case, True)))
        else:
            _ref[key] = S.golden_case(case)
    return _ref[key]


def device(be, case, inp, ref):  # noqa: F811
    """The three device runs of a case on a backend, once: staged from the reference's dutot, staged, fused."""
    key = (be.name, case.id)
    if key not in _dev:
        runs = {}
        for mode in ("given", "staged", "fused"):
            st = case.state()
            d = S.DevSurf(be, case, inp, st)
            if mode == "given":
                d.a["dutot"] = be.arr(ref["dutot"]); d.staged(dutot_given=True)
            elif mode == "staged":
                d.staged()
            else:
                d.fused()
            runs[mode] = d.outputs()
        _dev[key] = runs
    return _dev[key]


def exact_reference_here(be):  # noqa: F811
    """emul with the shim compiled on this host: same C library, no contraction -- every output bit for bit."""
    return be.name == "emul" and S.have_reference() and not RECORD


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_shim_compiles_and_golden_is_current(tmp_path):
    """not gpu: compiles the shim against the reference's headers; records the golden file (MHH_RECORD_SURFACE_GOLDEN=1) or checks
    that it still holds what the shim gives. Every recorded case must keep |zsl/L| <= 8 on every cell."""
    if not S.have_reference():
        pytest.skip("the reference tree is absent: the other tests read tests/golden/surface_ref.npz")
    assert S.shim() is not None
    rec = {}
    for config, shape in S.CASES:
        for dt in cm.DTYPES:
            case = S.SurfCase(config, shape, dt)
            inp, out = reference(case, True)
            zsl = S.zsl_of(case.g)
            if case.kind != S.NONE:
                assert np.max(np.abs(zsl / out["obuk"].astype(np.float64))) <= S.ZL_LIMIT, (case.id, np.max(np.abs(zsl / out["obuk"])))
            if case.mbcbot == S.DIRICHLET:
                core = out["dutot"][case.g.jstart:case.g.jend, case.g.istart:case.g.iend]
                assert core.min() >= 0.5 and core.max() <= 3., (case.id, core.min(), core.max())
            mid = case.id.rsplit("-", 1)[0]
            for k, v in case.master.items():
                rec["%s/in/%s" % (mid, k)] = v
            for k in case.out_names():
                rec["%s/out/%s" % (case.id, k)] = out[k]
    for form in ("flux", "dirichlet"):
        for dt in cm.DTYPES:
            case = S.SurfCase(form, S.SMALL, dt)
            rec["lut/%s" % case.id] = np.array(S.digest(*table_of(case, True)))
    rec.update(state_reference(True))
    if RECORD:
        S.GOLD.save(rec)
    z = S.golden()
    assert z is not None, "record tests/golden/surface_ref.npz first (MHH_RECORD_SURFACE_GOLDEN=1)"
    assert sorted(z.files) == sorted(rec)
    for k, v in rec.items():
        assert (str(z[k]) == str(v)) if v.dtype.kind == "U" else same(z[k], v), k


# ---- the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["flux", "dirichlet"])
@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_lut_is_prepare_lut(be, form, dtype):  # noqa: F811
    case = S.SurfCase(form, S.SMALL, dtype)
    got = S.lut(be.lib.mhh_surface_lut_host, case.g, case.mbcbot, case.thermobc)
    if be.name == "emul" and S.have_reference():
        want = table_of(case, True)
        assert same(got[0], want[0]) and same(got[1], want[1])
    assert S.digest(*got) == str(S.golden()["lut/%s" % case.id])
    assert abs(got[0][0] + 1e4) < 1. and got[0][-1] == np.float32(10.)     # the stretched end is a geometric sum, the top end exact
    if form == "flux":                      # not monotone on the stable side: it rises up to n ~ 4293 and then falls
        assert got[1][-1] < 1e-4 < got[1].max() and 4200 < int(np.argmax(got[1])) < 4400


# ---- the stages against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,shape", CASES)
@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_surface_layer_against_reference(be, config, shape, dtype):  # noqa: F811
    case = S.SurfCase(config, shape, dtype)
    bitwise = exact_reference_here(be)
    inp, ref = reference(case, bitwise)
    runs = device(be, case, inp, ref)
    names = case.out_names()
    flux_grads = ["sgradbot%d" % n for n, bc in enumerate(case.sbc) if bc == S.FLUX]
    # 1. exact from a given dutot
    given = runs["given"]
    for k in S.EXACT:
        if k in names and k not in flux_grads:
            assert same(given[k], ref[k]), (k, cm.ulp_diff(given[k].astype(np.float64), ref[k].astype(np.float64)))
    # 3. everything through pow / log / exp
    worst = {}
    for mode in ("given", "staged"):
        got = runs[mode]
        for k in names:
            if k == "nobuk" and not bitwise:
                # staged: dutot is the device's, so a column on an edge of a table interval may land one entry away
                assert same(got[k], ref[k]) if mode == "given" else int(np.abs(got[k].astype(np.int64) - ref[k]).max()) <= 1, k
                continue
            if bitwise:
                assert same(got[k], ref[k]), (mode, k, cm.ulp_diff(got[k], ref[k]))
            else:
                worst[k] = max(worst.get(k, 0.), S.rel(got[k], ref[k]))
    for k, r in sorted(worst.items()):
        print("surface_parity %s %s %s %.3e" % (be.name, case.id, k, r))
    for k, r in worst.items():
        # sgradbot of a FLUX scalar, (var - varbot)/zsl: varbot carries BOUND relative to ~300 K and the difference is a few K, so the
        # same absolute error is max|varbot| / max|var - varbot| times larger relative to the gradient (profiles/surface_parity.md)
        amp = float(np.max(np.abs(ref["sbot" + k[-1]])) / (S.zsl_of(case.g)*np.max(np.abs(ref[k])))) if k in flux_grads else 1.
        assert r <= CEILING[case.dtype], ("not rounding: find the cause", k, r)
        assert r <= BOUND[case.dtype]*amp, (k, r, amp)
    # 4. fused = staged, ghost cells included
    for k in names:
        assert same(runs["fused"][k], runs["staged"][k]), ("fused != staged", k)


# ---- the state in nobuk ----------------------------------------------------------------------------------------------------
STATE_SHAPE = (17, 9, 8, (3, 3, 1))
DU = 3.


def state_inputs(g):
    """Buoyancy fluxes of three calls at du = 3, zsl = 5 (Ri = -kappa*bflux*zsl/du^3): call 1 puts Ri = 1e-3 above the table's maximum
    (~1.36e-4) -> n = 9999; call 2 has Ri = 1e-4, below the maximum but above f[9999] -> the walk stays at 9999 (a walk from 0 would
    stop on the rising branch near 4200); call 3 is unstable beyond the table on every third column (Ri = -1e7 < f[0]) -> the walk
    runs down to the guard at n = 0 -- and mildly unstable elsewhere."""
    rs = np.random.RandomState(5)
    b = lambda ri: -ri*DU**3/(0.4*5.)                                                                 # noqa: E731
    col = np.arange(g.ijcells).reshape(g.shape2)
    third = np.where(col % 3 == 0, b(-1e7), b(-0.05 - 0.1*rs.random_sample(g.shape2)))
    return [np.full(g.shape2, b(1e-3)), np.full(g.shape2, b(1e-4)), third]


def state_case(dtype):
    case = S.SurfCase("flux", STATE_SHAPE, dtype)
    case.kind = S.BUOY                                   # the buoyancy flux is the scalar's flux: Ri is what state_inputs says
    return case


def state_reference(use_shim):
    """{key: array}: nobuk and obuk after each of the three calls, both dtypes."""
    out = {}
    for dt in cm.DTYPES:
        case = state_case(dt)
        tag = "state/%s" % ("f64" if case.dtype == np.float64 else "f32")
        if not use_shim:
            for c in range(3):
                for k in ("nobuk", "obuk"):
                    out["%s/%d/%s" % (tag, c, k)] = S.golden()["%s/%d/%s" % (tag, c, k)]
            continue
        inp, st = case.inputs(), case.state()
        for c, flux in enumerate(state_inputs(case.g)):
            inp["sfluxbot0"] = flux.astype(case.dtype)
            r = S.ref_exec(case, inp, st, table_of(case, True), dutot=np.full(case.g.shape2, DU))
            out["%s/%d/nobuk" % (tag, c)] = r["nobuk"].copy(); out["%s/%d/obuk" % (tag, c)] = r["obuk"].copy()
    return out


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_nobuk_is_state_carried_from_call_to_call(be, dtype):  # noqa: F811
    case = state_case(dtype)
    tag = "state/%s" % ("f64" if case.dtype == np.float64 else "f32")
    ref = state_reference(exact_reference_here(be))
    d = S.DevSurf(be, case, case.inputs(), case.state())
    d.a["dutot"] = be.arr(np.full(case.g.shape2, DU, dtype=case.dtype))
    for c, flux in enumerate(state_inputs(case.g)):
        d.a["sfluxbot0"] = be.arr(flux.astype(case.dtype)); d.f.s_fluxbot[0] = be.ptr(d.a["sfluxbot0"]).value
        d.call("mhh_surface_stability", be.ptr(d.a["dutot"]))
        be.sync()
        n, L = be.host(d.a["nobuk"]), be.host(d.a["obuk"])
        assert same(n, ref["%s/%d/nobuk" % (tag, c)]) and same(L, ref["%s/%d/obuk" % (tag, c)]), c
        if c < 2:
            assert (n == S.NZL - 1).all() and (L == case.dtype.type(5.)/case.dtype.type(10.)).all()      # zL = 10 at the table's end
        else:
            assert (n.ravel()[::3] == 0).all() and (n.ravel()[1::3] > 0).all()
    # the second call started from 0 instead lands on the rising branch: the result depends on the state
    d2 = S.DevSurf(be, case, case.inputs(), case.state())
    d2.a["dutot"] = d.a["dutot"]
    d2.a["sfluxbot0"] = be.arr(state_inputs(case.g)[1].astype(case.dtype)); d2.f.s_fluxbot[0] = be.ptr(d2.a["sfluxbot0"]).value
    d2.call("mhh_surface_stability", be.ptr(d2.a["dutot"]))
    be.sync()
    n0 = be.host(d2.a["nobuk"])
    assert (n0 > 3000).all() and (n0 < 6000).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(be):  # noqa: F811
    case = S.SurfCase("flux", S.SMALL, np.float64)
    d = S.DevSurf(be, case, case.inputs(), case.state())
    calls = [("mhh_boundary_surface_exec", (be.ptr(d.a["dutot"]),)), ("mhh_surface_dutot", (be.ptr(d.a["dutot"]),)),
             ("mhh_surface_stability", (be.ptr(d.a["dutot"]),)), ("mhh_surface_momentum", ()), ("mhh_surface_scalar", (0,)),
             ("mhh_surface_mo_gradients", ())]
    before = d.outputs()
    for member, value, word in (("swconstantz0", 0, "swconstantz0"), ("swcharnock", 1, "swcharnock")):
        keep = getattr(d.p, member); setattr(d.p, member, value)
        for name, args in calls:
            with pytest.raises(capi.MhhError, match=word):
                d.call(name, *args)
        setattr(d.p, member, keep)
    thin = S.grid_of((20, 4, 12, (1, 3, 1)), np.float64)
    G = be.grid(thin)
    for name, args in calls:
        rc = getattr(be.lib, name)(G, C.byref(d.f), C.byref(d.p), *args, be.stream)
        assert rc == 1 and b"igc >= 2" in be.lib.mhh_last_error()
    after = d.outputs()
    assert all(same(before[k], after[k]) for k in before), "a refused call wrote something"
