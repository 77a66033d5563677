"""Saturation adjustment per cell (cell_ops.h moist_*, mhh_thermo_moist_sat_adjust) against the reference's own header.

Reference: tests/cpp/ref_moist_shim.cpp compiled against the reference's headers where that tree exists, otherwise
tests/golden/moist_ref.npz (tests/moist_ref.py). Record the golden file with
    MHH_RECORD_MOIST_GOLDEN=1 python -m pytest tests/test_moist_cell.py
GPU tests read only the golden file.

Warm set (thl*exn >= T0 + 0.5, asserted): + - * /, max and fabs only, so ql, qi, t, qs agree bit for bit on both backends.
Mixed set (p in [55000, 102000], thl in [235, 320], qt in [0, 0.025]): most saturated cells take the cold branch, which passes
through exp (esat_ice). On emul with the shim built on the same host: bit for bit. Elsewhere: toleranced, relative to the array's
maximum; the bound is 8 times the largest difference measured (profiles/thermo_moist.md), under an independent ceiling: sat_adjust
stops at |dT|/T <= 1e-5, so a device that stops one iteration away from the reference may differ in t by that much and no more.
"""
import numpy as np
import pytest

import common as cm
import moist_ref as M
import refshim
from backends import be  # noqa: F401

# measured on the MI355X against the golden file (the largest of ql, qi, t, qs; relative to the array's maximum), times 8
# (profiles/thermo_moist.md): fp64 4.516e-17 (ql) -> 3.61e-16;  fp32 4.849e-8 (ql) -> 3.88e-7. t itself had the reference's bits in
# both dtypes: no cell of the set stopped an iteration away from the reference.
MEASURED = {np.dtype(np.float64): 4.516e-17, np.dtype(np.float32): 4.849e-8}
BOUND = {k: 8*v for k, v in MEASURED.items()}
CEILING_T = 1e-5          # the stopping rule of sat_adjust: a larger difference in t is a defect, not rounding
OUT = ("ql", "qi", "t", "qs")


def test_shim_compiles_and_golden_is_current():
    """not gpu: compiles the shim against the reference's headers; records the golden file (MHH_RECORD_MOIST_GOLDEN=1) or checks that
    it still holds what the shim gives."""
    if not M.have_reference():
        pytest.skip("the reference tree is absent: the other tests read tests/golden/moist_ref.npz")
    rec = M.computed()
    if M.RECORD:
        M.GOLD.save(rec)
    z = M.golden()
    assert z is not None, "record tests/golden/moist_ref.npz first (MHH_RECORD_MOIST_GOLDEN=1)"
    assert sorted(z.files) == sorted(rec)
    for k, v in rec.items():
        assert (str(z[k]) == str(v)) if v.dtype.kind == "U" else cm.same_bits(z[k], v), k


def test_inputs_are_the_recorded_ones():
    """The inputs are regenerated from their seeds on every host: their digests are the ones the golden file was recorded with."""
    for name in ("warm", "mixed"):
        assert refshim.digest(*[M.point_set(name)[k] for k in ("thl", "qt", "p", "exn")]) == str(M.golden()["digest/point/%s" % name]), name
    for shape in M.SHAPES:
        c = M.field_case(shape)
        assert c.digest() == str(M.golden()["digest/field/%s" % c.key]), c.key


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_warm_set_is_bit_exact(be, dtype):  # noqa: F811
    m = M.point_set("warm")
    inp = M.typed(m, dtype)
    assert (inp["thl"]*inp["exn"] >= dtype(M.T0 + 0.5)).all()
    got, n = M.dev_sat_adjust(be, dtype, m)
    sat = 0
    for k in OUT:
        want = M.ref("point/warm/%s/%s" % (M.tag(dtype), k), be)
        assert cm.same_bits(got[k], want), (k, M.rel(got[k], want))
    sat = np.count_nonzero(got["ql"])
    assert n == 0 and (got["qi"] == 0).all()
    assert 0.2*M.NPOINT < sat < 0.9*M.NPOINT, sat            # both the early return and the Newton loop are exercised


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_mixed_set(be, dtype):  # noqa: F811
    m = M.point_set("mixed")
    got, n = M.dev_sat_adjust(be, dtype, m)
    t = M.tag(dtype)
    want = {k: M.ref("point/mixed/%s/%s" % (t, k), be) for k in OUT}
    cold = np.count_nonzero(want["qi"])
    assert n == 0
    assert 0.55*M.NPOINT <= np.count_nonzero(want["ql"] + want["qi"]) <= 0.9*M.NPOINT and cold > 0.3*M.NPOINT
    worst = {k: M.rel(got[k], want[k]) for k in OUT}
    dt_rel = float(np.max(np.abs(got["t"].astype(np.float64) - want["t"])/want["t"]))
    print("mixed set %s on %s: rel. differences %s, max |dt|/t %.3e" % (t, be.name, worst, dt_rel))
    if M.exact_here(be):
        for k in OUT:
            assert cm.same_bits(got[k], want[k]), (k, worst[k])
        return
    assert dt_rel <= CEILING_T, dt_rel
    for k in OUT:
        assert worst[k] <= BOUND[np.dtype(dtype)], (k, worst[k])


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_non_convergence_is_counted_not_fatal(be, dtype):  # noqa: F811
    """Inputs on which the reference throws (the even entries), each followed by a converging one: the call succeeds, the counter
    holds their number, the neighbours have the reference's values, and with no counter the call still succeeds."""
    t = M.tag(dtype)
    m = {k: M.golden()["nonconv/%s/in/%s" % (t, k)] for k in ("thl", "qt", "p", "exn")}
    nbad = m["thl"].size // 2
    assert nbad >= 3
    got, n = M.dev_sat_adjust(be, dtype, m)
    assert n == nbad
    alone, n_alone = M.dev_sat_adjust(be, dtype, {k: v[1::2].copy() for k, v in m.items()})     # the neighbours without the bad cells
    assert n_alone == 0
    for k in OUT:
        assert np.isfinite(got[k]).all()
        assert cm.same_bits(np.ascontiguousarray(got[k][1::2]), alone[k]), k                      # unaffected: the same bits
        want = M.golden()["nonconv/%s/%s" % (t, k)][1::2]
        if np.max(np.abs(want)) > 0:
            assert M.rel(got[k][1::2], want) <= BOUND[np.dtype(dtype)], k
        else:
            assert (got[k][1::2] == 0).all()
    from microhh_amd import capi
    inp = M.typed(m, dtype)
    d = {k: be.arr(v) for k, v in inp.items()}
    ql = be.zeros(m["thl"].size, dtype)
    capi.check(be.lib.mhh_thermo_moist_sat_adjust(M.code(dtype), m["thl"].size, *[be.ptr(d[k]) for k in ("thl", "qt", "p", "exn")],
                                                  be.ptr(ql), None, None, None, None, be.stream), be.lib)
    be.sync()
    assert cm.same_bits(be.host(ql), got["ql"])
