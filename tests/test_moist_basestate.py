"""Thermo_moist's hydrostatic base state: mhh_thermo_moist_base_state_host and the device recurrence mhh_thermo_moist_base_state.

Reference: calc_top_and_bot + calc_base_state of the reference (tests/moist_ref.py: the shim where the reference tree exists, the
golden file elsewhere). Every level passes through pow (exner) and exp twice, so only the host entry on the host whose C library
the shim uses is bit for bit; everything else is toleranced, relative to the profile's maximum:

* device kernel against the host entry: 8 times the largest difference measured on the MI355X (profiles/thermo_moist.md).
* host entry against the golden file, recorded with another host's C library: the same bound. On the recording host and on the GPU
  box that difference is 0 (the same C library), and 8 times 0 is no tolerance; the device's math library is the second
  implementation of pow and exp at hand, so the difference measured between it and the host's on the same recurrence is the
  measured spread between two libraries that the bound is 8 times of.
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import moist_ref as M
from backends import be  # noqa: F401
from microhh_amd import thermo

# measured, relative to each profile's maximum, the worst of the eight profiles and the three cases:
#   device kernel against the host entry on the MI355X: fp64 1.907e-16 (bomex64, stretched) -> 1.53e-15; fp32 5.109e-7 (saturated) -> 4.09e-6
#   host entry against the golden file on the recording host and on the GPU box: 0 in both dtypes (the same C library)
MEASURED_DEV = {np.dtype(np.float64): 1.907e-16, np.dtype(np.float32): 5.109e-7}


def bound_dev(g):
    return 8*MEASURED_DEV[g.np_dtype]


def bound_host(g):
    return 8*MEASURED_DEV[g.np_dtype]


def inputs(name, dtype, be):  # noqa: F811
    """(grid, thl0, qt0 with zeroed ghost entries) of a case; the interior is the recorded one."""
    g, thl0, qt0 = M.base_case(name, dtype)
    key = "base/%s/%s/" % (name, M.tag(dtype))
    for a, n in ((thl0, "thl0"), (qt0, "qt0")):
        a[g.kstart:g.kend] = M.ref(key + n, be)[g.kstart:g.kend]
    return g, thl0, qt0, key


def host_entry(be, g, thl0, qt0, boussinesq=0, thvref0=0., skip=()):  # noqa: F811
    out = {n: np.full(g.kcells, -7., dtype=g.np_dtype) for n in M.BASE_OUT}
    thl0, qt0 = thl0.copy(), qt0.copy()
    n = C.c_int(0)
    B.ok(be, be.lib.mhh_thermo_moist_base_state_host(g.host_struct(), cm.ptr(thl0), cm.ptr(qt0), M.PBOT, boussinesq, thvref0,
                                                     *[cm.ptr(None if k in skip else out[k]) for k in M.BASE_OUT], C.byref(n)))
    assert n.value == 0
    return out, thl0, qt0


# the levels calc_base_state writes (thermo_moist_functions.h:306-348); the others keep what the caller put there
def written(g, n):
    ks, ke = g.kstart, g.kend
    return {"pref": slice(ks-1, ke+1), "prefh": slice(ks, ke+1), "exnrefh": slice(ks, ke+1), "thvrefh": slice(ks, ke+1), "rhorefh": slice(ks, ke+1),
            "exnref": slice(ks, ke), "thvref": slice(ks, ke), "rhoref": slice(ks, ke)}[n]


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("name", M.BASE_CASES)
def test_host_entry_is_create_basestate(be, name, dtype):  # noqa: F811
    g, thl0, qt0, key = inputs(name, dtype, be)
    got, thl_g, qt_g = host_entry(be, g, thl0, qt0)
    assert cm.same_bits(thl_g, M.ref(key + "thl0", be)) and cm.same_bits(qt_g, M.ref(key + "qt0", be))     # calc_top_and_bot: + - * / only
    worst = 0.
    for n in M.BASE_OUT:
        want, w = M.ref(key + n, be), written(g, n)
        keep = np.ones(g.kcells, dtype=bool); keep[w] = False
        assert (got[n][keep] == -7.).all(), n
        worst = max(worst, M.rel(got[n][w], want[w]))
        if M.exact_here(be):
            assert cm.same_bits(got[n][w], want[w]), (n, M.rel(got[n][w], want[w]))
    print("base state %s %s, host entry of %s against the reference: %.3e (bound %.3e)" % (name, M.tag(dtype), be.name, worst, bound_host(g)))
    assert worst <= bound_host(g)
    if name == "saturated":          # sat_adjust inside the recurrence: thvref differs from the unsaturated expression in the layer
        k = slice(g.kstart, g.kend)
        dry = thl_g[k].astype(np.float64)*(1. - (1. - 461.5/287.04)*qt_g[k].astype(np.float64))
        assert np.count_nonzero(np.abs(got["thvref"][k] - dry) > 1e-3*dry) >= 5
    else:
        assert name != "bomex64" or M.rel(got["thvref"][g.kstart:g.kend], thl_g[g.kstart:g.kend]*(1. - (1. - 461.5/287.04)*qt_g[g.kstart:g.kend])) < 1e-5


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_boussinesq_switch_overwrites_density_and_thvref(be, dtype):  # noqa: F811
    g, thl0, qt0, key = inputs("bomex64", dtype, be)
    ane, _, _ = host_entry(be, g, thl0, qt0)
    bou, _, _ = host_entry(be, g, thl0, qt0, boussinesq=1, thvref0=300.5)
    for n in ("rhoref", "rhorefh"):
        assert (bou[n] == 1.).all()
    for n in ("thvref", "thvrefh"):
        assert (bou[n] == dtype(300.5)).all()
    for n in ("pref", "prefh", "exnref", "exnrefh"):
        assert cm.same_bits(bou[n], ane[n])
    prof = thermo.base_state(be.lib, g, thl0[g.kstart:g.kend], qt0[g.kstart:g.kend], M.PBOT)
    for n in M.BASE_OUT:
        w = written(g, n)
        assert cm.same_bits(prof[n][w], ane[n][w]), n
    with pytest.raises(ValueError, match="thvref0"):
        thermo.base_state(be.lib, g, thl0[g.kstart:g.kend], qt0[g.kstart:g.kend], M.PBOT, swbasestate="boussinesq")


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("name", M.BASE_CASES)
def test_device_recurrence_against_the_host_entry(be, name, dtype):  # noqa: F811
    g, thl0, qt0, key = inputs(name, dtype, be)
    want, thl_g, qt_g = host_entry(be, g, thl0, qt0)
    G = be.grid(g)
    dthl, dqt = be.arr(thl_g), be.arr(qt_g)
    out = {n: be.arr(np.full(g.kcells, -7., dtype=dtype)) for n in M.BASE_OUT}
    keep, cptr, count = M.counter(be)
    B.ok(be, be.lib.mhh_thermo_moist_base_state(G, be.ptr(dthl), be.ptr(dqt), M.PBOT, *[be.ptr(out[n]) for n in M.BASE_OUT], cptr, be.stream))
    be.sync()
    worst = 0.
    for n in M.BASE_OUT:
        got, w = be.host(out[n]), written(g, n)
        mask = np.ones(g.kcells, dtype=bool); mask[w] = False
        assert (got[mask] == -7.).all(), n
        worst = max(worst, M.rel(got[w], want[n][w]))
    print("base state %s %s, device recurrence on %s against the host entry: %.3e (bound %.3e)" % (name, M.tag(dtype), be.name, worst, bound_dev(g)))
    assert worst <= bound_dev(g) and count() == 0
    # get_thermo_field refreshes the pressure and Exner profiles only: NULL outputs leave their arrays alone, the rest has the same bits
    part = {n: be.arr(np.full(g.kcells, -7., dtype=dtype)) for n in M.BASE_OUT}
    asked = ("pref", "prefh", "exnref", "exnrefh")
    B.ok(be, be.lib.mhh_thermo_moist_base_state(G, be.ptr(dthl), be.ptr(dqt), M.PBOT, *[be.ptr(part[n] if n in asked else None) for n in M.BASE_OUT],
                                                None, be.stream))
    be.sync()
    for n in M.BASE_OUT:
        if n in asked:
            assert cm.same_bits(be.host(part[n]), be.host(out[n])), n
        else:
            assert (be.host(part[n]) == -7.).all(), n
