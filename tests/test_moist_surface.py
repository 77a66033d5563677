"""The surface layer with Thermo_moist's hooks (thermo_kind MHH_THERMO_MOIST: calc_buoyancy_bot, calc_buoyancy_fluxbot, get_db_ref
inline in the stage kernels, csrc/surface_layer.h).

Thermo_buoy's hooks are plain copies and pinned to the reference (tests/test_surface_ref.py), so the oracle of kind 3 is the existing
BUOY path fed with arrays evaluated on the host: b and bbot (buoyancy_no_ql), bfluxbot (buoyancy_flux_no_ql) and bg_n2 := db_ref.
None of them holds a transcendental, so obuk, nobuk, ustar and dbdz agree bit for bit on both backends, fp64 and fp32. The host
evaluation is numpy's in the dtype, in the reference's expression order; test_host_hooks_are_the_references holds it against the shim
on the reference's own header, bit for bit, where the reference tree exists (the dirichlet case combines fluxes the DEVICE wrote, so
a recorded file could not hold that reference)."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import moist_ref as M
import surface_ref as S
from backends import be  # noqa: F401
from common import same_bits as same

MOIST = 3
SHAPES = [S.SMALL, (70, 9, 10, (3, 3, 1))]
IDS = ["20x1x12", "70x9x10"]
THVREF, THVREFH = 301.78631591796875, 301.7748107910156          # float32-exact: thvref[kstart], thvrefh[kstart] of the BOMEX base state
# (mbcbot, bottom bc of thl and qt)
CONFIGS = {"flux": (S.DIRICHLET, S.FLUX), "flux_ustar": (S.USTAR, S.FLUX), "dirichlet": (S.DIRICHLET, S.DIRICHLET)}


# ---- Thermo_moist's hooks on the host (include/thermo_moist_functions.h:65-75, src/thermo_moist.cxx:1713-1717) -------------------
def buoyancy_no_ql(thl, qt, thvref):
    t = thl.dtype.type
    return t(9.81) * (thl * (t(1.) - (t(1.) - t(461.5)/t(287.04))*qt) - thvref) / thvref


def buoyancy_flux_no_ql(thl, thlflux, qt, qtflux, thvref):
    t = thl.dtype.type
    return t(9.81)/thvref * (thlflux * (t(1.) - (t(1.)-t(461.5)/t(287.04))*qt) - (t(1.)-t(461.5)/t(287.04))*thl*qtflux)


def db_ref(t):
    return t(9.81)/t(THVREF)*(t(THVREF) - t(THVREFH))


class Case:
    """What surface_ref.DevSurf reads of a case."""
    state, out_names = S.SurfCase.state, S.SurfCase.out_names

    def __init__(self, shape, dtype, mbcbot, kind, sbc):
        self.shape, self.dtype, self.mbcbot, self.kind, self.sbc, self.thermobc = shape, np.dtype(dtype), mbcbot, kind, sbc, sbc[0]
        self.g = S.grid_of(shape, dtype)
        self.config = "moist"


def inputs(shape, dtype, bc):
    """u, v of surface_ref's seeded case; thl, qt at kstart, their bottom values (both signs of db) and fluxes; float32-exact."""
    wind = S.SurfCase("flux", shape, dtype)
    g = wind.g
    rs = np.random.RandomState(77 + shape[0])
    n2 = g.shape2
    m = {"u": wind.master["u"], "v": wind.master["v"]}
    m["s0"] = S.wrap(298.7 + 0.5*rs.random_sample(n2), g); m["s1"] = S.wrap(16.e-3 + 2.e-3*rs.random_sample(n2), g)
    thlbot = S.wrap(299.0 + 0.8*(rs.random_sample(n2) - 0.5), g); qtbot = S.wrap(17.e-3 + 3.e-3*(rs.random_sample(n2) - 0.5), g)
    sign = np.where(rs.random_sample(n2) < 0.3, -3., 1.)         # a buoyancy flux of both signs (qt's share is positive)
    thlflux = S.wrap(sign*(4.e-3 + 8.e-3*rs.random_sample(n2)), g); qtflux = S.wrap(2.e-5 + 6.e-5*rs.random_sample(n2), g)
    zero = np.zeros(n2)
    m["sbot0"], m["sbot1"] = (thlbot, qtbot) if bc == S.DIRICHLET else (zero, zero)
    m["sfluxbot0"], m["sfluxbot1"] = (thlflux, qtflux) if bc == S.FLUX else (zero, zero)
    m = {k: np.ascontiguousarray(M.f32exact(v), dtype=dtype) for k, v in m.items()}
    return m, {"thlbot": np.ascontiguousarray(M.f32exact(thlbot), dtype=dtype), "qtbot": np.ascontiguousarray(M.f32exact(qtbot), dtype=dtype)}


def moist_dev(be, shape, dtype, config, inp):  # noqa: F811
    mbc, bc = CONFIGS[config]
    case = Case(shape, dtype, mbc, MOIST, [bc, bc])
    d = S.DevSurf(be, case, inp, case.state())
    g = case.g
    tab = np.zeros(g.kcells, dtype=dtype); tabh = np.zeros(g.kcells, dtype=dtype)
    tab[g.kstart], tabh[g.kstart] = THVREF, THVREFH
    d.tabs = (be.arr(tab), be.arr(tabh))
    d.p.qt_index, d.p.thvref, d.p.thvrefh = 1, be.ptr(d.tabs[0]).value, be.ptr(d.tabs[1]).value
    return d


def buoy_dev(be, shape, dtype, config, inp, bflux=None):  # noqa: F811
    """The BUOY path on b, bbot, bfluxbot evaluated on the host from the moist inputs, with bg_n2 = db_ref."""
    mbc, bc = CONFIGS[config]
    t = np.dtype(dtype).type
    zero = np.zeros_like(inp["s0"])
    oin = {"u": inp["u"], "v": inp["v"], "s0": buoyancy_no_ql(inp["s0"], inp["s1"], t(THVREF)),
           "sbot0": buoyancy_no_ql(inp["sbot0"], inp["sbot1"], t(THVREFH)) if bc == S.DIRICHLET else zero,
           "sfluxbot0": bflux if bflux is not None else
           buoyancy_flux_no_ql(inp["s0"], inp["sfluxbot0"], inp["s1"], inp["sfluxbot1"], t(THVREFH)) if bc == S.FLUX else zero}
    assert all(v.dtype == np.dtype(dtype) for v in oin.values())
    case = Case(shape, dtype, mbc, S.BUOY, [bc])
    d = S.DevSurf(be, case, oin, case.state())
    d.p.bg_n2 = float(db_ref(t))
    return d


def stability(d):
    dut = d.be.ptr(d.a["dutot"])
    d.call("mhh_surface_dutot", dut); d.fill("dutot")
    d.call("mhh_surface_stability", dut)


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_host_hooks_are_the_references(dtype):
    """not gpu: the numpy restatement of the three hooks against the shim on the reference's header, bit for bit."""
    if not M.have_reference():
        pytest.skip("the reference tree is absent")
    inp, bot = inputs(SHAPES[1], dtype, S.FLUX)
    n = inp["s0"].size
    t = np.dtype(dtype).type
    out = [np.zeros(n, dtype=dtype) for _ in range(3)] + [np.zeros(1, dtype=dtype)]
    M.shim().ref_moist_surf_hooks(M.code(dtype), n, *[cm.ptr(np.ascontiguousarray(a.ravel())) for a in
                                  (inp["s0"], inp["s1"], bot["thlbot"], bot["qtbot"], inp["sfluxbot0"], inp["sfluxbot1"])], THVREF, THVREFH,
                                  *[cm.ptr(a) for a in out])
    assert same(out[0], buoyancy_no_ql(inp["s0"], inp["s1"], t(THVREF)).ravel())
    assert same(out[1], buoyancy_no_ql(bot["thlbot"], bot["qtbot"], t(THVREFH)).ravel())
    assert same(out[2], buoyancy_flux_no_ql(inp["s0"], inp["sfluxbot0"], inp["s1"], inp["sfluxbot1"], t(THVREFH)).ravel())
    assert out[3][0] == db_ref(t) and out[3].dtype == np.dtype(dtype)
    assert (out[2] > 0).any() and (out[2] < 0).any() and ((out[0] - out[1]) > 0).any() and ((out[0] - out[1]) < 0).any()


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_stability_and_gradients_equal_the_buoy_path(be, config, shape, dtype):  # noqa: F811
    mbc, bc = CONFIGS[config]
    inp, _ = inputs(shape, dtype, bc)
    g = S.grid_of(shape, dtype)
    core = (slice(g.jstart, g.jend), slice(g.istart, g.iend))
    m = moist_dev(be, shape, dtype, config, inp)
    stability(m)
    if bc == S.FLUX:
        o = buoy_dev(be, shape, dtype, config, inp)
        stability(o)
        m.call("mhh_surface_mo_gradients"); o.call("mhh_surface_mo_gradients")
    else:
        # dirichlet: the device's surfs writes the fluxes of thl and qt; their combination on the host is the BUOY path's flux
        m.call("mhh_surface_momentum"); m.fill("ufluxbot"); m.fill("vfluxbot")
        m.call("mhh_surface_scalar", 0); m.call("mhh_surface_scalar", 1)
        m.call("mhh_surface_mo_gradients")
        mo = m.outputs()
        t = np.dtype(dtype).type
        bflux = buoyancy_flux_no_ql(inp["s0"], mo["sfluxbot0"], inp["s1"], mo["sfluxbot1"], t(THVREFH))
        assert not same(mo["sfluxbot0"], np.zeros_like(mo["sfluxbot0"]))
        o = buoy_dev(be, shape, dtype, config, inp, bflux=bflux)
        stability(o)
        o.call("mhh_surface_mo_gradients")
    mo, oo = m.outputs(), o.outputs()
    for k in ("obuk", "nobuk", "ustar"):
        assert same(mo[k], oo[k]), k
    assert same(mo["dbdz"][core], oo["dbdz"][core])
    assert np.isfinite(mo["obuk"]).all() and np.count_nonzero(mo["dbdz"][core]) > 0
    if mbc == S.DIRICHLET:
        assert (mo["nobuk"][core] > 0).all()                          # the walk moved


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_fused_call_equals_the_stages(be, config, shape, dtype):  # noqa: F811
    inp, _ = inputs(shape, dtype, CONFIGS[config][1])
    a = moist_dev(be, shape, dtype, config, inp); a.staged()
    b = moist_dev(be, shape, dtype, config, inp); b.fused()
    oa, ob = a.outputs(), b.outputs()
    for k in oa:
        assert same(oa[k], ob[k]), k


def test_refusals_name_their_reason(be):  # noqa: F811
    inp, _ = inputs(S.SMALL, np.float64, S.FLUX)
    d = moist_dev(be, S.SMALL, np.float64, "flux", inp)
    dut = be.ptr(d.a["dutot"])
    d.p.sbcbot[1] = S.DIRICHLET
    assert be.lib.mhh_surface_stability(d.G, C.byref(d.f), C.byref(d.p), dut, be.stream) != 0
    assert b"same kind of bottom bc" in be.lib.mhh_last_error()
    d.p.sbcbot[1] = S.FLUX; d.p.thvrefh = None
    assert be.lib.mhh_boundary_surface_exec(d.G, C.byref(d.f), C.byref(d.p), dut, be.stream) != 0
    assert b"thvref" in be.lib.mhh_last_error()
    d.p.thvrefh = be.ptr(d.tabs[1]).value; d.p.qt_index = 0
    assert be.lib.mhh_surface_stability(d.G, C.byref(d.f), C.byref(d.p), dut, be.stream) != 0
    assert b"qt_index" in be.lib.mhh_last_error()
