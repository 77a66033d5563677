"""Thermo_moist's buoyancy tendency and diagnostic fields (csrc/thermo_moist.h) against the reference and against each other.

The inputs are warm (thl*exn >= T0 + 0.5 on every w level, asserted), so every cell takes the branch of sat_adjust that holds
+ - * /, max and fabs only: the marching form, the one-thread-per-cell form and the reference (tests/moist_ref.py: the shim on the
reference's own header where that tree exists, tests/golden/moist_ref.npz elsewhere) agree bit for bit in fp64 and fp32 on both
backends. The Exner tables come from the reference's C library (recorded), since the device reads exnrefh[k] where the reference
recomputes exner(prefh[k]).
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import moist_ref as M
from backends import be  # noqa: F401
from microhh_amd import capi

MARCH, CELL = 0, 1
CASES = [(s, gc) for s in M.SHAPES for gc in M.GCS]
IDS = ["%dx%dx%d-gc%d%d%d" % (s + gc) for s, gc in CASES]


def offset_arr(be, a, nbytes):  # noqa: F811
    """A device copy of `a` whose first element lies nbytes past an allocation's start (1-D view of the same shape's size)."""
    pad = nbytes // a.itemsize
    flat = np.concatenate([np.zeros(pad, dtype=a.dtype), a.ravel()])
    return be.arr(flat)[pad:]


class Tend:
    """The arrays of one (shape, gc, dtype) on a backend."""

    def __init__(self, be, shape, gc, dtype, nbytes=0):  # noqa: F811
        self.be, self.c, self.g = be, M.field_case(shape), M.grid_of(shape, gc, dtype)
        c, g = self.c, self.g
        self.key = "field/%s/%s/" % (c.key, M.tag(dtype))
        self.host = {n: c.embed(np.asarray(a, dtype=dtype), g) for n, a in (("thl", c.thl), ("qt", c.qt), ("wt", c.wt))}
        self.tab = {n: np.ascontiguousarray(getattr(c, n), dtype=dtype) for n in ("pref", "prefh", "thvref", "thvrefh")}
        for n in ("exnref", "exnrefh"):
            self.tab[n] = M.ref(self.key + n, be)
        ks, ke = g.kstart, g.kend
        assert (c.thl[ks+1:ke].astype(dtype) * self.tab["exnrefh"][ks+1:ke, None, None] >= dtype(M.T0 + 1.)).all()
        self.G = be.grid(g)
        self.d = {n: (offset_arr(be, a, nbytes) if nbytes else be.arr(a)) for n, a in self.host.items()}
        self.t = {n: be.arr(a) for n, a in self.tab.items()}
        self.keep, self.cptr, self.count = M.counter(be)

    def tend(self, impl=None):
        be, d, t = self.be, self.d, self.t
        a = (be.ptr(d["wt"]), be.ptr(d["thl"]), be.ptr(d["qt"]), be.ptr(t["prefh"]), be.ptr(t["exnrefh"]), be.ptr(t["thvrefh"]), self.cptr, be.stream)
        if impl is None:
            B.ok(be, be.lib.mhh_thermo_moist_buoyancy_tend(self.G, *a))
        else:
            B.ok(be, be.lib.mhh_thermo_moist_buoyancy_tend_impl(self.G, impl, *a))
        be.sync()
        return be.host(d["wt"]).reshape(self.g.shape3)


def check_tend(be, x, got, label):  # noqa: F811
    g = x.g
    want = x.host["wt"].copy()
    want[g.interior] = M.ref(x.key + "wt", be)
    inner = (slice(g.kstart+1, g.kend), slice(g.jstart, g.jend), slice(g.istart, g.iend))
    assert cm.same_bits(got[inner], want[inner]), (label, M.rel(got[inner], want[inner]))
    assert not np.array_equal(want[inner], x.host["wt"][inner])
    assert cm.same_bits(got, want), (label, "kstart, kend and the ghost cells are untouched")
    assert x.count() == 0


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES, ids=IDS)
def test_tendency_is_the_references(be, shape, gc, dtype):  # noqa: F811
    """The marching form (the default entry) and the cell form against the reference; the last shape in chunks of 8 levels."""
    with cm.switches(MHH_MARCH_KC_RT=8 if shape[2] == 40 else None):
        x = Tend(be, shape, gc, dtype)
        check_tend(be, x, x.tend(), "march")
        y = Tend(be, shape, gc, dtype)
        check_tend(be, y, y.tend(MARCH), "march by name")
    z = Tend(be, shape, gc, dtype)
    check_tend(be, z, z.tend(CELL), "cell")


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_tendency_with_base_pointers_8_bytes_off_16(be, dtype):  # noqa: F811
    x = Tend(be, (70, 9, 10), (3, 3, 1), dtype, nbytes=8)
    for n in ("wt", "thl", "qt"):
        assert be.ptr(x.d[n]).value % 16 == 8
    check_tend(be, x, x.tend(), "march, misaligned")


def test_refusals_name_their_reason(be):  # noqa: F811
    x = Tend(be, (20, 1, 12), (1, 1, 1), np.float64)
    a = (be.ptr(x.d["wt"]), be.ptr(x.d["thl"]), be.ptr(x.d["qt"]), be.ptr(x.t["prefh"]), be.ptr(x.t["exnrefh"]), be.ptr(x.t["thvrefh"]), None, be.stream)
    assert be.lib.mhh_thermo_moist_buoyancy_tend_impl(x.G, 7, *a) != 0
    assert b"impl" in be.lib.mhh_last_error()
    assert be.lib.mhh_thermo_moist_buoyancy_tend(x.G, None, *a[1:]) != 0
    assert b"null field" in be.lib.mhh_last_error()
    assert be.lib.mhh_thermo_moist_fields(x.G, *[a[1]]*5, None, None, None, None, None, be.stream) != 0
    assert b"no output" in be.lib.mhh_last_error()


# ---- the diagnostic fields ---------------------------------------------------------------------------------------------------
FIELDS = ("b", "ql", "qi", "T")
POISON = -123.


def run_fields(be, x, names):  # noqa: F811
    out = {n: be.arr(np.full(x.g.shape3, POISON, dtype=x.g.np_dtype)) for n in FIELDS}
    d, t = x.d, x.t
    B.ok(be, be.lib.mhh_thermo_moist_fields(x.G, be.ptr(d["thl"]), be.ptr(d["qt"]), be.ptr(t["pref"]), be.ptr(t["exnref"]), be.ptr(t["thvref"]),
                                            *[be.ptr(out[n] if n in names else None) for n in FIELDS], x.cptr, be.stream))
    be.sync()
    return {n: be.host(out[n]) for n in FIELDS}


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", M.SHAPES[1:3], ids=["17x9x8", "20x1x12"])
def test_fields_are_the_references_and_subsets_agree(be, shape, dtype):  # noqa: F811
    x = Tend(be, shape, (3, 3, 1), dtype)
    g = x.g
    full = run_fields(be, x, FIELDS)
    cols = (slice(None), slice(g.jstart, g.jend), slice(g.istart, g.iend))
    for n in FIELDS:
        want = np.full(g.shape3, POISON, dtype=dtype)
        if n == "b":
            want[cols] = M.ref(x.key + "b", be)          # every level; ql = qi = 0 on the ghost levels
        else:
            want[g.interior] = M.ref(x.key + n, be)
        assert cm.same_bits(full[n], want), (n, M.rel(full[n], want))
    assert np.count_nonzero(full["ql"][g.interior]) > 0.1*full["ql"][g.interior].size
    # b outside [kstart, kend) is the unsaturated expression
    thl, qt = x.host["thl"][0][cols[1:]].astype(np.float64), x.host["qt"][0][cols[1:]].astype(np.float64)
    dry = 9.81*(thl*(1. - (1. - 461.5/287.04)*qt) - x.tab["thvref"][0])/x.tab["thvref"][0]
    assert np.allclose(full["b"][0][cols[1:]], dry, rtol=1e-5, atol=1e-6)
    # every subset of the outputs: the bits of the all-outputs call, and nothing else written
    for mask in range(1, 15):
        names = [n for i, n in enumerate(FIELDS) if mask >> i & 1]
        part = run_fields(be, x, names)
        for n in FIELDS:
            if n in names:
                assert cm.same_bits(part[n], full[n]), (names, n)
            else:
                assert (part[n] == POISON).all(), (names, n)
    assert x.count() == 0


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_N2_is_the_dry_expression_with_thvref(be, dtype):  # noqa: F811
    """get_thermo_field("N2"): mhh_diff_exec_viscosity with buoyancy_kind = 0, th_for_N2 = the index of thl, thref = thvref and
    buoyancy = 0 against the reference's calc_N2 followed by the same call with that N2 supplied."""
    shape = (17, 9, 8)
    x = Tend(be, shape, (3, 3, 1), dtype)
    g = x.g
    c = cm.Case(g, nscalars=2, periodic=True)
    c.s[1] = x.host["thl"]
    n2 = np.zeros(g.shape3, dtype=dtype)
    n2[g.interior] = M.ref(x.key + "N2", be)
    out = {}
    for mode in ("inline", "supplied"):
        d = B.DevCase(be, c); f = d.fields()
        p = cm.diff_params(1)
        p.buoyancy_kind = 0; p.buoyancy = 0; p.grav = 9.81
        dn2, dth = be.arr(n2), be.arr(x.tab["thvref"])
        if mode == "inline":
            p.N2 = None; p.th_for_N2 = 1; p.thref = be.ptr(dth).value
        else:
            p.N2 = be.ptr(dn2).value
        ml = B.mlen0(be, g, 0.23); p.mlen0 = be.ptr(ml).value
        B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
        be.sync()
        out[mode] = be.host(d.evisc)
    assert cm.same_bits(out["inline"], out["supplied"]), cm.ulp_diff(out["inline"], out["supplied"])
    assert np.isfinite(out["inline"][g.interior]).all() and out["inline"][g.interior].max() > 0


# ---- the BOMEX field ---------------------------------------------------------------------------------------------------------
def test_bomex_field_is_partly_cloudy(be):  # noqa: F811
    """The input condition of the cost runs, asserted on the reference's result: on the synthetic BOMEX field at 64 x 8 x 64 at
    least 1 % of the w-level cells are saturated and at least 25 % are not. Where the shim is built, the device gives its bits."""
    nsat, ncells = (int(v) for v in M.ref("bomex/nsat", be))
    assert ncells == 64*8*63
    print("bomex 64x8x64: %d of %d w-level cells saturated (%.2f %%)" % (nsat, ncells, 100.*nsat/ncells))
    assert nsat >= 0.01*ncells and ncells - nsat >= 0.25*ncells
    if not M.exact_here(be):
        return
    want, _, _, tab = M.bomex_reference()
    g, thl, qt, wt, _ = M.bomex_inputs(np.float64, None)
    d = [be.arr(a) for a in (wt, thl, qt)] + [be.arr(a) for a in tab]
    keep, cptr, count = M.counter(be)
    B.ok(be, be.lib.mhh_thermo_moist_buoyancy_tend(be.grid(g), *[be.ptr(a) for a in d], cptr, be.stream))
    be.sync()
    assert cm.same_bits(be.host(d[0]), want) and count() == 0
