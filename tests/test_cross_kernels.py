"""The kernels of csrc/cross.h against their references: the gather against NumPy slicing (bit for bit, with a canary around every
plane), calc_cross_path and calc_cross_height_threshold against the reference's own loops (bit for bit), calc_lngrad_2nd / _4th
against them within a derived bound, and the refusals of the entry points. References: tests/cross_ref.py."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import cross_ref as R
from backends import be, ok  # noqa: F401
from microhh_amd import capi

XY, XZ, YZ, PLANE = 0, 1, 2, 3
CASES = [(s, gc, o, dt) for s, gc, o in R.LAYOUTS for dt in cm.DTYPES]
IDS = ["%dx%dx%d-%d%d%d-o%d-%s" % (s + gc + (o, R.tag(dt))) for s, gc, o, dt in CASES]
CANARY = 0xA5
PAD = 3                         # canary elements in front of, between and behind the planes


def test_record_golden():
    """With MHH_RECORD_CROSS_GOLDEN=1 this writes tests/golden/cross_ref.npz; always: the inputs behind the stored results are the
    ones this host draws."""
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/cross_ref.npz is missing"
    for shape in R.SHAPES:
        assert str(z["digest/%s" % R.case_of(shape).key]) == R.case_of(shape).digest()


@pytest.mark.skipif(not R.have_reference(), reason="the reference tree is not on this machine")
def test_golden_is_the_shim():
    z, rec = R.golden(), R.computed()
    assert set(z.files) == set(rec)
    for k in rec:
        assert (str(z[k]) == str(rec[k])) if k.startswith("digest/") else cm.same_bits(z[k], rec[k]), k


def shape_of(g, kind, k0, k1):
    return (g.jmax, g.imax) if kind in (XY, PLANE) else (k1 - k0, g.imax if kind == XZ else g.jmax)


class Staging:
    """A staging buffer of canary bytes with PAD elements around every plane, and the jobs that write into it."""

    def __init__(self, be, g, specs):
        """specs: (field on the backend, kind, index, k0, k1, offset)."""
        self.be, self.g, self.specs = be, g, specs
        self.pos, n = [], PAD
        for _, kind, _, k0, k1, _ in specs:
            r, c = shape_of(g, kind, k0, k1)
            self.pos.append(n)
            n += r*c + PAD
        self.start = np.frombuffer(bytes([CANARY])*(n*g.np_dtype.itemsize), dtype=g.np_dtype).copy()
        self.dev = be.arr(self.start)
        size = g.np_dtype.itemsize
        self.jobs = (capi.MhhCrossJob*len(specs))(*[capi.MhhCrossJob(be.ptr(f).value, kind, index, k0, k1, float(off), be.ptr(self.dev).value + p*size)
                                                    for (f, kind, index, k0, k1, off), p in zip(specs, self.pos)])

    def planes(self):
        """The planes as written, after checking that every byte outside them is the canary still."""
        got = self.be.host(self.dev)
        outside = np.ones(got.size, dtype=bool)
        out = []
        for (_, kind, _, k0, k1, _), p in zip(self.specs, self.pos):
            r, c = shape_of(self.g, kind, k0, k1)
            outside[p:p + r*c] = False
            out.append(got[p:p + r*c].reshape(r, c))
        assert np.array_equal(got.view(np.uint8).reshape(got.size, -1)[outside], self.start.view(np.uint8).reshape(got.size, -1)[outside])
        return out


# ---- gather ---------------------------------------------------------------------------------------------------------------------
# An offset whose narrowing matters in fp32: as a float it is 1 + 2^-22, which puts a value of [4, 7) exactly between two floats
# (a tie, to even); as the double it is, the sum lies just below that midpoint and rounds down.
NARROW = 1. + 2.**-22*(1. - 2.**-20)
OFFSETS = (0., 0.5, NARROW, -2.25)    # none; float-exact; the one whose narrowing matters; another exact one


@pytest.mark.parametrize("shape,gc,order,dtype", CASES, ids=IDS)
def test_gather_is_numpy_slicing(be, shape, gc, order, dtype):  # noqa: F811
    g = R.grid_of(shape, gc, order, dtype)
    h = R.case_of(shape).host(g)
    a, a2 = h["a"], np.ascontiguousarray(h["q"][g.kstart] + g.np_dtype.type(1.))
    da, da2 = be.arr(a), be.arr(a2)
    ks, ke = g.kstart, g.kend
    where = ([(XY, k, 0, 0) for k in (ks, ke-1, ke)] +                          # first and last level, the half level kmax (kend of w)
             [(XZ, j, ks, ke) for j in (g.jstart, g.jend-1, g.jend)] +          # first and last row, the half row jtot (north ghost row)
             [(YZ, i, ks, ke) for i in (g.istart, g.iend-1)] +                  # first and last column
             [(XZ, g.jstart, ks+1, ke-1), (YZ, g.istart + g.imax//2, ks+2, ke), (XZ, g.jstart, 0, g.kcells)])
    specs = [(da, kind, idx, k0, k1, off) for off in OFFSETS for kind, idx, k0, k1 in where] + [(da2, PLANE, 0, 0, 0, off) for off in OFFSETS]
    assert len(specs) > 32      # more jobs than travel with one launch
    st = Staging(be, g, specs)
    ok(be, be.lib.mhh_cross_gather(be.grid(g), st.jobs, len(specs), be.stream))
    be.sync()
    for (f, kind, idx, k0, k1, off), got in zip(specs, st.planes()):
        want = R.numpy_plane(g, a2 if kind == PLANE else a, kind, idx, k0, k1, off)
        assert cm.same_bits(got, np.ascontiguousarray(want)), (kind, idx, k0, k1, off)
    if np.dtype(dtype) == np.float32:
        # the offset is narrowed BEFORE the add (TF data0): adding the double and narrowing the sum gives other bits somewhere
        late = (a[g.interior].astype(np.float64) + NARROW).astype(np.float32)
        assert not np.array_equal(late, a[g.interior] + np.float32(NARROW))


# ---- path -----------------------------------------------------------------------------------------------------------------------
def serial_path(g, a, rho, assoc):
    """The column sums in the dtype, level by level: assoc "ref" is (rho*data)*dz, "table" is data*(rho*dz)."""
    t = g.np_dtype.type
    acc = np.zeros((g.jmax, g.imax), dtype=g.np_dtype)
    for k in range(g.kstart, g.kend):
        d = a[k, g.jstart:g.jend, g.istart:g.iend]
        acc = acc + ((t(rho[k])*d)*t(g.dz[k]) if assoc == "ref" else d*t(t(rho[k])*t(g.dz[k])))
    return acc


@pytest.mark.parametrize("shape,gc,order,dtype", CASES, ids=IDS)
def test_path_has_the_references_bits(be, shape, gc, order, dtype):  # noqa: F811
    g = R.grid_of(shape, gc, order, dtype)
    h = R.case_of(shape).host(g)
    out, da, drho = be.zeros((g.jmax, g.imax), dtype), be.arr(h["a"]), be.arr(h["rho"])
    ok(be, be.lib.mhh_cross_path(be.grid(g), be.ptr(da), be.ptr(drho), be.ptr(out), be.stream))
    be.sync()
    want = R.ref(shape, gc, order, dtype, "path", be)
    assert cm.same_bits(be.host(out), want)
    assert cm.same_bits(serial_path(g, h["a"], h["rho"], "ref"), want)
    if R.STRETCHED[shape] and np.dtype(dtype) == np.float32:
        # the operand order is under test: rhoref[k]*data*dz[k] is (rho*data)*dz. Multiplication commutes, so Stats' data*rho*dz has the
        # same bits; the association that differs is data*(rho*dz), what a per-level table of rho*dz would give. (In fp32 only: the
        # inputs are float-exact, so in fp64 the first product of either association is exact and both round the same triple product.)
        assert not np.array_equal(serial_path(g, h["a"], h["rho"], "table"), want)


# ---- threshold heights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gc,order,dtype", CASES, ids=IDS)
def test_threshold_heights_have_the_references_bits(be, shape, gc, order, dtype):  # noqa: F811
    g = R.grid_of(shape, gc, order, dtype)
    h = R.case_of(shape).host(g)
    kinds = R.column_kinds(shape)
    assert set(np.unique(kinds)) == set(range(R.NKIND))                   # every kind of column is in every shape
    dq = be.arr(h["q"])
    res = {}
    for name, up in (("base", 1), ("top", 0)):
        out = be.zeros((g.jmax, g.imax), dtype)
        ok(be, be.lib.mhh_cross_height_threshold(be.grid(g), be.ptr(dq), R.THRESHOLD, up, be.ptr(out), be.stream))
        be.sync()
        res[name] = be.host(out)
        assert cm.same_bits(res[name], R.ref(shape, gc, order, dtype, name, be)), name
    fill = g.np_dtype.type(-1e-9)
    z = g.z
    for name in ("base", "top"):
        assert np.all(res[name][kinds == R.NONE] == fill)                 # none above the threshold
        assert np.all(res[name][kinds == R.EQUAL] == fill)                # equal to the threshold is not above it
        assert np.all(res[name][kinds == R.ONLY_KSTART] == z[g.kstart])
        assert np.all(res[name][kinds == R.ONLY_TOP] == z[g.kend-1])
    assert np.all(res["base"][kinds == R.TWO_LAYERS] == z[g.kstart+1]) and np.all(res["top"][kinds == R.TWO_LAYERS] == z[g.kend-2])


# ---- lngrad ---------------------------------------------------------------------------------------------------------------------
def lngrad_planes(g):
    ks, ke = g.kstart, g.kend
    return [(XY, ks, 0, 0), (XY, ke-1, 0, 0), (XY, ks + g.kmax//2, 0, 0), (XZ, g.jstart + g.jmax//2, ks, ke), (YZ, g.istart + g.imax//3, ks, ke)]


_worst = {}


@pytest.mark.parametrize("shape,gc,order,dtype", CASES, ids=IDS)
def test_lngrad_within_the_derived_bound(be, shape, gc, order, dtype):  # noqa: F811
    g = R.grid_of(shape, gc, order, dtype)
    h = R.case_of(shape).host(g)
    for name, fld in (("lngrad", h["a"]), ("lngrad_const", h["const"])):
        d = be.arr(fld)
        specs = [(d, kind, idx, k0, k1, 0.) for kind, idx, k0, k1 in lngrad_planes(g)]
        st = Staging(be, g, specs)
        ok(be, be.lib.mhh_cross_lngrad(be.grid(g), order, st.jobs, len(specs), be.stream))
        be.sync()
        full = np.zeros(g.shape3, dtype=g.np_dtype)
        full[g.interior] = R.ref(shape, gc, order, dtype, name, be)
        for (_, kind, idx, k0, k1, _), got in zip(specs, st.planes()):
            want = R.numpy_plane(g, full, kind, idx, k0, k1, 0.)
            diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
            tol = R.lngrad_bound(g, want)
            key = (be.name, order, R.tag(dtype))
            _worst[key] = max(_worst.get(key, 0.), float((diff/tol).max()))
            assert np.all(diff <= tol), (name, kind, idx, float((diff/tol).max()))
    print("lngrad worst |got - want| / bound so far:", {"%s-o%d-%s" % k: "%.3f" % v for k, v in _worst.items()})


@pytest.mark.parametrize("shape,gc,order,dtype", CASES, ids=IDS)
def test_lngrad_of_a_constant_field_is_log_dtiny(be, shape, gc, order, dtype):  # noqa: F811
    """dtiny and the double-precision sum on float grids: every gradient is zero, so every cell is log(1e-30), narrowed. Order 2: the
    constant 2.5 (interp2 of equal values is exact). Order 4: the constant 0, because with any other constant the four products with
    cg0 .. cg3 do not cancel in the dtype and the reference itself is far from log(dtiny) (-41.75 instead of -69.08 at 2.5 in float)."""
    g = R.grid_of(shape, gc, order, dtype)
    d = be.arr(np.full(g.shape3, 2.5 if order == 2 else 0., dtype=g.np_dtype))
    specs = [(d, kind, idx, k0, k1, 0.) for kind, idx, k0, k1 in lngrad_planes(g)]
    st = Staging(be, g, specs)
    ok(be, be.lib.mhh_cross_lngrad(be.grid(g), order, st.jobs, len(specs), be.stream))
    be.sync()
    want = g.np_dtype.type(np.log(1.e-30))
    for got in st.planes():
        assert np.all(np.abs(got.astype(np.float64) - float(want)) <= R.lngrad_bound(g, np.full(got.shape, want)))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(be):  # noqa: F811
    g = R.grid_of(R.SHAPES[2], (3, 3, 1), 2, np.float64)
    a, out = be.arr(R.case_of(R.SHAPES[2]).host(g)["a"]), be.zeros((g.kcells*g.icells,), np.float64)
    G, lib = be.grid(g), be.lib

    def one(kind, index, k0, k1):
        return (capi.MhhCrossJob*1)(capi.MhhCrossJob(be.ptr(a).value, kind, index, k0, k1, 0., be.ptr(out).value))
    for job, reason in ((one(7, 0, 0, 0), "unknown kind 7"), (one(XY, g.kcells, 0, 0), r"index %d outside the rank's range \[0, %d\)" % (g.kcells, g.kcells)),
                        (one(XZ, -1, g.kstart, g.kend), "index -1 outside"), (one(YZ, g.icells, g.kstart, g.kend), "index %d outside" % g.icells),
                        (one(XZ, g.jstart, -1, g.kend), r"k0 = -1, k1 = %d outside \[0, %d\]" % (g.kend, g.kcells)),
                        (one(YZ, g.istart, 0, g.kcells + 1), "k1 = %d outside" % (g.kcells + 1)), (one(XZ, g.jstart, 5, 4), "k0 = 5, k1 = 4")):
        with pytest.raises(capi.MhhError, match=reason):
            ok(be, lib.mhh_cross_gather(G, job, 1, be.stream))
    with pytest.raises(capi.MhhError, match="at least one job"):
        ok(be, lib.mhh_cross_gather(G, one(XY, g.kstart, 0, 0), 0, be.stream))
    for order, job, reason in ((3, one(XY, g.kstart, 0, 0), "order: 2"), (2, one(PLANE, 0, 0, 0), "unknown kind 3"),
                               (2, one(XY, g.kend, 0, 0), "index %d outside" % g.kend), (2, one(XZ, g.jend, g.kstart, g.kend), "index %d outside" % g.jend),
                               (2, one(YZ, g.istart, g.kstart - 1, g.kend), "k0 = 0"), (4, one(XY, g.kstart, 0, 0), "three")):
        with pytest.raises(capi.MhhError, match=reason):
            ok(be, lib.mhh_cross_lngrad(G, order, job, 1, be.stream))
    with pytest.raises(capi.MhhError, match="null pointer"):
        ok(be, lib.mhh_cross_path(G, be.ptr(a), None, be.ptr(out), be.stream))
    with pytest.raises(capi.MhhError, match="null pointer"):
        ok(be, lib.mhh_cross_height_threshold(G, None, 0., 1, be.ptr(out), be.stream))
    n = C.c_int(0)
    with pytest.raises(capi.MhhError, match="unknown kind"):
        ok(be, lib.mhh_cross_indices_host(g.host_struct(), PLANE, (C.c_double*1)(0.), 1, (C.c_int*1)(), C.byref(n), (C.c_int*1)(), C.byref(n)))
