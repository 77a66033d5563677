"""Shared plumbing of the cross-section tests (tests/test_cross_*.py): the seeded cases and their reference results.

The reference is the reference's OWN source (src/cross.cxx) behind tests/cpp/ref_cross_shim.cpp, compiled into a temporary directory
where the reference tree exists. Where it is absent the same cases read tests/golden/cross_ref.npz, recorded with
MHH_RECORD_CROSS_GOLDEN=1 python -m pytest tests/test_cross_kernels.py: reference OUTPUTS only (lngrad of the interior, the path and
the two threshold heights). The inputs are not stored: every draw is numpy's seeded legacy generator, everything derived from a draw
uses + - * / only and is narrowed to values a float holds exactly, so they are the same numbers on every host and in both dtypes;
the file holds their digest per case. The gather has NumPy slicing as its reference and needs no shim.
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag
from microhh_amd.grid import Grid

ZSIZE = 3000.
KGMAX = 3                      # vertical ghost levels the inputs are drawn with

# (itot, jtot, ktot): 70 crosses a 64-lane row; jtot = 1 is the degenerate row; (17, 9, 8) is stretched
SHAPES = [(70, 9, 10), (20, 1, 12), (17, 9, 8)]
STRETCHED = {SHAPES[0]: False, SHAPES[1]: False, SHAPES[2]: True}
# (ghost cells, order): the two second-order layouts and the fourth-order one
GCS = [((1, 1, 1), 2), ((3, 3, 1), 2), ((3, 3, 3), 4)]
LAYOUTS = [(s, gc, order) for s in SHAPES for gc, order in GCS]
THRESHOLD = 0.25               # of the threshold heights: a value a float holds exactly, so that `equal` is equal in both dtypes
# the kinds of column of the thresholded field q, by (i + j*itot) % NKIND
NONE, ONLY_KSTART, ONLY_TOP, TWO_LAYERS, EQUAL, RANDOM = range(6)
NKIND = 6


XY, XZ, YZ, PLANE = 0, 1, 2, 3


def grid_of(shape, gc, order, dtype):
    z = None
    if STRETCHED[shape]:
        s = (np.arange(shape[2]) + 0.5)/shape[2]
        z = f32exact(ZSIZE*(s + 0.6*s*s)/1.6)
    return Grid(shape[0], shape[1], shape[2], 6400., 6400., ZSIZE, order=order, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype, z=z)


def column_kinds(shape):
    itot, jtot, _ = shape
    return (np.arange(jtot*itot) % NKIND).reshape(jtot, itot)


class CrossCase:
    """The fields of one shape on ktot + 2*KGMAX levels of jtot x itot columns, the same for every ghost layout and both dtypes:
    a (gather, lngrad, path), q (the threshold heights: one kind of column per residue of the column number), rho."""

    def __init__(self, shape):
        self.shape = shape
        self.key = "%dx%dx%d" % shape
        itot, jtot, ktot = shape
        rs = np.random.RandomState(9100 + itot + 7*ktot + 131*jtot)
        nk = ktot + 2*KGMAX
        n3 = (nk, jtot, itot)
        lev = np.arange(nk)[:, None, None]
        f = {}
        f["a"] = f32exact(3. + 0.25*lev + (rs.random_sample(n3) - 0.5))
        f["rho"] = f32exact(1.16 - 0.02*np.arange(nk) + 0.01*rs.random_sample(nk))
        below = f32exact(THRESHOLD*rs.random_sample(n3)*0.75)               # in [0, 0.1875]: never above the threshold
        above = f32exact(THRESHOLD + 0.125 + rs.random_sample(n3))
        kind = column_kinds(shape)[None]
        k = lev - KGMAX                                                     # the interior level, 0 .. ktot-1
        lo, hi = 1, ktot - 2                                                # the two layers of TWO_LAYERS (ktot >= 8: apart)
        q = np.where(kind == ONLY_KSTART, np.where(k == 0, above, below), below)
        q = np.where(kind == ONLY_TOP, np.where(k == ktot-1, above, below), q)
        q = np.where(kind == TWO_LAYERS, np.where((k == lo) | (k == hi), above, below), q)
        q = np.where(kind == EQUAL, np.where(k % 2 == 0, THRESHOLD, below), q)
        q = np.where(kind == RANDOM, np.where(rs.random_sample(n3) < 0.3, above, below), q)
        # the ghost levels would qualify: no loop may look at them
        q[:KGMAX] = 5.; q[KGMAX+ktot:] = 5.
        f["q"] = f32exact(q)
        self.f = f

    def digest(self):
        return refshim.digest(*[np.asarray(self.f[k], dtype=np.float64) for k in sorted(self.f)])

    def host(self, g):
        """Host arrays of grid g's dtype and layout: the vertical ghost levels hold the seeded values, the horizontal ghost cells the
        periodic images (Boundary_cyclic), as the model leaves them before a sample."""
        t, out = g.np_dtype, {}
        lv = slice(KGMAX - g.kgc, KGMAX + g.ktot + g.kgc)
        for k, a in self.f.items():
            if a.ndim == 3:
                out[k] = np.ascontiguousarray(np.pad(a[lv], [(0, 0), (g.jgc, g.jgc), (g.igc, g.igc)], mode="wrap"), dtype=t)
            else:
                out[k] = np.ascontiguousarray(a[lv], dtype=t)
        out["const"] = np.full(g.shape3, 2.5, dtype=t)
        return out


_cases = {}


def case_of(shape):
    if shape not in _cases:
        _cases[shape] = CrossCase(shape)
    return _cases[shape]


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    DP = C.POINTER(Dims)
    lib.ref_cross_lngrad.argtypes = [ci, DP, ci, vp, vp, cd, cd, vp]; lib.ref_cross_lngrad.restype = None
    lib.ref_cross_path.argtypes = [ci, DP, vp, vp, vp, vp]; lib.ref_cross_path.restype = None
    lib.ref_cross_height.argtypes = [ci, DP, vp, vp, vp, cd, ci]; lib.ref_cross_height.restype = None


shim = refshim.Shim("cross", ["ref_cross_shim.cpp"], _bind, stubs=True)


def inverse(g, d):
    """gd.dxi = 1./gd.dx (src/grid.cxx:244): a double quotient of the narrowed spacing, narrowed."""
    t = g.np_dtype.type
    return float(t(1./float(t(d))))


def ref_lngrad(g, a):
    """calc_lngrad_2nd / calc_lngrad_4th of the whole field a (host array of grid g), as Cross::cross_lngrad calls them."""
    out = np.zeros(g.shape3, dtype=g.np_dtype)
    d = dims_of(g)
    shim().ref_cross_lngrad(code(g.np_dtype), C.byref(d), g.order, cm.ptr(np.ascontiguousarray(a)), cm.ptr(out), inverse(g, g.dx), inverse(g, g.dy),
                            cm.ptr(g.dzi if g.order == 2 else g.dzi4))
    return out


def ref_path(g, a, rho):
    tmp = np.zeros(g.shape3, dtype=g.np_dtype)
    d = dims_of(g)
    shim().ref_cross_path(code(g.np_dtype), C.byref(d), cm.ptr(np.ascontiguousarray(a)), cm.ptr(tmp), cm.ptr(np.ascontiguousarray(rho)), cm.ptr(g.dz))
    return tmp[g.kstart, g.jstart:g.jend, g.istart:g.iend].copy()


def ref_height(g, a, threshold, upward):
    out = np.full(g.shape2, 777., dtype=g.np_dtype)
    d = dims_of(g)
    shim().ref_cross_height(code(g.np_dtype), C.byref(d), cm.ptr(np.ascontiguousarray(a)), cm.ptr(out), cm.ptr(g.z), threshold, int(upward))
    return out[g.jstart:g.jend, g.istart:g.iend].copy()


def ref_case(shape, gc, order, dtype):
    """Everything the reference gives on one case: {key: array of the interior}."""
    c, g = case_of(shape), grid_of(shape, gc, order, dtype)
    h = c.host(g)
    return {"lngrad": ref_lngrad(g, h["a"])[g.interior].copy(), "lngrad_const": ref_lngrad(g, h["const"])[g.interior].copy(),
            "path": ref_path(g, h["a"], h["rho"]), "base": ref_height(g, h["q"], THRESHOLD, True), "top": ref_height(g, h["q"], THRESHOLD, False)}


def case_key(shape, gc, order, dtype):
    return "%s/%d%d%d-o%d/%s/" % (case_of(shape).key, gc[0], gc[1], gc[2], order, tag(dtype))


def _compute_all():
    rec = {}
    for shape, gc, order in LAYOUTS:
        for dt in cm.DTYPES:
            for k, v in ref_case(shape, gc, order, dt).items():
                rec[case_key(shape, gc, order, dt) + k] = v
        rec["digest/%s" % case_of(shape).key] = np.array(case_of(shape).digest())
    return rec


GOLD = refshim.Golden("cross", _compute_all, "tests/test_cross_kernels.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(shape, gc, order, dtype, name, be=None):
    """A reference result by name (Golden.ref)."""
    return GOLD.ref(case_key(shape, gc, order, dtype) + name, be)


# ---- what the tests hold the library against -------------------------------------------------------------------------------------
def numpy_plane(g, a, kind, index, k0, k1, off):
    """What save_xy_slice / save_xz_slice / save_yz_slice (src/field3d_io.cxx:754-861) put into tmp: data + TF(data0)."""
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    o = g.np_dtype.type(off)
    if kind == PLANE:
        return a[js, ie] + o
    if kind == XY:
        return a[index, js, ie] + o
    if kind == XZ:
        return a[k0:k1, index, ie] + o
    return a[k0:k1, js, index] + o


def lngrad_bound(g, want):
    """|got - want| for log(dtiny + gx^2 + gy^2 + gz^2), derived, not tuned:
      - gx, gy, gz have the reference's bits (the same expressions, no contraction on either side). The reference squares with pow(x, 2),
        within 1 ulp of x^2; x*x here is correctly rounded. So each square differs by at most one ulp of the type it is formed in:
        TF in calc_lngrad_2nd (pow(x, TF(2))), double in calc_lngrad_4th (pow(x, 2.)): relative 2^-23 or 2^-52.
      - the three additions in double are of positive terms, so the sum carries at most that relative difference, plus one ulp of
        double per addition whose rounding falls differently: 3 * 2^-52.
      - log(s (1 + e)) = log(s) + e: the logarithm moves by the same ABSOLUTE amount e.
      - the two logarithms: glibc's log is within 1 ulp of the result, the device library's within 3 ulp (the OpenCL bound its
        documentation states for log); in ulp of double at the result.
      - on a float grid both sides narrow last: one ulp of float at the result.
    """
    f32 = g.np_dtype == np.float32
    e = (2.**-23 if (f32 and g.order == 2) else 2.**-52) + 3*2.**-52
    w = np.abs(want.astype(np.float64))
    return e + 4.*np.spacing(w) + (np.spacing(np.abs(want)).astype(np.float64) if f32 else 0.)
