"""Shared plumbing of the warm-rain microphysics tests (tests/test_micro_*.py): the seeded cases and their reference results.

The reference is the reference's OWN source (src/microphys_2mom_warm.cxx, src/limiter.cxx) behind tests/cpp/ref_micro_shim.cpp,
compiled into a temporary directory where the reference tree exists. Where it is absent the same cases read
tests/golden/micro_ref.npz, recorded with MHH_RECORD_MICRO_GOLDEN=1 python -m pytest tests/test_micro_exec.py: reference OUTPUTS only,
of runs that start from zero tendencies (so that the cells no process touches compress away). The inputs are not stored: every draw
is numpy's seeded legacy generator, everything derived from a draw uses + - * / only and is narrowed to values a float holds
exactly, so they are the same numbers on every host; the file holds their digest per case.
"""
import ctypes as C

import numpy as np

import common as cm
import moist_ref as M
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag
from microhh_amd.grid import Grid

PBOT = 101540.
NC0 = 70.e6
ZSIZE = 4000.

AUTO, ACCR, EVAP, SCBR, SEDI, CLIP = 1, 2, 4, 8, 16, 32
ALL = 63
PROCESSES = {"auto": AUTO, "accr": ACCR, "evap": EVAP, "scbr": SCBR, "sedi": SEDI}
OUT = ("qrt", "nrt", "thlt", "qtt")
# what a process writes (the others must keep their bits)
WRITES = {AUTO: OUT, ACCR: ("qrt", "thlt", "qtt"), EVAP: OUT, SCBR: ("nrt",), SEDI: ("qrt", "nrt", "rr_bot"), ALL: OUT + ("rr_bot",)}

# (itot, jtot, ktot) and whether the grid is stretched; the last one runs with 8 levels per chunk, so that a gather crosses a seam
SHAPES = M.SHAPES
STRETCHED = {(70, 9, 10): False, (17, 9, 8): True, (20, 1, 12): False, (130, 6, 40): True,
             (66, 100, 40): True, (130, 132, 9): False}       # the last two: tests/test_launch_geometry.py (no reference results, not in SHAPES)
GCS = M.GCS
CFLS = {"lo": 0.3, "hi": 3.5}
# the runs the golden file holds: every mask on the two small shapes (sedimentation with both steps), everything at once with the
# long step on all four; of the largest shape qtt is not kept (the same sums as thlt, which is): the file stays below 1 MB
SMALL = [(17, 9, 8), (20, 1, 12)]


def stored(shape, mask):
    """The outputs of a run that the golden file holds."""
    names = WRITES[ALL if mask == ALL else mask & ~CLIP]
    return tuple(n for n in names if not (shape == SHAPES[3] and n == "qtt"))


def grid_of(shape, gc, dtype):
    z = None
    if STRETCHED[shape]:
        s = (np.arange(shape[2]) + 0.5)/shape[2]
        z = f32exact(ZSIZE*(s + 0.6*s*s)/1.6)
    return Grid(shape[0], shape[1], shape[2], 12800., 12800., ZSIZE, order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype, z=z)


class RainCase:
    """Warm inputs of one shape on ktot + 2 levels of jtot x itot columns (the same for every ghost layout): thl, qt, qr, nr, four
    non-zero tendencies and the tables rho, p, exn. Rain in about half of the columns, a tenth of those in the top level only and a
    tenth in the bottom level only; negative qr and nr in a few cells anywhere; nr < 1; mean drop masses beyond both clamps; rain
    water below qr_min; ghost levels that hold rain of their own (the slopes read them)."""

    def __init__(self, shape):
        self.shape = shape
        self.key = "%dx%dx%d" % shape
        itot, jtot, ktot = shape
        rs = np.random.RandomState(7001 + itot + 7*ktot)
        g = grid_of(shape, (1, 1, 1), np.float64)
        n3, n2 = (ktot + 2, jtot, itot), (1, jtot, itot)
        z = g.z.astype(np.float64)
        z3 = z[:, None, None]
        s = 1. - z/44000.
        self.p = f32exact(PBOT*s*s*s*s*s)
        self.exn = f32exact(M.exn_like(self.p))
        self.rho = f32exact(1.16*(1. - z/22000.))
        self.thl = f32exact(297. + 0.006*z3 + (rs.random_sample(n3) - 0.5))
        assert (self.thl*self.exn[:, None, None] >= M.T0 + 0.6).all(), "warm inputs only"
        self.qt = f32exact((0.019 - 0.0025e-3*z3)*(0.55 + 0.65*rs.random_sample(n3)))
        # rain: which columns, which levels
        kind = rs.random_sample(n2)                          # < 0.5: rain; of those < 0.05 top only, < 0.10 bottom only
        lev = np.arange(ktot + 2)[:, None, None]
        wet = (kind < 0.5) & (rs.random_sample(n3) < 0.7)
        wet = np.where(kind < 0.05, lev >= ktot, np.where(kind < 0.10, lev <= 1, wet))
        u = rs.random_sample(n3)
        qr = 1.e-7 + 1.e-3*u*u*u*u
        u = rs.random_sample(n3)
        dr = 6.e-5 + 2.2e-3*u*u                              # the mean diameter aimed at: beyond mr_min and mr_max at the ends
        nr = self.rho[:, None, None]*qr/(3.14159265359*1.e3/6.*dr*dr*dr)
        few = rs.random_sample(n3)
        nr = np.where(few < 0.02, few*40., nr)               # nr < 1: the clamp in calc_rain_mass
        qr = np.where((few > 0.02) & (few < 0.03), 1.e-16*few, qr)       # 0 < qr <= qr_min
        qr, nr = np.where(wet, qr, 0.), np.where(wet, nr, 0.)
        neg = rs.random_sample(n3)
        qr = np.where(neg < 0.02, -1.e-6*neg, qr)            # spurious negative values, in dry columns too
        nr = np.where((neg > 0.01) & (neg < 0.03), -4000.*neg, nr)
        self.qr, self.nr = f32exact(qr), f32exact(nr)
        self.tend0 = {"qrt": f32exact(1.e-7*(rs.random_sample(n3) - 0.5)), "nrt": f32exact(10.*(rs.random_sample(n3) - 0.5)),
                      "thlt": f32exact(1.e-3*(rs.random_sample(n3) - 0.5)), "qtt": f32exact(1.e-6*(rs.random_sample(n3) - 0.5))}
        dzmin = float(np.min(g.dz[g.kstart:g.kend].astype(np.float64)))
        # 6.6 m/s: the largest three-level mean of w_qr these fields reach (w_max = 9.65 m/s on single levels)
        self.dt = {name: float(np.float32(cfl*dzmin/6.6)) for name, cfl in CFLS.items()}

    def digest(self):
        return refshim.digest(self.thl, self.qt, self.qr, self.nr, self.p, self.exn, self.rho, self.tend0["qrt"], self.tend0["nrt"], self.tend0["thlt"],
                              self.tend0["qtt"], np.array([self.dt["lo"], self.dt["hi"]]))

    def embed(self, a3, g, fill=777.):
        """The (ktot+2, jtot, itot) block inside a [kcells][jcells][icells] array of g's dtype; the horizontal ghost cells hold
        `fill`, which no kernel of this module may read into a result."""
        out = np.full(g.shape3, fill, dtype=g.np_dtype)
        out[:, g.jstart:g.jend, g.istart:g.iend] = a3
        return out

    def inputs(self, g, zero_tend=False):
        """Host arrays of grid g: the four fields, the four tendencies, rr_bot and the tables."""
        t = g.np_dtype
        h = {n: self.embed(np.asarray(getattr(self, n), dtype=t), g) for n in ("thl", "qt", "qr", "nr")}
        for n in OUT:
            h[n] = self.embed(np.zeros_like(self.tend0[n], dtype=t) if zero_tend else np.asarray(self.tend0[n], dtype=t), g)
        h["rr_bot"] = np.full(g.shape2, 555., dtype=t)
        for n in ("rho", "p", "exn"):
            h[n] = np.ascontiguousarray(getattr(self, n), dtype=t)
        return h


_cases = {}


def rain_case(shape):
    if shape not in _cases:
        _cases[shape] = RainCase(shape)
    return _cases[shape]


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.ref_micro_exec.argtypes = [ci, C.POINTER(Dims), ci, cd, cd] + [vp]*17; lib.ref_micro_exec.restype = None
    lib.ref_micro_cfl.argtypes = [ci, C.POINTER(Dims), vp, vp, vp, vp, cd]; lib.ref_micro_cfl.restype = cd
    lib.ref_limiter.argtypes = [ci, C.POINTER(Dims), vp, vp, cd]; lib.ref_limiter.restype = None


shim = refshim.Shim("micro", ["ref_micro_shim.cpp"], _bind, ref_sources=refshim.MASTER)


def ref_exec(shape, dtype, mask, dtname, zero_tend=False, gc=(1, 1, 1)):
    """The reference on the case: {qr, nr (clipped), qrt, nrt, thlt, qtt, rr_bot, ql, dr} as arrays of the grid's shape."""
    c, g = rain_case(shape), grid_of(shape, gc, dtype)
    h = c.inputs(g, zero_tend)
    d = dims_of(g)
    ql, dr = np.zeros(g.shape3, dtype=dtype), np.zeros(g.shape3, dtype=dtype)
    shim().ref_micro_exec(code(dtype), C.byref(d), mask, NC0, c.dt[dtname], *[cm.ptr(h[n]) for n in ("qr", "nr", "thl", "qt")], cm.ptr(ql),
                          *[cm.ptr(h[n]) for n in OUT], cm.ptr(h["rr_bot"]), cm.ptr(h["rho"]), cm.ptr(h["rho"]), cm.ptr(h["p"]), cm.ptr(h["exn"]),
                          cm.ptr(g.dz), cm.ptr(g.dzi), cm.ptr(dr))
    h["ql"], h["dr"] = ql, dr
    return h


def ref_cfl(shape, dtype, dtname):
    c, g = rain_case(shape), grid_of(shape, (1, 1, 1), dtype)
    h = c.inputs(g)
    d = dims_of(g)
    return shim().ref_micro_cfl(code(dtype), C.byref(d), cm.ptr(h["qr"]), cm.ptr(h["nr"]), cm.ptr(h["rho"]), cm.ptr(g.dzi), c.dt[dtname])


def ref_limiter(g, at, a, dt):
    at = at.copy()
    d = dims_of(g)
    shim().ref_limiter(code(g.np_dtype), C.byref(d), cm.ptr(at), cm.ptr(a), dt)
    return at


BREAKS = (0.35e-3, 0.9e-3)       # selfcollection_breakup's two jumps in dr


def near_break(dr, dtype):
    """Interior cells whose reference dr lies within a relative 1e-12 (fp64) / 1e-5 (fp32) of a jump of the breakup term."""
    tol = 1e-12 if np.dtype(dtype) == np.float64 else 1e-5
    dr = dr.astype(np.float64)
    return (np.abs(dr - BREAKS[0]) <= tol*BREAKS[0]) | (np.abs(dr - BREAKS[1]) <= tol*BREAKS[1])


def golden_runs():
    """(shape, mask name, mask, step name) of every run the golden file holds."""
    runs = []
    for shape in SHAPES:
        runs.append((shape, "all", ALL, "hi"))
    for shape in SMALL:
        for name, mask in PROCESSES.items():
            for dtname in (("lo", "hi") if mask == SEDI else ("hi",)):
                runs.append((shape, name, mask | CLIP, dtname))
    return runs


def run_key(shape, name, dtname, dtype):
    return "exec/%dx%dx%d/%s/%s/%s/" % (shape + (name, dtname, tag(dtype)))


def _compute_all():
    rec = {}
    for dt in cm.DTYPES:
        for shape, name, mask, dtname in golden_runs():
            r = ref_exec(shape, dt, mask, dtname, zero_tend=True)
            g = grid_of(shape, (1, 1, 1), dt)
            key = run_key(shape, name, dtname, dt)
            for n in stored(shape, mask):
                rec[key + n] = r[n][g.jstart:g.jend, g.istart:g.iend].copy() if n == "rr_bot" else r[n][g.interior].copy()
            near = near_break(r["dr"][g.interior], dt)
            rain = r["qr"][g.interior] > 1e-15
            assert not near.any(), "the seeded inputs put %d of %d rain cells on a jump of the breakup term: change the seed" % (near.sum(), rain.sum())
            rec[key + "excluded"] = np.flatnonzero(near).astype(np.int32)
        for shape in SHAPES:
            for dtname in CFLS:
                rec["cfl/%dx%dx%d/%s/%s" % (shape + (dtname, tag(dt)))] = np.array([ref_cfl(shape, dt, dtname)])
    for shape in SHAPES:
        rec["digest/%s" % rain_case(shape).key] = np.array(rain_case(shape).digest())
    return rec


GOLD = refshim.Golden("micro", _compute_all, "tests/test_micro_exec.py")
RECORD, golden, computed, exact_here, ref, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.exact_here, GOLD.ref, GOLD.record_if_asked


# ---- the device -------------------------------------------------------------------------------------------------------------
MARCH, CELL = 0, 1


class Dev:
    """The arrays of one (shape, gc, dtype) on a backend and the calls on them."""

    def __init__(self, be, shape, gc, dtype, zero_tend=False, host=None):
        from microhh_amd import capi
        self.capi = capi
        self.be, self.c, self.g = be, rain_case(shape), grid_of(shape, gc, dtype)
        self.h = self.c.inputs(self.g, zero_tend) if host is None else host
        self.G = be.grid(self.g)
        self.d = {n: be.arr(a) for n, a in self.h.items()}
        self.scratch = [be.arr(np.full(self.g.ncells, -9.e9, dtype=dtype)) for _ in range(4)]
        self.scratch_ptrs = (C.c_void_p*4)(*[be.ptr(a).value for a in self.scratch])
        self.work = be.zeros(16, np.float64)
        self.keep, self.cptr, self.count = M.counter(be)

    def exec(self, mask, dt, impl=None, nc0=NC0):
        be, d = self.be, self.d
        p = self.capi.MhhMicroParams(nc0, dt, mask)
        a = [be.ptr(d[n]) for n in ("qr", "nr", "thl", "qt", "qrt", "nrt", "thlt", "qtt", "rr_bot", "rho", "p", "exn")] + [self.scratch_ptrs, self.cptr, be.stream]
        if impl is None:
            rc = be.lib.mhh_micro_2mom_warm_exec(self.G, C.byref(p), *a)
        else:
            rc = be.lib.mhh_micro_2mom_warm_exec_impl(self.G, impl, C.byref(p), *a)
        self.capi.check(rc, be.lib)
        be.sync()
        g = self.g
        out = {n: be.host(d[n]).reshape(g.shape3) for n in ("qr", "nr") + OUT}
        out["rr_bot"] = be.host(d["rr_bot"]).reshape(g.shape2)
        return out

    def cfl(self, dt):
        be, d = self.be, self.d
        out = C.c_double(0)
        self.capi.check(be.lib.mhh_micro_2mom_warm_cfl(self.G, be.ptr(d["qr"]), be.ptr(d["nr"]), be.ptr(d["rho"]), dt, be.ptr(self.work), C.byref(out),
                                                       be.stream), be.lib)
        return out.value
