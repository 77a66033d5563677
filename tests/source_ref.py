"""Shared plumbing of the Source and Decay tests (tests/test_source_*.py): the grids, the source set and their reference results.

The reference is the reference's OWN source (src/source.cxx, src/decay.cxx) behind tests/cpp/ref_source_shim.cpp, compiled into a
temporary directory where the reference tree exists. Where it is absent the same cases read tests/golden/source_ref.npz, recorded
with MHH_RECORD_SOURCE_GOLDEN=1 python -m pytest tests/test_source_setup.py: per case the INPUTS (the initial tendencies and the
scalars, as bytes: multiples of 1/256), the ranges and norms of every source, the tendencies after Source::exec's loops run in
sequence, per cell the sum of the |terms| added (for the device tolerance), and the tendencies after Decay::exec.

The source set (sources_of) covers: a blob in the interior; blobs cut by the west/south/bottom and the east/north/top edges (where the
inclusive norm test against the exclusive emission loop shows); sigma < dx; sources wholly outside the domain, east (norm 0) and west
(the norm of the first plane); line_x, line_y and line_z with all three branches populated; two sources with two non-zero line
lengths (only the first gets the segment); swvmr on and off; two profile sources sharing a profile, one with its own, one whose
profile is zero everywhere; three overlapping sources on scalar 1 with sources on scalars 0 and 2 in the same launch.
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag  # noqa: F401
from microhh_amd.grid import Grid

F64, F32 = np.float64, np.float32
GC = (3, 3, 1)
# 24 x 20 x 16: more than one tile in every direction (tiles of 16 x 4 x 4); 37 x 19 x 11: ragged in all three
SHAPES = ((24, 20, 16), (37, 19, 11))
CASES = [(shape, dt) for shape in SHAPES for dt in (F64, F32)]
NSCALARS = 3
DX = DY = 100.
DT_SUB = 7.5
DECAY = {0: 600., 1: 2.5}            # scalar: timescale; 2.5 < DT_SUB: the dt branch of max(timescale, dt)


def case_id(case):
    return "%dx%dx%d-%s" % (case[0] + (tag(case[1]),))


def sizes(shape):
    return shape[0]*DX, shape[1]*DY, 75.*shape[2]


def grid_of(case, npy=1, rank=0):
    shape, dt = case
    xs, ys, zs = sizes(shape)
    # stretched: levels at multiples of 1/64 m
    z = np.round(zs*((np.arange(shape[2]) + 0.5)/shape[2])**1.3*64.)/64.
    return Grid(*shape, xs, ys, zs, order=2, igc=GC[0], jgc=GC[1], kgc=GC[2], z=z, dtype=dt, npy=npy, mpicoordy=rank)


def coords(g):
    """gd.x, gd.y of the one-rank grid (src/grid.cxx:252-262), [icells] and [jtot + 2 jgc]."""
    t = g.np_dtype
    px = ((np.arange(g.icells) - g.igc).astype(t)*t.type(g.dx)).astype(np.float64)
    py = ((np.arange(g.jtot + 2*g.jgc) - g.jgc).astype(t)*t.type(g.dy)).astype(np.float64)
    return (0.5*g.dx + px + 0.).astype(t), (0.5*g.dy + py + 0.).astype(t)


def rhoref_of(g):
    return np.ascontiguousarray(f32exact(1.2*np.exp(-g.z.astype(np.float64)/8000.)), dtype=g.np_dtype)


def profiles_of(g):
    """Three emission profiles [3][kcells]: a hump low down, a slab aloft, zero everywhere."""
    k = np.arange(g.kcells)
    p = np.zeros((3, g.kcells))
    p[0] = np.where((k >= g.kstart + 1) & (k < g.kstart + 6), f32exact(np.exp(-0.5*(k - g.kstart - 3.)**2)), 0.)
    p[1] = np.where((k >= g.kend - 4) & (k < g.kend), 0.25, 0.)
    return np.ascontiguousarray(p, dtype=g.np_dtype)


def sources_of(shape):
    X, Y, Z = sizes(shape)

    def s(scalar, x0, y0, z0, sx, sy, sz, strength=1., **kw):
        d = dict(scalar=scalar, x0=x0, y0=y0, z0=z0, sigma_x=sx, sigma_y=sy, sigma_z=sz, strength=strength)
        d.update(kw)
        return d
    return [
        s(0, 0.52*X, 0.48*Y, 0.4*Z, 150., 120., 60., 2.5),                                 # 0 interior blob
        s(0, 60., 40., 30., 100., 100., 80., 1.25, swvmr=True),                            # 1 cut by west/south/bottom
        s(0, X - 70., Y - 30., Z - 50., 110., 90., 100., 3.),                              # 2 cut by east/north/top
        s(1, 0.40*X, 0.50*Y, 0.5*Z, 150., 140., 120., 1.5),                                # 3, 4, 5 overlap on scalar 1
        s(1, 0.45*X, 0.55*Y, 0.45*Z, 130., 150., 110., 0.75, swvmr=True),
        s(1, 0.50*X, 0.45*Y, 0.55*Z, 160., 120., 100., 2.),
        s(0, 0.30*X + 13., 0.70*Y - 21., 0.6*Z, 20., 20., 12., 1.),                        # 6 sigma < dx: one or two cells
        s(2, X + 2000., 0.5*Y, 0.5*Z, 100., 100., 80., 1.),                                # 7 outside, east: empty, norm 0
        s(2, -500., 0.5*Y, 0.5*Z, 100., 100., 80., 1.),                                    # 8 outside, west: empty, the first plane's norm
        s(2, 0.25*X, 0.3*Y, 0.3*Z, 120., 100., 80., 4., line_x=0.4*X),                     # 9 line_x
        s(1, 0.7*X, 0.2*Y, 0.6*Z, 100., 110., 90., 3., line_y=0.5*Y, swvmr=True),          # 10 line_y
        s(2, 0.6*X, 0.7*Y, 0.2*Z, 110., 100., 60., 2., line_z=0.5*Z),                      # 11 line_z
        s(2, 0.3*X, 0.5*Y, 0.7*Z, 100., 100., 70., 1.5, line_x=300., line_y=400.),         # 12 two lengths: x gets the segment
        s(1, 0.2*X, 0.3*Y, 0.3*Z, 100., 100., 70., 1.5, line_y=350., line_z=0.3*Z),        # 13 two lengths: y gets the segment
        s(0, 0.7*X, 0.3*Y, 0., 140., 130., 1., 5., profile_index=0),                       # 14, 15 share profile 0
        s(1, 0.3*X, 0.7*Y, 0., 120., 150., 1., 2., profile_index=0, swvmr=True),
        s(2, 0.5*X, 0.5*Y, 0., 130., 130., 1., 3., profile_index=1),                       # 16 its own
        s(0, 0.5*X, 0.5*Y, 0., 130., 130., 1., 3., profile_index=2),                       # 17 a profile of zeroes: empty in z
    ]


def shape_id(case):
    return "%dx%dx%d" % case[0]


class Inputs:
    """The fields of one shape: the tendencies before and the scalars, multiples of 1/256 drawn as bytes (and stored as bytes)."""
    STORED = ("st0", "s", "cv")

    def __init__(self, case):
        self.case, self.g = case, grid_of(case)
        rs = np.random.RandomState(9100 + case[0][0] + 7*case[0][2])
        self.drawn = {k: rs.randint(0, 256, (NSCALARS,) + self.g.shape3).astype(np.uint8) for k in self.STORED}
        self.take({"%s/in/%s" % (shape_id(case), k): v for k, v in self.drawn.items()})

    def take(self, z):
        self.st0 = z["%s/in/st0" % shape_id(self.case)].astype(np.float64)/256.
        self.s = z["%s/in/s" % shape_id(self.case)].astype(np.float64)/256. + 1.
        # the couvreux scalar: multiples of 1/16 in [0, 4). A level's sums of s and of s*s (multiples of 1/256 below 16, at most 703 of
        # them) are then exact in a float, so the reference's own sequential TF sums carry no error and stay inside the bound
        self.cv = (z["%s/in/cv" % shape_id(self.case)] % 64).astype(np.float64)/16.

    def field(self, name, n):
        return np.array(getattr(self, name)[n], dtype=self.g.np_dtype, order="C", copy=True)


_inputs = {}


def inputs(case):
    key = case_id(case)
    if key not in _inputs:
        _inputs[key] = c = Inputs(case)
        if not GOLD.record and GOLD.golden() is not None:
            c.take(GOLD.golden())
    return _inputs[key]


# ---- the shim -------------------------------------------------------------------------------------------------------------------
class Desc(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("x0", "y0", "z0", "sigma_x", "sigma_y", "sigma_z", "line_x", "line_y", "line_z", "strength")] + \
               [("swvmr", C.c_int), ("use_profile", C.c_int)]


def desc_of(src):
    d = Desc()
    for n, _ in Desc._fields_[:10]:
        setattr(d, n, float(src.get(n, 1. if n == "strength" else 0.)))
    d.swvmr, d.use_profile = int(bool(src.get("swvmr", False))), int(src.get("profile_index") is not None)
    return d


def _bind(lib):
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    DP, SP, IP = C.POINTER(Dims), C.POINTER(Desc), C.POINTER(C.c_int)
    lib.ref_source_shape.argtypes = [ci, DP, SP, vp, vp, vp, vp, IP]; lib.ref_source_shape.restype = None
    lib.ref_source_norm.argtypes = [ci, DP, SP, vp, vp, vp, vp, cd, cd, vp, IP, vp]; lib.ref_source_norm.restype = cd
    lib.ref_source_emit.argtypes = [ci, DP, SP, vp, vp, vp, vp, vp, cd, IP]; lib.ref_source_emit.restype = None
    lib.ref_decay.argtypes = [ci, DP, vp, vp, cd, cd]; lib.ref_decay.restype = None


shim = refshim.Shim("source", ["ref_source_shim.cpp"], _bind, ref_sources=refshim.MASTER, stubs=True, defines=refshim.NC_FILL)


class Ref:
    """The reference on one grid (one rank): Source::create's ranges and norms, Source::exec's loops, Decay::exec."""

    def __init__(self, g, profiles=None, rhoref=None):
        self.g, self.lib, self.t = g, shim(), g.np_dtype
        assert g.npy == 1
        self.d = dims_of(g)
        self.x, self.y = coords(g)
        self.prof = profiles_of(g) if profiles is None else np.ascontiguousarray(profiles, dtype=self.t)
        self.rho = rhoref_of(g) if rhoref is None else np.ascontiguousarray(rhoref, dtype=self.t)

    def _prof(self, src):
        p = src.get("profile_index")
        return None if p is None else np.ascontiguousarray(self.prof[p])

    def ranges(self, src):
        r = (C.c_int*6)()
        self.lib.ref_source_shape(code(self.t), C.byref(self.d), C.byref(desc_of(src)), cm.ptr(self.x), cm.ptr(self.y), cm.ptr(self.g.z), cm.ptr(self._prof(src)), r)
        return np.array(r, dtype=np.int32)

    def norm(self, src, r):
        rr = (C.c_int*6)(*[int(v) for v in r])
        return self.lib.ref_source_norm(code(self.t), C.byref(self.d), C.byref(desc_of(src)), cm.ptr(self.x), cm.ptr(self.y), cm.ptr(self.g.z), cm.ptr(self.g.dz),
                                        self.g.dx, self.g.dy, cm.ptr(self._prof(src)), rr, cm.ptr(self.rho))

    def emit(self, src, st, r, norm, strength=None):
        d = desc_of(src)
        if strength is not None:
            d.strength = strength
        rr = (C.c_int*6)(*[int(v) for v in r])
        self.lib.ref_source_emit(code(self.t), C.byref(self.d), C.byref(d), cm.ptr(st), cm.ptr(self.x), cm.ptr(self.y), cm.ptr(self.g.z), cm.ptr(self._prof(src)), norm, rr)

    def exec(self, sources, st, absolute=False):
        """Source::create then Source::exec (:403-431) on the tendencies st[scalar] in place; (ranges [n][6], norms [n]).
        absolute: |strength|, for the sum of the |terms| per cell."""
        R, N = [], []
        for src in sources:
            r = self.ranges(src)
            n = self.norm(src, r)
            self.emit(src, st[src["scalar"]], r, n, abs(src.get("strength", 1.)) if absolute else None)
            R.append(r); N.append(n)
        return np.array(R, dtype=np.int32), np.array(N, dtype=np.float64)

    def decay(self, st, s, timescale, dt):
        self.lib.ref_decay(code(self.t), C.byref(self.d), cm.ptr(st), cm.ptr(s), timescale, dt)


NSTD = 1.25


def level_bound(g, a):
    """4 n 2^-53 S_k + ulp for the mean of a level: per level, S_k = sum |x| / n."""
    n = g.itot*g.jtot
    S = np.abs(a.astype(np.float64)).sum(axis=(1, 2))/n
    return 4.*n*2.**-53*S


def ref_couvreux(g, s, nstd=NSTD):
    """Decay::get_mask("couvreux") (src/decay.cxx:142-173) restated: its loops are written inside a member that needs Fields, Stats
    and tmp fields, so no shim call reaches them. Sequential TF sums in j, i order (cumsum is sequential), the quotients, the variance
    and the square root in TF, the field in TF; interpolate_2nd's double literals (src/grid.cxx:482-496). Returns mean, var
    [kcells], the field and the half-level field [shape3] (zero outside the interior, as a zeroed tmp field)."""
    t = g.np_dtype.type
    s = np.ascontiguousarray(s, dtype=t)
    out, mean, var = np.zeros(g.shape3, dtype=t), np.zeros(g.kcells, dtype=t), np.zeros(g.kcells, dtype=t)
    ijtot = t(g.itot*g.jtot)
    for k in range(g.kstart, g.kend):
        a = s[k, g.jstart:g.jend, g.istart:g.iend]
        m = t(np.cumsum(a.ravel(), dtype=t)[-1]/ijtot)
        v = t(np.cumsum((a*a).ravel(), dtype=t)[-1]/ijtot)
        v = t(v - m*m)
        mean[k], var[k] = m, v
        out[k, g.jstart:g.jend, g.istart:g.iend] = (a - m) - t(nstd)*np.sqrt(v)
    a = out.astype(np.float64)
    b = np.zeros_like(a); b[1:] = a[:-1]
    outh = 0.25*(0.5*a + 0.5*a) + 0.25*(0.5*a + 0.5*a) + 0.25*(0.5*b + 0.5*b) + 0.25*(0.5*b + 0.5*b)
    outh[0] = 0.25*(0.5*a[0] + 0.5*a[0]) + 0.25*(0.5*a[0] + 0.5*a[0])
    return mean, var, out, outh.astype(t)


def couvreux_excluded(g, fld):
    """Largest share of a level's cells whose |mask field| lies under the level's bound (they are left out of the mask comparison)."""
    it = g.interior
    b = level_bound(g, fld[it]) + np.spacing(np.abs(fld[it]).max(axis=(1, 2)).astype(np.float64))
    return float((np.abs(fld[it].astype(np.float64)) <= b[:, None, None]).mean(axis=(1, 2)).max())


def ref_case(case):
    g, inp = grid_of(case), inputs(case)
    R = Ref(g)
    src = sources_of(case[0])
    st = [inp.field("st0", n) for n in range(NSCALARS)]
    ranges, norms = R.exec(src, st)
    tot = [np.zeros(g.shape3, dtype=g.np_dtype) for n in range(NSCALARS)]
    R.exec(src, tot, absolute=True)
    tot = np.array(tot)[(slice(None),) + g.interior].astype(np.float64)
    # a bound, not a result: rounded up into a float, and never to zero
    small = np.where(tot > 0, float(np.finfo(np.float32).smallest_subnormal), 0.).astype(np.float32)
    out = {"ranges": ranges, "norms": norms, "st": np.array(st)[(slice(None),) + g.interior].copy(),
           "abs": np.maximum((tot*(1. + 2.**-20)).astype(np.float32), small)}
    dec = [inp.field("st0", n) for n in range(NSCALARS)]
    for n, ts in DECAY.items():
        R.decay(dec[n], inp.field("s", n), ts, DT_SUB)
    out["decay"] = np.array(dec)[(slice(None),) + g.interior].copy()
    if case[0] == SHAPES[1]:                  # the ragged grid carries the couvreux reference
        mean, var, fld, fldh = ref_couvreux(g, inp.field("cv", 0))
        out["cv_mean"], out["cv_var"] = mean, var
        out["cv_fld"], out["cv_fldh"] = fld[g.interior].copy(), fldh[g.kstart:g.kend+1, g.jstart:g.jend, g.istart:g.iend].copy()
        out["cv_mask"] = np.packbits(fld[g.interior] > 0)
        out["cv_maskh"] = np.packbits(fldh[g.kstart:g.kend+1, g.jstart:g.jend, g.istart:g.iend] > 0)
        out["cv_excluded"] = np.array([couvreux_excluded(g, fld)])
        assert out["cv_excluded"][0] <= 0.01
    return out


def _compute_all():
    rec = {}
    for case in CASES:
        for k, v in ref_case(case).items():
            rec["%s/%s" % (case_id(case), k)] = v
        for k, v in Inputs(case).drawn.items():
            rec["%s/in/%s" % (shape_id(case), k)] = v
    return rec


GOLD = refshim.Golden("source", _compute_all, "tests/test_source_setup.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(case, name, be=None):
    return GOLD.ref("%s/%s" % (case_id(case), name), be)
