"""Shared plumbing of the moist-thermodynamics tests (tests/test_moist_*.py): the seeded cases and their reference results.

The reference is the reference's OWN header (thermo_moist_functions.h) behind tests/cpp/ref_moist_shim.cpp, compiled into a
temporary directory where the reference tree exists. Where it is absent (the GPU box) the same cases read
tests/golden/moist_ref.npz, recorded with MHH_RECORD_MOIST_GOLDEN=1 python -m pytest tests/test_moist_cell.py: the reference outputs
of every case and what the cases take from the reference's C library (the Exner tables). The inputs are not stored: every draw is
numpy's seeded legacy generator, narrowed to values a float holds exactly, and everything derived from a draw uses + - * / only, so
they are the same numbers on every host; the file holds their digest per case.
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag
from microhh_amd.grid import Grid
from microhh_amd.thermo import bomex_profiles, bomex_synthetic

T0 = 273.15
PBOT = 101500.
NPOINT = 2048

# (itot, jtot, ktot); the last one runs with 8 levels per chunk, so that several chunks meet
SHAPES = [(70, 9, 10), (17, 9, 8), (20, 1, 12), (130, 6, 40)]
GCS = [(1, 1, 1), (3, 3, 1)]


def exn_like(p):
    """An Exner-like function of p from + - * / alone (the cubic Taylor polynomial of (p/p0)^(Rd/cp) at p0): the same bits on
    every host. sat_adjust takes exn as an input of its own, so the point sets need no more than a realistic value."""
    a = 287.04/1005.
    x = p/1.e5 - 1.
    return 1. + a*x*(1. + (a - 1.)/2.*x*(1. + (a - 2.)/3.*x))


# ---- the point sets ---------------------------------------------------------------------------------------------------------
def point_set(name):
    """float64 master inputs {thl, qt, p, exn} of the warm or the mixed set, every value float32-exact."""
    rs = np.random.RandomState(20260 + len(name))
    if name == "warm":
        p = f32exact(70000. + 32000.*rs.random_sample(NPOINT))
        exn = f32exact(exn_like(p))
        thl = f32exact((T0 + 0.6 + 30.*rs.random_sample(NPOINT)) / exn)
    else:
        p = f32exact(55000. + 47000.*rs.random_sample(NPOINT))
        exn = f32exact(exn_like(p))
        thl = f32exact(235. + 85.*rs.random_sample(NPOINT))
    qt = f32exact(0.025*rs.random_sample(NPOINT))
    return {"thl": thl, "qt": qt, "p": p, "exn": exn}


def search_nonconv(dtype, want=6):
    """Inputs on which the reference throws (about 1 in 1e4 of thl in [200, 330], qt < 0.04), each followed by a converging
    neighbour: found by the recording step, kept in the golden file."""
    lib = shim()
    rs = np.random.RandomState(99)
    found = []
    for _ in range(40):
        n = 50000
        p = f32exact(55000. + 47000.*rs.random_sample(n)); exn = f32exact(exn_like(p))
        thl = f32exact(200. + 130.*rs.random_sample(n)); qt = f32exact(0.04*rs.random_sample(n))
        out = ref_sat_adjust(lib, dtype, {"thl": thl, "qt": qt, "p": p, "exn": exn})
        bad = np.flatnonzero(out["threw"])
        for c in bad:
            if c + 1 < n and not out["threw"][c+1]:
                found.append((thl[c], qt[c], p[c], exn[c])); found.append((thl[c+1], qt[c+1], p[c+1], exn[c+1]))
            if len(found) >= 2*want:
                break
        if len(found) >= 2*want:
            break
    a = np.array(found[:2*want])
    return {"thl": a[:, 0].copy(), "qt": a[:, 1].copy(), "p": a[:, 2].copy(), "exn": a[:, 3].copy()}


# ---- the 3-D cases ----------------------------------------------------------------------------------------------------------
def grid_of(shape, gc, dtype):
    return Grid(shape[0], shape[1], shape[2], 6400., 6400., 3000., order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype)


class FieldCase:
    """Warm inputs of one shape: thl, qt and a non-zero wt on ktot + 2 levels of jtot x itot columns (the same for every ghost
    layout), and the half- and full-level tables that need no C library (pressure, thvref)."""

    def __init__(self, shape):
        self.shape = shape
        self.key = "%dx%dx%d" % shape
        itot, jtot, ktot = shape
        rs = np.random.RandomState(4000 + itot + 7*ktot)
        g = grid_of(shape, (1, 1, 1), np.float64)
        n3 = (ktot + 2, jtot, itot)
        z = g.z[:, None, None]
        self.thl = f32exact(292. + 0.005*z + (rs.random_sample(n3) - 0.5))
        self.qt = f32exact(0.02*rs.random_sample(n3))
        self.wt = f32exact(1.e-2*(rs.random_sample(n3) - 0.5))
        s = 1. - g.z/44000.; sh = 1. - g.zh/44000.
        self.pref = f32exact(PBOT*s*s*s*s*s); self.prefh = f32exact(PBOT*sh*sh*sh*sh*sh)
        self.thvref = f32exact(300. + 0.004*g.z); self.thvrefh = f32exact(300. + 0.004*g.zh)

    def digest(self):
        return refshim.digest(self.thl, self.qt, self.wt, self.pref, self.prefh, self.thvref, self.thvrefh)

    def embed(self, a3, g, fill=777.):
        """The (ktot+2, jtot, itot) block inside a [kcells][jcells][icells] array of g's dtype; the horizontal ghost cells hold
        `fill`, which no kernel of this module may read into a result."""
        out = np.full(g.shape3, fill, dtype=g.np_dtype)
        out[:, g.jstart:g.jend, g.istart:g.iend] = a3
        return out


_cases = {}


def field_case(shape):
    if shape not in _cases:
        _cases[shape] = FieldCase(shape)
    return _cases[shape]


# ---- base-state profiles ----------------------------------------------------------------------------------------------------
BASE_CASES = ["bomex64", "stretched", "saturated"]


def base_case(name, dtype):
    """(grid, thl0, qt0) of a base-state case: [kcells] profiles in the dtype with the interior set (float32-exact)."""
    if name == "stretched":
        s = (np.arange(40) + 0.5)/40.
        g = Grid(4, 4, 40, 6400., 6400., 3000., order=2, igc=1, jgc=1, kgc=1, dtype=dtype, z=f32exact(3000.*(s + 0.6*s*s)/1.6))
    else:
        g = Grid(4, 4, 64, 6400., 6400., 3000., order=2, igc=1, jgc=1, kgc=1, dtype=dtype)
    z = g.z[g.kstart:g.kend].astype(np.float64)
    thl, qt = bomex_profiles(z)
    if name == "saturated":
        qt = qt + np.where((z > 600.) & (z < 1400.), 3.e-3, 0.)      # a supersaturated layer: sat_adjust inside the recurrence
    thl0, qt0 = np.zeros(g.kcells, dtype=dtype), np.zeros(g.kcells, dtype=dtype)
    thl0[g.kstart:g.kend] = f32exact(thl); qt0[g.kstart:g.kend] = f32exact(qt)
    return g, thl0, qt0


BASE_OUT = ["pref", "prefh", "rhoref", "rhorefh", "thvref", "thvrefh", "exnref", "exnrefh"]


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci = C.c_void_p, C.c_int
    lib.ref_moist_sat_adjust.argtypes = [ci, C.c_longlong] + [vp]*9; lib.ref_moist_sat_adjust.restype = ci
    lib.ref_moist_exner.argtypes = [ci, ci, vp, vp]; lib.ref_moist_exner.restype = None
    lib.ref_moist_tend.argtypes = [ci, C.POINTER(Dims)] + [vp]*5; lib.ref_moist_tend.restype = ci
    lib.ref_moist_fields.argtypes = [ci, C.POINTER(Dims)] + [vp]*9; lib.ref_moist_fields.restype = None
    lib.ref_moist_N2.argtypes = [ci, C.POINTER(Dims)] + [vp]*4; lib.ref_moist_N2.restype = None
    lib.ref_moist_surf_hooks.argtypes = [ci, ci] + [vp]*6 + [C.c_double]*2 + [vp]*4; lib.ref_moist_surf_hooks.restype = None
    lib.ref_moist_base_state.argtypes = [ci, ci, ci, ci, vp, vp, C.c_double] + [vp]*13; lib.ref_moist_base_state.restype = None


shim = refshim.Shim("moist", ["ref_moist_shim.cpp"], _bind)


def typed(master, dtype):
    return {k: np.ascontiguousarray(v, dtype=dtype) for k, v in master.items()}


def ref_sat_adjust(lib, dtype, master):
    inp = typed(master, dtype)
    n = inp["thl"].size
    out = {k: np.zeros(n, dtype=dtype) for k in ("ql", "qi", "t", "qs")}
    out["threw"] = np.zeros(n, dtype=np.int32)
    lib.ref_moist_sat_adjust(code(dtype), n, *[cm.ptr(inp[k]) for k in ("thl", "qt", "p", "exn")],
                             *[cm.ptr(out[k]) for k in ("ql", "qi", "t", "qs", "threw")])
    return out


def ref_exner(lib, dtype, p):
    p = np.ascontiguousarray(p, dtype=dtype); out = np.zeros_like(p)
    lib.ref_moist_exner(code(dtype), p.size, cm.ptr(p), cm.ptr(out))
    return out


def _compute_all():
    """Every reference array of every case, by key, from the shim."""
    lib = shim()
    rec = {}
    for dt in cm.DTYPES:
        t = tag(dt)
        for name in ("warm", "mixed"):
            out = ref_sat_adjust(lib, dt, point_set(name))
            assert not out["threw"].any(), "the %s set must converge on the reference" % name
            for k in ("ql", "qi", "t", "qs"):
                rec["point/%s/%s/%s" % (name, t, k)] = out[k]
        if RECORD or golden() is None:
            bad = search_nonconv(dt)
        else:                       # the search is the recording step's; afterwards its finds are read back
            bad = {k: golden()["nonconv/%s/in/%s" % (t, k)] for k in ("thl", "qt", "p", "exn")}
        out = ref_sat_adjust(lib, dt, bad)
        assert out["threw"][0::2].all() and not out["threw"][1::2].any()
        for k, v in bad.items():
            rec["nonconv/%s/in/%s" % (t, k)] = v
        for k in ("ql", "qi", "t", "qs"):
            rec["nonconv/%s/%s" % (t, k)] = out[k]
        for shape in SHAPES:
            c = field_case(shape)
            g = grid_of(shape, (1, 1, 1), dt)
            d = dims_of(g)
            thl, qt, wt = (np.ascontiguousarray(a, dtype=dt) for a in (c.thl, c.qt, c.wt))
            prefh, thvrefh, pref, thvref = (np.ascontiguousarray(a, dtype=dt) for a in (c.prefh, c.thvrefh, c.pref, c.thvref))
            key = "field/%s/%s/" % (c.key, t)
            rec[key + "exnrefh"] = ref_exner(lib, dt, prefh); rec[key + "exnref"] = ref_exner(lib, dt, pref)
            # (1,1,1) ghost cells: embed with the horizontal ghosts set, run, keep the interior
            e = {n: c.embed(a, g) for n, a in (("thl", thl), ("qt", qt), ("wt", wt))}
            nsat = lib.ref_moist_tend(code(dt), C.byref(d), cm.ptr(e["wt"]), cm.ptr(e["thl"]), cm.ptr(e["qt"]), cm.ptr(prefh), cm.ptr(thvrefh))
            rec[key + "wt"] = e["wt"][g.interior].copy()
            rec[key + "nsat"] = np.array([nsat])
            if shape in SHAPES[1:3]:
                o = {n: np.zeros(g.shape3, dtype=dt) for n in ("b", "ql", "qi", "T")}
                lib.ref_moist_fields(code(dt), C.byref(d), cm.ptr(e["thl"]), cm.ptr(e["qt"]), cm.ptr(pref), cm.ptr(rec[key + "exnref"]), cm.ptr(thvref),
                                     *[cm.ptr(o[n]) for n in ("b", "ql", "qi", "T")])
                for n in ("ql", "qi", "T"):
                    rec[key + n] = o[n][g.interior].copy()
                rec[key + "b"] = o["b"][:, g.jstart:g.jend, g.istart:g.iend].copy()
                n2 = np.zeros(g.shape3, dtype=dt)
                lib.ref_moist_N2(code(dt), C.byref(d), cm.ptr(n2), cm.ptr(e["thl"]), cm.ptr(g.dzi), cm.ptr(thvref))
                rec[key + "N2"] = n2[g.interior].copy()
        for name in BASE_CASES:
            g, thl0, qt0 = base_case(name, dt)
            o = {n: np.zeros(g.kcells, dtype=dt) for n in BASE_OUT}
            lib.ref_moist_base_state(code(dt), g.kstart, g.kend, 1, cm.ptr(thl0), cm.ptr(qt0), PBOT,
                                     cm.ptr(g.z), cm.ptr(g.zh), cm.ptr(g.dz), cm.ptr(g.dzh), cm.ptr(g.dzhi),
                                     *[cm.ptr(o[n]) for n in BASE_OUT])
            for n in BASE_OUT:
                rec["base/%s/%s/%s" % (name, t, n)] = o[n]
            rec["base/%s/%s/thl0" % (name, t)] = thl0; rec["base/%s/%s/qt0" % (name, t)] = qt0
    rec["bomex/nsat"] = np.array([bomex_reference()[1], bomex_reference()[2]])
    for shape in SHAPES:
        rec["digest/field/%s" % field_case(shape).key] = np.array(field_case(shape).digest())
    for name in ("warm", "mixed"):
        rec["digest/point/%s" % name] = np.array(refshim.digest(*[point_set(name)[k] for k in ("thl", "qt", "p", "exn")]))
    return rec


BOMEX_SHAPE = (64, 8, 64)
_bomex = {}


def bomex_inputs(dtype, tables):
    """(grid, thl, qt, wt) of the synthetic BOMEX field at 64 x 8 x 64 and the three half-level tables from `tables`, a function of
    the profile's name (the base state of the bomex64 case)."""
    g = grid_of(BOMEX_SHAPE, (3, 3, 1), dtype)
    thl, qt = bomex_synthetic(g, seed=1)
    wt = np.zeros(g.shape3, dtype=dtype)
    tab = None if tables is None else [np.ascontiguousarray(tables(n), dtype=dtype) for n in ("prefh", "exnrefh", "thvrefh")]
    return g, thl, qt, wt, tab


def bomex_reference():
    """(wt, saturated w-level cells, w-level cells, the half-level tables) of the reference on the synthetic BOMEX field, fp64; needs the shim."""
    if "r" not in _bomex:
        lib = shim()
        bs = {}
        g0, thl0, qt0 = base_case("bomex64", np.float64)
        o = {n: np.zeros(g0.kcells) for n in BASE_OUT}
        lib.ref_moist_base_state(0, g0.kstart, g0.kend, 1, cm.ptr(thl0), cm.ptr(qt0), PBOT, cm.ptr(g0.z), cm.ptr(g0.zh), cm.ptr(g0.dz),
                                 cm.ptr(g0.dzh), cm.ptr(g0.dzhi), *[cm.ptr(o[n]) for n in BASE_OUT])
        bs.update(o)
        g, thl, qt, wt, tab = bomex_inputs(np.float64, lambda n: bs[n])
        assert (thl[g.kstart:g.kend]*tab[1][g.kstart:g.kend, None, None] >= T0 + 10.).all()      # warm everywhere
        d = dims_of(g)
        nsat = lib.ref_moist_tend(0, C.byref(d), cm.ptr(wt), cm.ptr(thl), cm.ptr(qt), cm.ptr(tab[0]), cm.ptr(tab[2]))
        _bomex["r"] = (wt, nsat, g.imax*g.jmax*(g.kmax - 1), tab)
    return _bomex["r"]


GOLD = refshim.Golden("moist", _compute_all, "tests/test_moist_cell.py")       # its first test records: it holds computed() against the file
RECORD, golden, computed, exact_here, ref = GOLD.record, GOLD.golden, GOLD.computed, GOLD.exact_here, GOLD.ref


def rel(got, want):
    """max |got - want| / max |want| of one array, in float64."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.max(np.abs(want))
    return float(np.max(np.abs(got - want)) / den) if den > 0 else float(np.max(np.abs(got)))


# ---- the device -------------------------------------------------------------------------------------------------------------
def counter(be):
    """A zeroed int counter in device memory and a function that reads it."""
    if be.name == "emul":
        c = np.zeros(1, dtype=np.int32)
        return c, cm.ptr(c), (lambda: int(c[0]))
    c = be.torch.zeros(1, dtype=be.torch.int32, device=be.dev)
    return c, C.c_void_p(c.data_ptr()), (lambda: int(c.cpu()[0]))


def dev_sat_adjust(be, dtype, master, outputs=("ql", "qi", "t", "qs")):
    """mhh_thermo_moist_sat_adjust on the inputs `master`; returns the outputs asked for and the counter of non-converged cells."""
    from microhh_amd import capi
    inp = typed(master, dtype)
    n = inp["thl"].size
    d = {k: be.arr(v) for k, v in inp.items()}
    o = {k: be.zeros(n, dtype) for k in outputs}
    keep, cptr, read = counter(be)
    capi.check(be.lib.mhh_thermo_moist_sat_adjust(code(dtype), n, *[be.ptr(d[k]) for k in ("thl", "qt", "p", "exn")],
                                                  *[be.ptr(o.get(k)) for k in ("ql", "qi", "t", "qs")], cptr, be.stream), be.lib)
    be.sync()
    return {k: be.host(v) for k, v in o.items()}, read()
