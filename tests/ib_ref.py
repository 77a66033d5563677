"""Shared plumbing of the immersed-boundary tests (tests/test_ib_*.py): the terrain cases and their reference results.

The reference is the reference's OWN source (src/immersed_boundary.cxx) behind tests/cpp/ref_ib_shim.cpp, compiled into a temporary
directory where the reference tree exists. Where it is absent the same cases read tests/golden/ib_ref.npz, recorded with
MHH_RECORD_IB_GOLDEN=1 python -m pytest tests/test_ib_setup.py: per case the INPUTS (the terrain, one random field, the boundary
values, the sbot plane), the ghost-cell lists of every location, and the OUTPUTS of set_ghost_cells (the values at the ghost cells:
every other cell is the input), calc_mask, find_k_dem, calc_fluxes and interp2_dem; and the field and wall flux of the HotPath
test's grid. The terrain is the sine of the issue rounded to 1/64 m (so that an ulp of a host's sin and cos does not move it),
every draw is numpy's seeded legacy generator narrowed to values a float holds exactly, so the inputs are stored as floats. Where
the file exists the tests take the inputs FROM it; test_record_golden checks that this host draws the same.
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag
from microhh_amd import ib
from microhh_amd.grid import Grid

XSIZE, YSIZE, ZSIZE = 3200., 1600., 1200.
N_IDW = 5
VISC = 1e-5
DIRICHLET, NEUMANN, FLUX = 0, 1, 2
BCS = {"dirichlet": DIRICHLET, "neumann": NEUMANN, "flux": FLUX}
F64, F32 = np.float64, np.float32
# (itot, jtot, ktot), ghost cells, amplitude, dtype: 264 (w at 16x8x16) crosses a block of 256, 152 is no multiple of a wave;
# jtot = 1 is the shape of cases/ib_sine; the steep terrain makes neighbouring columns differ in k_dem (the side loops of calc_fluxes)
CASES = ([((16, 8, 16), gc, 0.15, dt) for gc in ((2, 2, 1), (3, 3, 1)) for dt in (F64, F32)] + [((12, 6, 12), (3, 3, 1), 0.15, F32)] +
         [((16, 1, 16), (3, 3, 1), 0.15, dt) for dt in (F64, F32)] + [((16, 8, 10), (3, 3, 1), 0.22, dt) for dt in (F64, F32)])
LOCS = ("u", "v", "w", "s")
INTS = ("i", "j", "k", "ip_i", "ip_j", "ip_k")
REALS = ("xb", "yb", "zb", "xi", "yi", "zi", "di", "ip_d", "c_idw", "c_idw_sum")
LISTS = INTS + REALS


def case_id(case):
    shape, gc, amp, dt = case
    return "%dx%dx%d-%d%d%d-A%02d-%s" % (shape + gc + (int(round(amp*100)), tag(dt)))


def grid_of(case):
    shape, gc, _, dt = case
    return Grid(shape[0], shape[1], shape[2], XSIZE, YSIZE, ZSIZE, order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dt)


def interior_dem(case):
    """The terrain on the (jtot, itot) columns, in double: multiples of 1/64 m."""
    shape, _, amp, _ = case
    return np.round(ib.sine_dem(shape[0], shape[1], XSIZE, YSIZE, ZSIZE, amp)*64.)/64.


def with_halos(g, a, dtype=None):
    """[jcells][icells] with the cyclic images (boundary_cyclic.exec_2d), jtot = 1 replicated."""
    return np.ascontiguousarray(np.pad(a, [(g.jgc, g.jgc), (g.igc, g.igc)], mode="wrap"), dtype=dtype or g.np_dtype)


def dem_of(case, g=None):
    return with_halos(g or grid_of(case), inputs(case).dem)


def axes(g):
    """{location: (x, y, z, dz)} as Immersed_boundary::create passes them (:810-864)."""
    c = ib.locations(g)
    return {"u": (c["xh"], c["y"], g.z, g.dz), "v": (c["x"], c["yh"], g.z, g.dz), "w": (c["x"], c["y"], g.zh, g.dzh), "s": (c["x"], c["y"], g.z, g.dz)}


class IbCase:
    """The inputs of one case: the terrain on the interior columns, ONE random field that serves every location (every cell drawn,
    the halos too), boundary values per list (the first nghost of `draw`), the plane of a spatial sbot. Drawn here; taken from the
    golden file where it exists."""
    STORED = ("dem", "field", "draw", "sbot_plane")

    def __init__(self, case):
        self.case, self.g = case, grid_of(case)
        shape = case[0]
        rs = np.random.RandomState(4400 + shape[0] + 7*shape[2] + 131*shape[1] + int(case[2]*100))
        self.dem = interior_dem(case)
        self.field = f32exact(300. + rs.random_sample(self.g.shape3))
        self.draw = f32exact(rs.random_sample(512) - 0.25)
        self.sbot_plane = f32exact(290. + 4.*rs.random_sample((shape[1], shape[0])))
        self.drawn = {k: getattr(self, k).astype(np.float32) for k in self.STORED}
        for k in self.STORED:
            assert np.array_equal(self.drawn[k].astype(np.float64), getattr(self, k)), k          # a float holds them exactly

    def take(self, z):
        """The inputs the golden file z holds."""
        for k in self.STORED:
            setattr(self, k, z["%s/in/%s" % (case_id(self.case), k)].astype(np.float64))

    @property
    def fld(self):
        f = np.ascontiguousarray(self.field, dtype=self.g.np_dtype)
        return {n: f for n in LOCS}

    def bv(self, nghost):
        return np.ascontiguousarray(self.draw[:nghost], dtype=self.g.np_dtype)


_cases = {}


def inputs(case):
    key = case_id(case)
    if key not in _cases:
        _cases[key] = c = IbCase(case)
        if not GOLD.record and GOLD.golden() is not None:
            c.take(GOLD.golden())
    return _cases[key]


# ---- the HotPath test's own grid: drycblles 16 x 8 x 16 (3200 x 3200 x 1200 m), the steep terrain ------------------------------
HOTPATH_GRID, HOTPATH_AMPLITUDE = (16, 8, 16), 0.22


def hotpath_grid(dtype):
    from microhh_amd.model import CASES
    return Grid(*HOTPATH_GRID, *CASES["drycblles"]["size"], order=2, igc=3, jgc=3, kgc=1, dtype=dtype)


def hotpath_dem():
    from microhh_amd.model import CASES
    if not GOLD.record and GOLD.golden() is not None:
        return GOLD.golden()["hotpath/in/dem"].astype(np.float64)
    return np.round(ib.sine_dem(HOTPATH_GRID[0], HOTPATH_GRID[1], *CASES["drycblles"]["size"], HOTPATH_AMPLITUDE)*64.)/64.


def hotpath_th():
    """th of the HotPath test [kcells][jcells][icells] in double, the horizontal halos the cyclic images: from the golden file where
    it exists."""
    if not GOLD.record and GOLD.golden() is not None:
        return GOLD.golden()["hotpath/in/th"].astype(np.float64)
    g = hotpath_grid(np.float64)
    a = f32exact(300. + np.random.RandomState(7722).random_sample((g.kcells, g.jmax, g.imax)))
    return np.pad(a, [(0, 0), (g.jgc, g.jgc), (g.igc, g.igc)], mode="wrap")


def ref_hotpath(dtype):
    g = hotpath_grid(dtype)
    kd = ref_k_dem(g, with_halos(g, hotpath_dem()))
    return ref_fluxes(g, k_dem_with_halos(g, kd), np.ascontiguousarray(hotpath_th(), dtype=g.np_dtype))


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    DP = C.POINTER(Dims)
    lib.ref_ib_message.argtypes = []; lib.ref_ib_message.restype = C.c_char_p
    lib.ref_ib_ghost.argtypes = [ci, DP, vp, vp, vp, vp, vp, ci, cd, cd, ci, ci, ci]; lib.ref_ib_ghost.restype = ci
    lib.ref_ib_ghost_get.argtypes = [ci, C.POINTER(vp), C.POINTER(vp)]; lib.ref_ib_ghost_get.restype = None
    lib.ref_ib_interp.argtypes = [ci, DP, ci, vp, vp, vp, vp, vp, cd, cd, ci, ci, vp]; lib.ref_ib_interp.restype = ci
    lib.ref_ib_set_ghost_cells.argtypes = [ci, DP] + [vp]*11 + [ci, cd, ci, ci]; lib.ref_ib_set_ghost_cells.restype = None
    lib.ref_ib_mask.argtypes = [ci, DP, vp, vp, vp, vp, vp]; lib.ref_ib_mask.restype = None
    lib.ref_ib_k_dem.argtypes = [ci, DP, vp, vp, vp]; lib.ref_ib_k_dem.restype = None
    lib.ref_ib_fluxes.argtypes = [ci, DP, vp, vp, vp, cd, cd, vp, cd, cd, vp, cd]; lib.ref_ib_fluxes.restype = None


shim = refshim.Shim("ib", ["ref_ib_shim.cpp"], _bind, stubs=True, defines=refshim.NC_FILL)


class RefThrows(RuntimeError):
    """What the reference threw."""


def ref_ghost(g, dem, x, y, z, dz, bc, n_idw=N_IDW, offsets=None):
    """calc_ghost_cells of the reference for one location: {name: array}, "nghost"; RefThrows with its text where it throws."""
    lib, t = shim(), g.np_dtype
    ox, oy = ib.mpi_offsets(g) if offsets is None else offsets
    d = dims_of(g)
    arrs = [np.ascontiguousarray(a, dtype=t) for a in (dem, x, y, z, dz)]
    ng = lib.ref_ib_ghost(code(t), C.byref(d), *[cm.ptr(a) for a in arrs], bc, g.dx, g.dy, n_idw, ox, oy)
    if ng < 0:
        raise RefThrows(lib.ref_ib_message().decode())
    out = {k: np.zeros(ng if not k.startswith("ip_") else (ng, n_idw), dtype=np.int32) for k in INTS}
    out.update({k: np.zeros((ng, n_idw) if k in ("ip_d", "c_idw") else ng, dtype=t) for k in REALS})
    ints = (C.c_void_p*6)(*[out[k].ctypes.data for k in INTS])
    reals = (C.c_void_p*10)(*[out[k].ctypes.data for k in REALS])
    lib.ref_ib_ghost_get(code(t), ints, reals)
    out["nghost"] = ng
    return out


def ref_set(g, fld, bv, gh, bc, visc=VISC, n_idw=N_IDW):
    """set_ghost_cells of the reference on a copy of fld."""
    out = np.ascontiguousarray(fld).copy()
    d = dims_of(g)
    a = [np.ascontiguousarray(gh[k]) for k in ("c_idw", "c_idw_sum", "di", "i", "j", "k", "ip_i", "ip_j", "ip_k")]
    bv = np.ascontiguousarray(bv, dtype=g.np_dtype)
    shim().ref_ib_set_ghost_cells(code(g.np_dtype), C.byref(d), cm.ptr(out), cm.ptr(bv), *[cm.ptr(x) for x in a], bc, visc, gh["nghost"], n_idw)
    return out


def ref_mask(g, dem):
    mask, maskh = np.zeros(g.shape3, dtype=g.np_dtype), np.zeros(g.shape3, dtype=g.np_dtype)
    d = dims_of(g)
    shim().ref_ib_mask(code(g.np_dtype), C.byref(d), cm.ptr(mask), cm.ptr(maskh), cm.ptr(dem), cm.ptr(g.z), cm.ptr(g.zh))
    return mask, maskh


def ref_k_dem(g, dem):
    out = np.zeros(g.shape2, dtype=np.uint32)
    d = dims_of(g)
    shim().ref_ib_k_dem(code(g.np_dtype), C.byref(d), cm.ptr(out), cm.ptr(dem), cm.ptr(g.z))
    return out


def inverse(g, d):
    """gd.dxi = 1./gd.dx (src/grid.cxx:244): a double quotient of the narrowed spacing, narrowed."""
    t = g.np_dtype.type
    return float(t(1./float(t(d))))


def ref_fluxes(g, k_dem, s, svisc=VISC):
    """calc_fluxes: the interior of flux_bot. k_dem with filled halos."""
    out = np.zeros(g.shape2, dtype=g.np_dtype)
    d = dims_of(g)
    k_dem = np.ascontiguousarray(k_dem, dtype=np.uint32)
    shim().ref_ib_fluxes(code(g.np_dtype), C.byref(d), cm.ptr(out), cm.ptr(k_dem), cm.ptr(np.ascontiguousarray(s)), g.dx, g.dy, cm.ptr(g.dz),
                         inverse(g, g.dx), inverse(g, g.dy), cm.ptr(g.dzhi), svisc)
    return out[g.jstart:g.jend, g.istart:g.iend].copy()


def ref_interp(g, plane, xp, yp, offsets=None):
    lib, t = shim(), g.np_dtype
    ox, oy = ib.mpi_offsets(g) if offsets is None else offsets
    c = ib.locations(g)
    d = dims_of(g)
    plane, xp, yp = (np.ascontiguousarray(a, dtype=t) for a in (plane, xp, yp))
    out = np.zeros(xp.size, dtype=t)
    if lib.ref_ib_interp(code(t), C.byref(d), xp.size, cm.ptr(xp), cm.ptr(yp), cm.ptr(c["x"]), cm.ptr(c["y"]), cm.ptr(plane), g.dx, g.dy, ox, oy, cm.ptr(out)) < 0:
        raise RefThrows(lib.ref_ib_message().decode())
    return out


def cells_of(g, gh):
    return gh["i"].astype(np.int64) + gh["j"].astype(np.int64)*g.icells + gh["k"].astype(np.int64)*g.ijcells


def k_dem_with_halos(g, kd):
    return with_halos(g, kd[g.jstart:g.jend, g.istart:g.iend], dtype=np.uint32)


def ref_case(case):
    """Everything the reference gives on one case: {key: array}."""
    g, dem, inp = grid_of(case), dem_of(case), inputs(case)
    out = {}
    lists = {}
    for loc, ax in axes(g).items():
        lists[loc] = ref_ghost(g, dem, *ax, DIRICHLET)
    for name, bc in (("s_neumann", NEUMANN), ("s_flux", FLUX)):
        lists[name] = ref_ghost(g, dem, *axes(g)["s"], bc)
        for k in LISTS:              # the boundary type decides the weights alone
            assert k in ("c_idw", "c_idw_sum") or np.array_equal(lists[name][k], lists["s"][k]), (name, k)
    for loc, gh in lists.items():
        assert gh["nghost"] > 0 and gh["ip_k"].max() < g.kcells and gh["k"].max() + 5 < g.kcells       # the reference alone stays inside its arrays
        for k in (LISTS if loc in LOCS else ("c_idw", "c_idw_sum")):
            out["%s/%s" % (loc, k)] = gh[k]
    for loc, name, bc in (("u", "u", DIRICHLET), ("v", "v", DIRICHLET), ("w", "w", DIRICHLET), ("s", "s", DIRICHLET), ("s", "s_neumann", NEUMANN), ("s", "s_flux", FLUX)):
        gh = lists[name]
        after = ref_set(g, inp.fld[loc], inp.bv(gh["nghost"]), gh, bc)
        cells = cells_of(g, gh)
        outside = np.ones(g.ncells, dtype=bool); outside[cells] = False
        assert np.array_equal(after.reshape(-1)[outside], inp.fld[loc].reshape(-1)[outside])
        out["set/%s" % name] = after.reshape(-1)[cells].copy()
    mask, maskh = ref_mask(g, dem)
    out["mask"], out["maskh"] = mask[g.interior].astype(np.uint8), maskh[g.interior].astype(np.uint8)
    kd = ref_k_dem(g, dem)
    out["k_dem"] = kd[g.jstart:g.jend, g.istart:g.iend].copy()
    out["flux"] = ref_fluxes(g, k_dem_with_halos(g, kd), inp.fld["s"])
    out["interp"] = ref_interp(g, with_halos(g, inp.sbot_plane), lists["s"]["xb"], lists["s"]["yb"])
    return out


def _compute_all():
    rec = {}
    for case in CASES:
        for k, v in ref_case(case).items():
            rec["%s/%s" % (case_id(case), k)] = v
        for k, v in inputs(case).drawn.items():
            rec["%s/in/%s" % (case_id(case), k)] = v
    th = hotpath_th()
    rec["hotpath/in/th"], rec["hotpath/in/dem"] = th.astype(np.float32), hotpath_dem().astype(np.float32)
    assert np.array_equal(rec["hotpath/in/dem"].astype(np.float64), hotpath_dem())
    assert np.array_equal(rec["hotpath/in/th"].astype(np.float64), th)
    for dt in (F64, F32):
        rec["hotpath/%s/flux" % tag(dt)] = ref_hotpath(dt)
    return rec


GOLD = refshim.Golden("ib", _compute_all, "tests/test_ib_setup.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(case, name, be=None):
    """A reference result by name (Golden.ref)."""
    return GOLD.ref("%s/%s" % (case_id(case), name), be)


def ref_lists(case, name, be=None):
    """One list as ref_ghost gives it: name in u, v, w, s, s_neumann, s_flux."""
    base = name if name in LOCS else "s"
    gh = {k: ref(case, "%s/%s" % (name if (name in LOCS or k in ("c_idw", "c_idw_sum")) else base, k), be) for k in LISTS}
    gh["nghost"] = int(gh["i"].size)
    return gh
