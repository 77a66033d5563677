"""Shared plumbing of the Boundary_outflow tests (tests/test_outflow_*.py): the cases, their inputs and their reference results.

The reference is the reference's OWN source (src/boundary_outflow.cxx) behind tests/cpp/ref_outflow_shim.cpp, compiled into a
temporary directory where the reference tree exists: its loops in the order of Boundary_outflow<TF>::exec, with gd.kgc in the place
of jgc as there, on a rank that owns the edges of a mask. Where the tree is absent, and on the GPU, the same cases read
tests/golden/outflow_ref.npz, recorded with MHH_RECORD_OUTFLOW_GOLDEN=1 python -m pytest tests/test_outflow_exec.py: per case the
whole fields after the fill. The inputs are not stored: numpy's seeded legacy generator draws the same doubles on every host. They
carry full mantissas, so that a contracted or re-ordered inflow rule shows in the last bit.
"""
import collections
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import code, have_reference, tag  # noqa: F401
from microhh_amd.grid import Grid, moser_z

F64, F32 = np.float64, np.float32
WEST, EAST, SOUTH, NORTH = 1, 2, 4, 8
ALL = WEST | EAST | SOUTH | NORTH
OUT, IN = 0, 1

# shape, gc, dtype, dirs (West, East, South, North), the edge mask, the grid's order, the number of fields
Case = collections.namedtuple("Case", "shape gc dtype dirs mask order nf")

JAENSCHWALDE = (IN, OUT, OUT, OUT)
# the smallest shapes at which each hazard exists: kgc = 1, 2, 3 of jgc = 3 rows (the untouched rows keep their values); the advec_2
# layout; igc = 16 at the limit itot == igc and above it; a ragged grid
LAYOUTS = [((8, 6, 5), (3, 3, 1)), ((8, 6, 5), (3, 3, 2)), ((8, 6, 5), (3, 3, 3)), ((8, 6, 5), (1, 1, 1)),
           ((16, 6, 5), (16, 3, 1)), ((24, 6, 5), (16, 3, 1)), ((37, 5, 3), (3, 3, 1))]
COMBO_LAYOUT = LAYOUTS[1]
COMBOS = [tuple((n >> e) & 1 for e in range(4)) for n in range(16)]
MASKS = (WEST, SOUTH, 0)
FOURTH_LAYOUT = ((8, 6, 8), (3, 3, 3))


def layout_cases(dt):
    return [Case(s, gc, dt, JAENSCHWALDE, ALL, 2, 1) for s, gc in LAYOUTS]


def combo_cases(dt):
    return [Case(*COMBO_LAYOUT, dt, dirs, ALL, 2, 1) for dirs in COMBOS]


def mask_cases(dt):
    return [Case(*COMBO_LAYOUT, dt, (IN, IN, IN, IN), m, 2, 1) for m in MASKS]


def several_case(dt):
    return Case(*COMBO_LAYOUT, dt, (IN, OUT, OUT, IN), ALL, 2, 3)


def fourth_cases(dt):
    return [Case(*FOURTH_LAYOUT, dt, JAENSCHWALDE, m, 4, 1) for m in (ALL, WEST)]


def all_cases():
    out = []
    for dt in (F64, F32):
        out += layout_cases(dt) + combo_cases(dt) + mask_cases(dt) + [several_case(dt)] + fourth_cases(dt)
    return out


def case_id(c):
    return "%dx%dx%d-gc%d.%d.%d-%s-d%d%d%d%d-m%d-o%d-n%d" % (c.shape + c.gc + (tag(c.dtype),) + tuple(c.dirs) + (c.mask, c.order, c.nf))


def grid_of(c):
    s, gc = c.shape, c.gc
    if c.order == 4:          # a stretched grid: the fill does not read the metrics, the grid's order selects the kernels
        return Grid(*s, 2*np.pi, np.pi, 2., order=4, igc=gc[0], jgc=gc[1], kgc=gc[2], z=moser_z(s[2], 2.), dtype=c.dtype)
    return cm.grid_2nd(*s, gc=gc, dtype=c.dtype)


def fields_of(c):
    """nf fields [kcells][jcells][icells] of full-mantissa values in [-1, 2), ghost cells included, and nf profiles of ktot values."""
    g = grid_of(c)
    rs = np.random.RandomState(4200 + 13*c.shape[0] + 5*c.gc[0] + c.gc[2])
    a = [np.ascontiguousarray(rs.random_sample(g.shape3)*3. - 1., dtype=c.dtype) for _ in range(c.nf)]
    p = [np.ascontiguousarray(rs.random_sample(g.ktot)*2. - 0.5, dtype=c.dtype) for _ in range(c.nf)]
    return a, p


def table_of(g, prof):
    """The kcells table of Boundary::process_inflow (src/boundary.cxx:421-424) restated: ktot values at kstart, zero ghost levels."""
    t = np.zeros(g.kcells, dtype=g.np_dtype)
    t[g.kstart:g.kend] = prof
    return t


# ---- the shim -------------------------------------------------------------------------------------------------------------------
class ODims(C.Structure):
    """struct ODims of tests/cpp/ref_outflow_shim.cpp."""
    _fields_ = [(n, C.c_int) for n in ("istart", "iend", "igc", "jstart", "jend", "jgc", "kgc", "icells", "jcells", "kcells", "ijcells")]


def odims_of(g):
    d = ODims()
    for n, _ in ODims._fields_:
        setattr(d, n, getattr(g, n))
    return d


def _bind(lib):
    lib.ref_outflow_exec.argtypes = [C.c_int, C.c_int, C.POINTER(ODims), C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
    lib.ref_outflow_exec.restype = None


shim = refshim.Shim("outflow", ["ref_outflow_shim.cpp"], _bind, stubs=True, defines=refshim.NC_FILL)


def ref_exec(g, a, table, dirs, mask, order=2):
    """Boundary_outflow<TF>::exec of the reference on the host array `a` (in place) with the kcells table."""
    assert a.flags.c_contiguous and a.dtype == g.np_dtype and a.shape == g.shape3 and table.shape == (g.kcells,) and table.dtype == g.np_dtype
    shim().ref_outflow_exec(code(g.np_dtype), order, C.byref(odims_of(g)), cm.ptr(a), cm.ptr(table), (C.c_int*4)(*dirs), mask)
    return a


def ref_case(c):
    g = grid_of(c)
    a, p = fields_of(c)
    return np.array([ref_exec(g, x.copy(), table_of(g, q), c.dirs, c.mask, c.order) for x, q in zip(a, p)])


def _compute_all():
    return {case_id(c): ref_case(c) for c in all_cases()}


GOLD = refshim.Golden("outflow", _compute_all, "tests/test_outflow_exec.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(c, be=None):
    return GOLD.ref(case_id(c), be)


# ---- the library's call -------------------------------------------------------------------------------------------------------
def lib_exec(be, g, fields, tables, dirs, mask, order=2, expect=0):
    """mhh_boundary_outflow_exec on backend arrays (in place); returns the status and the launches of the call."""
    n = len(fields)
    fa = (C.c_void_p * max(1, n))(*[be.ptr(x).value for x in fields])
    pa = (C.c_void_p * max(1, n))(*[be.ptr(x).value for x in tables])
    rc = be.lib.mhh_boundary_outflow_exec(be.grid(g), order, fa, n, pa, (C.c_int*4)(*dirs), mask, be.stream)
    launches = be.lib.mhh_boundary_outflow_last_launches()
    be.sync()
    return rc, launches


def ghost_blocks(g, nrows_y=None):
    """Named index blocks of the lateral ghost cells: the four edges without the corners, and the four corners; nrows_y South / North
    rows (default kgc: what the fill sets), over all levels."""
    n = g.kgc if nrows_y is None else nrows_y
    W, E, X = slice(0, g.istart), slice(g.iend, g.icells), slice(g.istart, g.iend)
    S, N, Y = slice(g.jstart - n, g.jstart), slice(g.jend, g.jend + n), slice(g.jstart, g.jend)
    K = slice(None)
    return {"west": (K, Y, W), "east": (K, Y, E), "south": (K, S, X), "north": (K, N, X),
            "corner south-west": (K, S, W), "corner south-east": (K, S, E), "corner north-west": (K, N, W), "corner north-east": (K, N, E)}
