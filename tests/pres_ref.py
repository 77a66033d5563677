"""Shared plumbing of tests/test_pres_ref.py: the seeded cases of the pressure solver, the cyclic fills and the horizontal means, and
their reference results.

The reference is the reference's OWN source (src/pres_2.cxx, src/pres_4.cxx, src/boundary_cyclic.cxx, src/field3d_operators.cxx, the evisc kernels of
src/diff_smag2.cxx, the kernels of src/thermo_dry.cxx, src/force.cxx and src/buffer.cxx) behind tests/cpp/ref_pres_shim.cpp, ref_thermo_dry_shim.cpp
and ref_force_shim.cpp, compiled into a temporary directory where the reference tree exists; nothing compiled from it is kept.
Its transforms are a seam: none (they do nothing) or the oracle's DFT (orc_fft_forward / orc_fft_backward, pinned against numpy.fft in
tests/test_oracle_pres.py); FFTW's own bits depend on its plan and stay unpinned.

Where the tree is absent the same cases read tests/golden/pres_ref.npz, recorded with
    MHH_RECORD_PRES_GOLDEN=1 python -m pytest tests/test_pres_ref.py
It holds reference OUTPUTS only: the coefficient vectors, the interior of p after Pres::exec (and of ut, vt, wt for the shapes the
library's solve is held against), the mean profiles, the stretched z profiles (moser_z's last bits follow the host's numpy), and the
SHA-256 of every array that is compared bit for bit. The inputs are common.Case's seeded draws on every host."""
import contextlib
import ctypes as C
import json

import numpy as np

import common as cm
import refshim
from common import ptr, dbl
from refshim import have_reference, tag, typed_digest as digest  # noqa: F401

GOLD = refshim.Golden("pres", None, "tests/test_pres_ref.py")       # recorded piece by piece, by the src=reference cases of the tests
RECORD, golden = GOLD.record, GOLD.need
DT = 0.7

# (order, (itot, jtot, ktot), (igc, jgc, kgc)): the shapes of test_pres (tests/test_parity.py), an odd itot and jtot (the n/2+1 mirror
# of the wave numbers), the fewest levels each order's grid can be built with, and the power-of-two shapes of the LDS forms
CASES = [
    (2, (16, 12, 10), (1, 1, 1)), (2, (12, 10, 8), (3, 3, 1)), (2, (12, 1, 8), (1, 1, 1)), (2, (16, 8, 6), (2, 2, 1)),
    (2, (9, 7, 6), (1, 1, 1)), (2, (8, 6, 1), (1, 1, 1)), (2, (32, 16, 10), (3, 3, 1)),
    (4, (16, 12, 12), (3, 3, 3)), (4, (12, 1, 8), (3, 3, 3)), (4, (16, 8, 8), (3, 3, 3)),
    (4, (9, 7, 6), (3, 3, 3)), (4, (8, 6, 2), (3, 3, 3)), (4, (32, 16, 13), (3, 3, 3)),
]
# the shapes mhh_pres_exec is held against (their ut, vt, wt are stored as values)
EXEC_CASES = [c for c in CASES if c[1] in ((16, 8, 6), (32, 16, 10), (16, 8, 8), (32, 16, 13))]
# what the library's stages are held against: test_pres's shapes and the above
LIB_CASES = [c for c in CASES if c[1] not in ((9, 7, 6), (8, 6, 1), (8, 6, 2))]

CYCLIC_CASES = [((16, 12, 10), (1, 1, 1)), ((12, 10, 8), (3, 3, 1)), ((12, 1, 8), (1, 1, 1)), ((12, 1, 8), (3, 2, 1)), ((9, 7, 6), (2, 3, 2)),
                ((16, 8, 6), (2, 2, 1)), ((5, 4, 3), (3, 1, 1)), ((70, 9, 8), (3, 3, 2))]
MEAN_SHAPES = [(70, 9, 10), (20, 1, 12), (130, 37, 6)]          # tests/test_field_means.py
THERMO_SHAPES = [(70, 9, 10), (17, 9, 8), (20, 1, 12)]          # tests/test_thermo_buoy.py
GRAV = 9.81                                                      # Constants::grav, which the reference's kernels read themselves


def case_id(case):
    order, shape, gc = case
    return "o%d-%dx%dx%d-gc%d%d%d" % ((order,) + shape + gc)


# ---- the golden file ------------------------------------------------------------------------------------------------------------
_digests = {}
REC = {"arrays": {}, "digests": {}}


def golden_digest(key):
    """The recorded digest of the reference's output `key` (the file's JSON table, parsed once per loaded file)."""
    z = golden()
    if _digests.get("of") is not z:
        _digests.update(of=z, table=json.loads(str(z["digests"])))
    return _digests["table"][key]


def zprofile(ktot, zsize):
    """The stored stretched profile (recorded from moser_z)."""
    key = "z/%d/%r" % (ktot, zsize)
    if RECORD:
        if key not in REC["arrays"]:
            REC["arrays"][key] = cm.moser_z(ktot, zsize)
        return REC["arrays"][key]
    return golden()[key]


def write_record():
    GOLD.save(dict(digests=np.array(json.dumps(REC["digests"], sort_keys=True)), **REC["arrays"]))


def expect_bits(src, key, got, run_ref):
    """got against the reference bit for bit. src 'reference': its own output run_ref() (recorded when asked); src 'golden': the
    recorded digest of that output. Returns (equal, detail)."""
    got = np.asarray(got)
    if src == "reference":
        want = np.asarray(run_ref())
        if RECORD:
            REC["digests"][key] = digest(want)
        ok = got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
        return ok, (key, "ulp", cm.ulp_diff(got, want)) if not ok and got.shape == want.shape and got.dtype.kind == "f" else (key,)
    return digest(got) == golden_digest(key), MISMATCH % key


def expect_values(src, key, run_ref):
    """The reference's values under key: computed (and recorded when asked) or read from the file."""
    if src == "reference":
        want = np.ascontiguousarray(run_ref())
        if RECORD:
            REC["arrays"][key] = want
        return want
    return golden()[key]


MISMATCH = ("%s differs from the recorded reference output. The golden file holds this array's SHA-256 only: where the reference tree "
            "exists, rerun the src=reference case of tests/test_pres_ref.py (the test_oracle_* / *_against_the_reference_* tests), which "
            "reports the ulp difference against the reference itself")


def same_as_golden(key, got):
    """(equal, message) of the library's array got against the recorded digest of the reference's output."""
    return digest(got) == golden_digest(key), MISMATCH % key


# ---- grids and inputs ---------------------------------------------------------------------------------------------------------------
def grid_of(case, dtype):
    order, shape, gc = case
    if order == 2:
        return cm.grid_2nd(*shape, gc=gc, dtype=dtype, z=zprofile(shape[2], 1200.))
    return cm.grid_4th(*shape, dtype=dtype, z=zprofile(shape[2], 2.))


_cases = {}


def inputs(case, dtype):
    """(grid, Case) as tests/test_parity.py::test_pres prepares them: random rhoref / rhorefh for order 2, cyclic velocities, mirrored w
    below and above the walls for order 4. Shared and never written to."""
    key = (case, tag(dtype))
    if key not in _cases:
        g = grid_of(case, dtype)
        c = cm.Case(g, rho=("random" if case[0] == 2 else "one"), periodic=True)
        if case[0] == 4:
            for m in (1, 2):
                c.w[g.kstart-m] = -c.w[g.kstart+m]; c.w[g.kend+m] = -c.w[g.kend-m]
        for a in [c.u, c.v, c.w, c.ut, c.vt, c.wt, c.rhoref, c.rhorefh]:
            a.setflags(write=False)
        _cases[key] = (g, c)
    return _cases[key]


def written(g, order):
    """The cells of p that Pres::solve leaves with a value of its own: the interior, the mirrored ghost levels (one below for order 2,
    two below and two above for order 4) and their cyclic ghost cells. The levels beyond keep whatever the array held, and in a 2-D run
    (jtot == 1) Boundary_cyclic fills the ghost rows of the interior levels only."""
    m = np.zeros(g.shape3, dtype=bool)
    k0, k1 = (g.kstart-1, g.kend) if order == 2 else (g.kstart-2, g.kend+2)
    m[k0:k1] = True
    if g.jtot == 1:
        m[k0:g.kstart, :g.jstart] = False; m[k0:g.kstart, g.jend:] = False
        m[g.kend:k1, :g.jstart] = False; m[g.kend:k1, g.jend:] = False
    return m


def masked(p, g, order):
    return np.where(written(g, order), p, 0).astype(p.dtype)


def packed_random(g, seed=3):
    return np.random.RandomState(seed).random_sample((g.ktot, g.jtot, g.itot)).astype(g.np_dtype)


def field_with_packed(g, packed):
    """A whole field with the packed values at its start, as the reference's Pres::exec hands its p to solve."""
    p = np.zeros(g.ncells, dtype=g.np_dtype)
    p[:packed.size] = packed.ravel()
    return p


# ---- the shim ---------------------------------------------------------------------------------------------------------------------
def _bind(lib):
    lib.ref_pres_divergence.restype = C.c_double
    lib.ref_thermo_dry_grav.restype = C.c_double
    lib.ref_calc_mean.restype = C.c_double
    lib.ref_pres_set_fft.argtypes = [C.c_void_p, C.c_void_p]


shim = refshim.Shim("pres", ["ref_pres_shim.cpp", "ref_thermo_dry_shim.cpp", "ref_force_shim.cpp"], _bind, ref_sources=refshim.MASTER,
                    stubs=True, project_include=True)


@contextlib.contextmanager
def transforms(mode):
    """mode 'identity': the reference's FFT does nothing; 'oracle': it is the oracle's DFT."""
    lib = shim()
    if mode == "oracle":
        O = cm.oracle()
        lib.ref_pres_set_fft(C.cast(O.orc_fft_forward, C.c_void_p), C.cast(O.orc_fft_backward, C.c_void_p))
    else:
        lib.ref_pres_set_fft(None, None)
    try:
        yield lib
    finally:
        lib.ref_pres_set_fft(None, None)


def ref_exec(case, dtype):
    """The reference's input -> solve (the oracle's DFT) -> output on the case: (p, ut, vt, wt), whole arrays."""
    g, c = inputs(case, dtype)
    p = np.zeros(g.ncells, dtype=dtype)
    ut, vt, wt = c.ut.copy(), c.vt.copy(), c.wt.copy()
    with transforms("oracle") as R:
        R.ref_pres_exec(g.host_struct(), case[0], ptr(p), ptr(c.u), ptr(c.v), ptr(c.w), ptr(ut), ptr(vt), ptr(wt), ptr(c.rhoref), ptr(c.rhorefh), dbl(DT))
    return p.reshape(g.shape3), ut, vt, wt


def golden_exec(case, dtype):
    """For the tests of the library: (p with every ghost cell the reference writes, ut, vt, wt interiors or None) from the file alone.
    p is rebuilt from its stored interior by the oracle's unpack, and checked against the digest of the reference's whole array."""
    g, c = inputs(case, dtype)
    z = golden()
    key = "exec/%s/%s/" % (case_id(case), tag(dtype))
    p = np.zeros(g.shape3, dtype=dtype)
    interior = np.ascontiguousarray(z[key + "p"])
    cm.oracle().orc_pres_unpack(g.host_struct(), case[0], ptr(p), ptr(interior))
    p = masked(p, g, case[0])
    assert digest(p) == golden_digest(key + "p_written"), key
    tend = tuple(z[key + n] for n in ("ut", "vt", "wt")) if case in EXEC_CASES else None
    return p, tend
