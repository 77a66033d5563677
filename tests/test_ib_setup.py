"""The host set-up of csrc/immersed_boundary.h (mhh_ib_ghost_cells_host, mhh_ib_k_dem_host, mhh_ib_interp_dem_host) against the
reference's calc_ghost_cells, find_k_dem and interp2_dem: every array bit for bit, for the four staggered locations, the three
boundary types of s, both dtypes and every shape of tests/ib_ref.py; against tests/golden/ib_ref.npz where the reference tree is
absent. And: the cells a list reads are never cells it writes; terrain below the first level gives empty lists; the refusals."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import ib_ref as R
from microhh_amd import capi, ib
from microhh_amd.grid import Grid

IDS = [R.case_id(c) for c in R.CASES]
NAMES = ("u", "v", "w", "s", "s_neumann", "s_flux")
BC_OF = {"u": 0, "v": 0, "w": 0, "s": 0, "s_neumann": 1, "s_flux": 2}
CASE0 = R.CASES[1]              # 16x8x16, gc (2,2,1), fp32


def lib():
    return B.get("emul").lib


def test_record_golden():
    """With MHH_RECORD_IB_GOLDEN=1 this writes tests/golden/ib_ref.npz; always: the inputs the file holds are the ones this host
    draws."""
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/ib_ref.npz is missing"
    for case in R.CASES:
        for k, v in R.IbCase(case).drawn.items():
            assert cm.same_bits(z["%s/in/%s" % (R.case_id(case), k)], v), (R.case_id(case), k)


@pytest.mark.skipif(not R.have_reference(), reason="the reference tree is not on this machine")
def test_golden_is_the_shim():
    z, rec = R.golden(), R.computed()
    assert set(z.files) == set(rec)
    for k in rec:
        assert cm.same_bits(z[k], rec[k]), k


def test_the_locations_are_the_grids():
    """gd.x, gd.xh, gd.y, gd.yh (src/grid.cxx:248-262) on the second rank of two: cell centres and faces, offset by the rank's rows."""
    g = Grid(16, 8, 16, R.XSIZE, R.YSIZE, R.ZSIZE, igc=2, jgc=2, kgc=1, npy=2, mpicoordy=1)
    c = ib.locations(g)
    assert np.array_equal(c["xh"], (np.arange(g.icells) - 2)*200.) and np.array_equal(c["x"], c["xh"] + 100.)
    assert np.array_equal(c["yh"], (np.arange(g.jcells) - 2)*200. + 800.) and np.array_equal(c["y"], c["yh"] + 100.)
    assert ib.mpi_offsets(g) == (2, -4 + 2)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_setup_is_the_reference(case):
    g, dem = R.grid_of(case), R.dem_of(case)
    ax = R.axes(g)
    for name in NAMES:
        want = R.ref_lists(case, name)
        got = ib.ghost_cells(lib(), g, dem, *ax[name if name in R.LOCS else "s"], R.N_IDW, BC_OF[name])
        assert got["nghost"] == want["nghost"] > 0
        for k in R.LISTS:
            assert cm.same_bits(np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])), (name, k)
        # the cells a launch reads and the cells it writes are disjoint: no interpolation point is a ghost cell of its list ...
        tab = ib.device_tables(g, got)
        assert tab["ip"].shape == (R.N_IDW, got["nghost"]) and tab["c_idw"].shape == (R.N_IDW, got["nghost"])
        assert not np.isin(tab["ip"], tab["cell"]).any()
        # ... since the points lie outside the wall and the ghost cells inside it, each at its own column
        x, y, z, _ = ax[name if name in R.LOCS else "s"]
        zd = ib.interp_dem(lib(), g, dem, x[got["i"]], y[got["j"]], x=x, y=y)
        assert np.all(z[got["k"]] <= zd)
        zd = ib.interp_dem(lib(), g, dem, x[got["ip_i"].ravel()], y[got["ip_j"].ravel()], x=x, y=y)
        assert np.all(z[got["ip_k"].ravel()] > zd)
        assert np.array_equal(tab["cell"], R.cells_of(g, want)) and np.array_equal(tab["ip"][2], R.cells_of(g, {k: want["ip_" + k][:, 2] for k in "ijk"}))
    assert np.array_equal(ib.k_dem(lib(), g, dem)[g.jstart:g.jend, g.istart:g.iend], R.ref(case, "k_dem"))
    gs = R.ref_lists(case, "s")
    plane = R.with_halos(g, R.inputs(case).sbot_plane)
    assert cm.same_bits(ib.interp_dem(lib(), g, plane, gs["xb"], gs["yb"]), R.ref(case, "interp"))


def test_a_fill_takes_the_count_calls_scan_only_for_the_same_inputs():
    """The counting call keeps its scan for the filling call. A filling call that is handed other values (here: the count was made
    for another terrain with, by construction, the same number of ghost cells) must scan again."""
    case = R.CASES[0]
    g, dem = R.grid_of(case), R.dem_of(case)
    ax = R.axes(g)["s"]
    want = ib.ghost_cells(lib(), g, dem, *ax, R.N_IDW, 0)
    mirrored = np.ascontiguousarray(dem[:, ::-1])            # the terrain mirrored in x: other cells, the same count
    keep = [np.ascontiguousarray(a, dtype=g.np_dtype) for a in ax]
    n = C.c_int(0)
    capi.check(lib().mhh_ib_ghost_cells_host(g.host_struct(), mirrored.ctypes.data, *[a.ctypes.data for a in keep], R.N_IDW, 0, *ib.mpi_offsets(g), C.byref(n), None), lib())
    assert n.value == want["nghost"]
    got = {k: np.zeros_like(np.ascontiguousarray(v)) for k, v in want.items() if k != "nghost"}
    lists = capi.MhhIbGhostLists()
    for k, a in got.items():
        setattr(lists, k, a.ctypes.data_as(capi.IP) if k in ib.INT_LISTS else a.ctypes.data)
    capi.check(lib().mhh_ib_ghost_cells_host(g.host_struct(), dem.ctypes.data, *[a.ctypes.data for a in keep], R.N_IDW, 0, *ib.mpi_offsets(g), C.byref(n), C.byref(lists)), lib())
    for k in R.LISTS:
        assert cm.same_bits(got[k], np.ascontiguousarray(want[k])), k


def test_ties_are_the_rule():
    """Neighbours at exactly equal distance: hundreds of adjacent pairs per list, so the order std::sort leaves them in is tested."""
    gh = R.ref_lists(R.CASES[0], "s")
    assert np.count_nonzero(gh["ip_d"][:, 1:] == gh["ip_d"][:, :-1]) > 100


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
def test_terrain_below_the_first_level_gives_empty_lists(dtype):
    case = ((16, 8, 16), (3, 3, 1), 0.15, dtype)
    g = R.grid_of(case)
    dem = np.full(g.shape2, -10., dtype=g.np_dtype)
    for loc, ax in R.axes(g).items():
        got = ib.ghost_cells(lib(), g, dem, *ax, R.N_IDW, 0)
        assert got["nghost"] == 0 and all(got[k].size == 0 for k in R.LISTS)
    assert np.all(ib.k_dem(lib(), g, dem)[g.jstart:g.jend, g.istart:g.iend] == g.kstart)


def refused(match, g, dem, ax, n_idw=R.N_IDW, bc=0, offsets=None):
    with pytest.raises(capi.MhhError, match=match):
        ib.ghost_cells(lib(), g, dem, *ax, n_idw, bc, offsets)


def test_refusals():
    g, dem = R.grid_of(CASE0), R.dem_of(CASE0)
    ax = R.axes(g)["s"]
    # the DEM interpolation out of bounds, in the reference's words: the offsets of another rank
    refused("IB dem interpolation out of bounds!", g, dem, ax, offsets=(2, -40))
    with pytest.raises(capi.MhhError, match="IB dem interpolation out of bounds!"):
        ib.interp_dem(lib(), g, dem, [-1000.], [100.])
    if R.have_reference():
        with pytest.raises(R.RefThrows, match="IB dem interpolation out of bounds!"):
            R.ref_ghost(g, dem, *ax, 0, offsets=(2, -40))
    # fewer than n_idw neighbours: the box holds 8 x 9 cells at the most; the message names the first ghost cell
    gh = R.ref_lists(CASE0, "s")
    refused("only found .* interpolation points @ i=%d, j=%d, k=%d" % (gh["i"][0], gh["j"][0], gh["k"][0]), g, dem, ax, n_idw=73)
    refused("n_idw_points must be at least 1", g, dem, ax, n_idw=0)
    refused("unknown boundary type 7", g, dem, ax, bc=7)
    # fewer than two horizontal ghost cells (src/immersed_boundary.cxx:622)
    g1 = Grid(16, 8, 16, R.XSIZE, R.YSIZE, R.ZSIZE, igc=1, jgc=1, kgc=1, dtype=CASE0[3])
    refused("at least two horizontal ghost cells", g1, R.with_halos(g1, R.interior_dem(CASE0)), R.axes(g1)["s"])
    # terrain between levels kend-4 and kend-3: the ghost cells at kend-4 would read level k+5 = kcells
    top = np.full(g.shape2, 0.5*(float(g.z[g.kend-4]) + float(g.z[g.kend-3])), dtype=g.np_dtype)
    refused("too close to the top", g, top, ax)
    ok = np.full(g.shape2, 0.5*(float(g.z[g.kend-5]) + float(g.z[g.kend-4])), dtype=g.np_dtype)       # one level lower: inside the arrays
    got = ib.ghost_cells(lib(), g, ok, *ax, R.N_IDW, 0)
    assert got["nghost"] > 0 and got["k"].max() == g.kend-5 and got["k"].max() + 5 == g.kcells-1
    # more than 2^31-1 cells: refused before anything is read
    big = Grid(2048, 2048, 600, R.XSIZE, R.YSIZE, R.ZSIZE, igc=2, jgc=2, kgc=1)
    assert big.ncells > 2**31 - 1
    n = C.c_int(0)
    with pytest.raises(capi.MhhError, match="32-bit cell"):
        capi.check(lib().mhh_ib_ghost_cells_host(big.host_struct(), dem.ctypes.data, dem.ctypes.data, dem.ctypes.data, dem.ctypes.data, dem.ctypes.data,
                                                 5, 0, 2, 2, C.byref(n), None), lib())
    # the two-call shape: room for another count is refused
    n = C.c_int(3)
    with pytest.raises(capi.MhhError, match="count first"):
        arrs = [np.ascontiguousarray(a, dtype=g.np_dtype) for a in (dem,) + tuple(ax)]
        capi.check(lib().mhh_ib_ghost_cells_host(g.host_struct(), *[a.ctypes.data for a in arrs], 5, 0, 2, 2, C.byref(n), C.byref(capi.MhhIbGhostLists())), lib())
    with pytest.raises(capi.MhhError, match="null pointer"):
        capi.check(lib().mhh_ib_k_dem_host(g.host_struct(), None, g.z.ctypes.data, None), lib())
