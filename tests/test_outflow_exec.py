"""mhh_boundary_outflow_exec against the reference's Boundary_outflow loops, bit for bit, fp64 and fp32.

The reference is tests/outflow_ref.py: the reference's own loops behind a shim on the emulation where the reference tree exists, the
golden file elsewhere and on the GPU; on the emulation with the tree both are compared. The shapes are the smallest at which each
hazard exists (outflow_ref.LAYOUTS). A test compares the whole field first and then names the block that differs: the four edges and,
separately, the four corners, which are the South / North rule applied to what West / East wrote.
"""
import ctypes as C

import numpy as np
import pytest

import common as cm
import outflow_ref as R
from backends import be  # noqa: F401
from common import same_bits as same

ids = R.case_id


def _run(be, c, g=None):
    g = R.grid_of(c) if g is None else g
    a, p = R.fields_of(c)
    dev = [be.arr(x) for x in a]
    tabs = [be.arr(R.table_of(g, q)) for q in p]
    rc, launches = R.lib_exec(be, g, dev, tabs, c.dirs, c.mask, c.order)
    return rc, launches, np.array([be.host(x) for x in dev]), np.array(a)


def _check(be, c):
    rc, launches, got, before = _run(be, c)
    assert rc == 0, be.lib.mhh_last_error()
    want = R.ref(c, be)
    g = R.grid_of(c)
    for name, blk in R.ghost_blocks(g).items():
        for n in range(c.nf):
            assert same(got[n][blk], want[n][blk]), "%s of field %d differs from the reference (%s)" % (name, n, ids(c))
    assert same(got, want), ids(c)
    assert same(got[(slice(None),) + g.interior], before[(slice(None),) + g.interior])
    return launches, got, before


def test_record_or_compare_the_golden_file():
    """With MHH_RECORD_OUTFLOW_GOLDEN=1: write the file. With the reference tree: the shim's results are the file's."""
    R.record_if_asked()
    z = R.GOLD.need()
    assert sorted(z.files) == sorted({ids(c) for c in R.all_cases()})        # (a layout case is also one of the combinations)
    if R.have_reference():
        rec = R.computed()
        for k in z.files:
            assert same(z[k], rec[k]), k


@pytest.mark.parametrize("c", R.layout_cases(R.F64) + R.layout_cases(R.F32), ids=ids)
def test_layouts(be, c):
    """kgc = 1, 2, 3 rows of jgc = 3; gc (1,1,1); igc = 16 at itot == igc and above; a ragged grid."""
    launches, got, before = _check(be, c)
    assert launches == 2
    g = R.grid_of(c)
    # South and North set kgc rows: the ghost rows beyond, and whatever West / East wrote there, are not the South / North rule's
    for j in list(range(0, g.jstart - g.kgc)) + list(range(g.jend + g.kgc, g.jcells)):
        assert same(got[0][:, j, g.istart:g.iend], before[0][:, j, g.istart:g.iend]), "ghost row %d beyond kgc was written" % j


@pytest.mark.parametrize("c", R.combo_cases(R.F64) + R.combo_cases(R.F32), ids=ids)
def test_every_combination_of_inflow_and_outflow(be, c):
    _check(be, c)


@pytest.mark.parametrize("c", R.mask_cases(R.F64) + R.mask_cases(R.F32), ids=ids)
def test_edge_masks(be, c):
    """West only, South only, none: the edges of other ranks are left alone."""
    launches, got, before = _check(be, c)
    assert launches == (1 if c.mask else 0)
    g = R.grid_of(c)
    touched = np.zeros(g.shape3, dtype=bool)
    if c.mask & R.WEST:
        touched[:, :, :g.istart] = True
    if c.mask & R.SOUTH:
        touched[:, g.jstart - g.kgc:g.jstart, :] = True
    assert same(got[0][~touched], before[0][~touched])
    assert not c.mask or not same(got[0][touched], before[0][touched])


@pytest.mark.parametrize("dt", cm.DTYPES, ids=["f64", "f32"])
def test_several_scalars_in_the_launches_of_one(be, dt):
    """Three scalars with different profiles in one call: the launch count is that of a one-scalar call, at most two."""
    c = R.several_case(dt)
    launches, got, _ = _check(be, c)
    one, _, _ = _check(be, R.Case(*R.COMBO_LAYOUT, dt, c.dirs, c.mask, 2, 1))
    assert launches == one == 2
    assert not same(got[0], got[1]) and not same(got[1], got[2])


@pytest.mark.parametrize("c", R.fourth_cases(R.F64) + R.fourth_cases(R.F32), ids=ids)
def test_fourth_order(be, c):
    """compute_inflow_4th with value 0 at West, compute_outflow_4th at East; directions and profiles are ignored, North and South
    stay as they were."""
    launches, got, before = _check(be, c)
    assert launches == 1
    g = R.grid_of(c)
    assert same(got[0][:, :, g.istart:g.iend], before[0][:, :, g.istart:g.iend])
    # ignored: the other directions and no profiles at all give the same bits
    dev = [be.arr(before[0])]
    fa = (C.c_void_p * 1)(be.ptr(dev[0]).value)
    assert be.lib.mhh_boundary_outflow_exec(be.grid(g), 4, fa, 1, None, None, c.mask, be.stream) == 0, be.lib.mhh_last_error()
    be.sync()
    assert same(be.host(dev[0]), got[0])


def _patched(g, **kw):
    for k, v in kw.items():
        setattr(g, k, v)
    g.icells, g.jcells = g.imax + 2*g.igc, g.jmax + 2*g.jgc
    g.iend, g.jend = g.istart + g.imax, g.jstart + g.jmax
    g.ijcells = g.icells*g.jcells
    g.ncells = g.ijcells*g.kcells
    return g


@pytest.mark.parametrize("dt", cm.DTYPES, ids=["f64", "f32"])
def test_refused_geometries_leave_the_field_untouched(be, dt):
    """The reference's serial loops would read cells they also write, or index outside the field: an error, and no launch."""
    wide = cm.grid_2nd(8, 6, 5, gc=(16, 3, 1), dtype=dt)                                   # itot < igc
    thin = _patched(cm.grid_2nd(8, 6, 5, gc=(3, 3, 3), dtype=dt), jtot=2, jmax=2)          # jmax < kgc
    tall = cm.grid_2nd(8, 6, 5, gc=(3, 1, 2), dtype=dt)                                    # kgc > jgc
    for g, mask, word in ((wide, R.ALL, "itot < igc"), (thin, R.SOUTH, "jmax < kgc"), (thin, R.NORTH, "jmax < kgc"), (tall, R.ALL, "kgc > jgc"),
                          (tall, R.WEST, "kgc > jgc")):
        rs = np.random.RandomState(5)
        a = np.ascontiguousarray(rs.random_sample(g.shape3), dtype=dt)
        dev, tab = be.arr(a), be.arr(np.zeros(g.kcells, dtype=dt))
        rc, launches = R.lib_exec(be, g, [dev], [tab], (R.IN, R.OUT, R.OUT, R.IN), mask)
        assert rc != 0 and launches == 0, word
        assert word in be.lib.mhh_last_error().decode()
        assert same(be.host(dev), a), word
    # jmax < kgc is refused for a South or North edge only: West and East of the same grid run
    a = np.ascontiguousarray(np.random.RandomState(6).random_sample(thin.shape3), dtype=dt)
    dev = be.arr(a)
    rc, launches = R.lib_exec(be, thin, [dev], [be.arr(np.zeros(thin.kcells, dtype=dt))], (R.OUT,)*4, R.WEST | R.EAST)
    assert rc == 0 and launches == 1


@pytest.mark.parametrize("dt", cm.DTYPES, ids=["f64", "f32"])
def test_exact_properties(be, dt):
    """No reference needed: a field that equals the inflow profile on every level keeps that value in the inflow ghost cells; pure
    outflow is an exact mirror; bytes outside the ghost cells of the active edges are unchanged."""
    g = cm.grid_2nd(8, 6, 5, gc=(3, 3, 2), dtype=dt)
    rs = np.random.RandomState(11)
    prof = np.ascontiguousarray(rs.random_sample(g.ktot) + 0.25, dtype=dt)
    a = np.zeros(g.shape3, dtype=dt)
    a[g.kstart:g.kend] = prof[:, None, None]             # the ghost levels hold the table's zero
    dev = be.arr(a)
    rc, _ = R.lib_exec(be, g, [dev], [be.arr(R.table_of(g, prof))], (R.IN,)*4, R.ALL)
    assert rc == 0
    assert same(be.host(dev), a)
    # the helper that makes the table
    tab = np.full(g.kcells, 7., dtype=dt)
    assert be.lib.mhh_boundary_outflow_profile_host(g.host_struct(), cm.ptr(prof), cm.ptr(tab)) == 0
    assert same(tab, R.table_of(g, prof)) and not tab[:g.kstart].any() and not tab[g.kend:].any()
    # pure outflow
    b = np.ascontiguousarray(rs.random_sample(g.shape3), dtype=dt)
    dev = be.arr(b)
    rc, _ = R.lib_exec(be, g, [dev], [be.arr(R.table_of(g, prof))], (R.OUT,)*4, R.ALL)
    assert rc == 0
    got = be.host(dev)
    n = g.kgc
    want = b.copy()
    want[:, :, :g.istart] = b[:, :, g.istart:g.istart + g.igc][:, :, ::-1]
    want[:, :, g.iend:] = b[:, :, g.iend - g.igc:g.iend][:, :, ::-1]
    want[:, g.jstart - n:g.jstart, :] = want[:, g.jstart:g.jstart + n, :][:, ::-1, :]
    want[:, g.jend:g.jend + n, :] = want[:, g.jend - n:g.jend, :][:, ::-1, :]
    assert same(got, want)
    keep = np.ones(g.shape3, dtype=bool)
    keep[:, :, :g.istart] = keep[:, :, g.iend:] = False
    keep[:, g.jstart - n:g.jstart, :] = keep[:, g.jend:g.jend + n, :] = False
    assert same(got[keep], b[keep])


@pytest.mark.parametrize("dt", cm.DTYPES, ids=["f64", "f32"])
def test_pure_outflow_needs_no_profiles(be, dt):
    """Second order, every active edge outflow: profiles may be NULL (no table is read), and the result is that of a call with one.
    An inflow direction on an edge that the mask leaves out needs none either; an active inflow edge without one is refused."""
    g = cm.grid_2nd(8, 6, 5, gc=(3, 3, 2), dtype=dt)
    a = np.ascontiguousarray(np.random.RandomState(21).random_sample(g.shape3), dtype=dt)
    with_table = be.arr(a)
    rc, _ = R.lib_exec(be, g, [with_table], [be.arr(np.ones(g.kcells, dtype=dt))], (R.OUT,)*4, R.ALL)
    assert rc == 0
    want = be.host(with_table)
    for dirs, mask in (((R.OUT,)*4, R.ALL), ((R.IN, R.OUT, R.OUT, R.OUT), R.EAST | R.SOUTH | R.NORTH), ((R.OUT, R.OUT, R.IN, R.OUT), R.WEST | R.EAST | R.NORTH)):
        dev = be.arr(a)
        fa = (C.c_void_p * 1)(be.ptr(dev).value)
        for profiles in (None, (C.c_void_p * 1)(None)):
            assert be.lib.mhh_boundary_outflow_exec(be.grid(g), 2, fa, 1, profiles, (C.c_int*4)(*dirs), mask, be.stream) == 0, be.lib.mhh_last_error()
            be.sync()
        got = be.host(dev)
        keep = np.ones(g.shape3, dtype=bool)
        if not mask & R.WEST:
            keep[:, :, :g.istart] = False
        if not mask & R.SOUTH:
            keep[:, g.jstart - g.kgc:g.jstart, :] = False
        assert same(got[keep], want[keep])           # (the columns and rows left out hold what the other rule made of unfilled cells)
    dev = be.arr(a)
    fa = (C.c_void_p * 1)(be.ptr(dev).value)
    for profiles in (None, (C.c_void_p * 1)(None)):
        assert be.lib.mhh_boundary_outflow_exec(be.grid(g), 2, fa, 1, profiles, (C.c_int*4)(R.OUT, R.OUT, R.OUT, R.IN), R.ALL, be.stream) != 0
        assert be.lib.mhh_boundary_outflow_last_launches() == 0
    assert same(be.host(dev), a)


@pytest.mark.parametrize("dt", cm.DTYPES, ids=["f64", "f32"])
def test_fourth_order_refusals(be, dt):
    """Three ghost columns from three interior cells: igc < 3 is refused, and itot < 3 (which with igc >= 3 is itot < igc), the field
    untouched."""
    from microhh_amd.grid import Grid, moser_z
    narrow = Grid(8, 6, 8, 6.3, 3.1, 2., order=4, igc=2, jgc=3, kgc=3, z=moser_z(8, 2.), dtype=dt)        # igc < 3
    short = _patched(Grid(8, 6, 8, 6.3, 3.1, 2., order=4, igc=3, jgc=3, kgc=3, z=moser_z(8, 2.), dtype=dt), itot=2, imax=2)      # itot < 3, hence < igc
    for g, word in ((narrow, "fourth-order"), (short, "itot < igc")):
        a = np.ascontiguousarray(np.random.RandomState(8).random_sample(g.shape3), dtype=dt)
        dev = be.arr(a)
        rc, launches = R.lib_exec(be, g, [dev], [be.arr(np.zeros(g.kcells, dtype=dt))], R.JAENSCHWALDE, R.ALL, order=4)
        assert rc != 0 and launches == 0
        assert word in be.lib.mhh_last_error().decode()
        assert same(be.host(dev), a)
