"""Boundary_outflow on a y-slab: West and East act on every rank, over its ghost rows too; South acts on rank 0 only and North on rank
npy-1 only (src/boundary_outflow.cxx:303, :323).

The fill: N = 2 and 3 ranks held in one process (tests/vranks.py), every rank's fields -- the halo exchange, then
mhh_boundary_outflow_exec with the rank's edge mask -- are the rank's rows of the one-rank fields after the cyclic fill and the fill
of all four edges, ghost rows and columns included: the interior, the domain's outer ghost cells, and the rows between the ranks.

The step: with scalar 0 open (it feeds N2, hence evisc) HotPath switches evisc_local_ghosts off and exchanges evisc; two gloo ranks
on the emulation, and one rank on the slab path (force_slab), have evisc and the scalar tendencies of the plain one-rank step bit for
bit, and the two ranks have every field of the one rank on the slab path (whose pressure solve transforms in the same order).
"""
import numpy as np
import pytest

import backends as B
import common as cm
import outflow_ref as R
import vranks as V
from backends import be  # noqa: F401
from common import same_bits as same
from ranks import run_ranks

GC = (3, 3, 2)
NAMES = ("u", "v", "w")                 # three fields of the rank cases stand in for three open scalars
DIRS = (R.IN, R.OUT, R.IN, R.OUT)


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("npy", [2, 3])
def test_the_ranks_fill_is_the_one_rank_fill(be, npy, dtype):
    from microhh_amd.outflow import edges_of
    gg = cm.grid_2nd(6*npy, 12*npy, 5, gc=GC, dtype=dtype)          # itot and jtot divide by npy
    rs = np.random.RandomState(77 + npy)
    case = cm.Case(gg, nscalars=0)
    for n in NAMES:
        setattr(case, n, np.ascontiguousarray(rs.random_sample(gg.shape3)*3. - 1., dtype=dtype))
    profs = [np.ascontiguousarray(rs.random_sample(gg.ktot), dtype=dtype) for _ in NAMES]
    tabs = [be.arr(R.table_of(gg, p)) for p in profs]
    # one rank: the cyclic fill, then all four edges
    one = [be.arr(getattr(case, n)) for n in NAMES]
    B.ok(be, be.lib.mhh_boundary_cyclic_n(be.grid(gg), (V.C.c_void_p * 3)(*[be.ptr(a).value for a in one]), 3, cm.EDGE_BOTH, be.stream))
    rc, _ = R.lib_exec(be, gg, one, tabs, DIRS, R.ALL)
    assert rc == 0, be.lib.mhh_last_error()
    want = [be.host(a) for a in one]
    vr = V.VRanks(be, case, npy, plans=False)
    assert vr.grids[0].jmax >= 12
    vr.ring([vr.f(n) for n in NAMES])
    for r, g in enumerate(vr.grids):
        mask = edges_of(npy, r)
        assert mask == R.WEST | R.EAST | (R.SOUTH if r == 0 else 0) | (R.NORTH if r == npy - 1 else 0)
        rc, launches = R.lib_exec(be, g, [vr.f(n)[r] for n in NAMES], tabs, DIRS, mask)
        assert rc == 0 and launches == (2 if r in (0, npy - 1) else 1)
    for n, w in zip(NAMES, want):
        for r, g in enumerate(vr.grids):
            assert same(be.host(vr.f(n)[r]), V.rows_of(gg, g, w)), (n, r)
        assert same(vr.gather(n), w[gg.interior])


# ---- the step with scalar 0 open ------------------------------------------------------------------------------------------------
GRID = (32, 24, 16)
FIELDS = ("evisc", "st0", "st1", "ut", "vt", "wt", "p")
EXACT = ("evisc", "st0", "st1")          # what does not pass through the pressure solve


def _make(**kw):
    from microhh_amd.model import HotPath, synthetic_global
    from microhh_amd.outflow import Outflow
    g = cm.grid_2nd(*GRID)
    prof = 300. + 0.02*np.arange(g.ktot)
    return HotPath("drycblles", *GRID, device="cpu", lib=B.get("emul").lib, nscalars=2, global_init=synthetic_global("drycblles", *GRID, nscalars=2),
                   outflow=Outflow({0: prof, 1: prof + 1.}, west="inflow", east="outflow", south="inflow", north="outflow"), **kw)


def _results(hp, out):
    g = hp.grid
    out["local_ghosts"] = np.array([int(hp.evisc_local_ghosts), int(hp.can_overlap)])
    hp.step(); hp.sync()
    for n, t in zip(FIELDS, (hp.evisc, hp.st[0], hp.st[1], hp.ut, hp.vt, hp.wt, hp.p)):
        out[n] = t.detach().cpu().numpy()[g.interior].copy()
    hp.close()


def _worker(rank, world, out):
    _results(_make(npy=world, rank=rank), out)


def _single(**kw):
    out = {}
    _results(_make(**kw), out)
    return out


@pytest.fixture(scope="module")
def plain():
    return _single()


def test_scalar_0_open_on_one_rank_on_the_slab_path(plain):
    one = _single(force_slab=True)
    assert not one["local_ghosts"].any()
    for n in EXACT:
        assert same(one[n], plain[n]), n


def test_scalar_0_open_on_two_ranks(plain):
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")
    assert GRID[1]//2 >= 12
    one = _single(force_slab=True)
    for p in parts:
        assert not p["local_ghosts"].any()          # evisc is exchanged, the sub-step is the plain sequence
    for n in FIELDS:
        got = np.concatenate([p[n] for p in parts], axis=1)
        assert same(got, one[n]), n
        if n in EXACT:
            assert same(got, plain[n]), n
