"""The immersed boundary on a slab (npy = 2, gloo ranks on the emulation): the ranks' ghost-cell lists, with j shifted by the rank's
rows, put together are the single-rank lists; after two steps with a Runge-Kutta sub-step between them (so that the momentum ghost
cells reach the RHS and the pressure input) every rank's rows of every prognostic field, tendency, p and evisc equal, bit for bit,
those of one rank that takes the same slab code path (force_slab: the same split pressure solve with the exchanges as local
copies), the halo rows and columns of u, v, w and th included; and they agree with the plain single-rank run within the 1e-10 of
tests/test_slab_gloo.py, whose pressure solve transforms in another order."""
import numpy as np
import pytest

import backends as B
import ib_ref as R
from microhh_amd import ib
from microhh_amd.ib import Dem
from microhh_amd.model import CASES, HotPath, synthetic_global
from ranks import run_ranks

GRID = (16, 16, 16)
N_IDW = 5
LOCS = ("u", "v", "w", "s")
FIELDS = ("u", "v", "w", "th", "ut", "vt", "wt", "tht", "p", "evisc")
WITH_HALOS = ("u", "v", "w", "th")          # whose cyclic fills are the last thing a step does to them


def _make(lib, **kw):
    dem = ib.sine_dem(GRID[0], GRID[1], *CASES["drycblles"]["size"])
    return HotPath("drycblles", *GRID, device="cpu", lib=lib, global_init=synthetic_global("drycblles", *GRID),
                   ib=Dem(dem, N_IDW, sbcbot="flux", sbot=(0.1,)), **kw)


def _results(hp, out):
    g = hp.grid
    for loc in LOCS:
        for k in R.LISTS:
            out["%s/%s" % (loc, k)] = hp.ib.ghost[loc][k]
    hp.step()
    hp.pres_rk(3, 0, 0.5)
    for t, tt in zip(hp.s, hp.st):       # timeloop.exec() of the scalars; pres_rk has done u, v, w
        hp._ok(hp.lib.mhh_rk_substep(hp.G, 3, 0, 0.5, t.data_ptr(), tt.data_ptr(), hp.stream))
    hp.step()
    hp.sync()
    for n, t in zip(FIELDS, (hp.u, hp.v, hp.w, hp.s[0], hp.ut, hp.vt, hp.wt, hp.st[0], hp.p, hp.evisc)):
        a = t.detach().cpu().numpy()
        out[n] = a[:, g.jstart:g.jend, g.istart:g.iend].copy()
        if n in WITH_HALOS:
            out[n + "/all"] = a.copy()
    out["mask"] = hp.ib.mask.cpu().numpy()[:, g.jstart:g.jend, g.istart:g.iend].copy()
    out["k_dem"] = hp.ib.k_dem.cpu().numpy().copy()


def _worker(rank, world, out):
    hp = _make(B.get("emul").lib, npy=world, rank=rank)
    _results(hp, out)
    hp.close()


def _single(**kw):
    hp = _make(B.get("emul").lib, **kw)
    out = {"jgc": hp.grid.jgc}
    _results(hp, out)
    hp.close()
    return out


@pytest.fixture(scope="module")
def parts():
    return run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")


def test_the_ranks_lists_are_the_single_rank_lists(parts):
    single = _single()
    jmax = GRID[1]//len(parts)
    for loc in LOCS:
        # a rank finds its own rows' ghost cells in k-j-i order: sorted by (k, global j, i) the ranks' lists are the single-rank list
        rows = []
        for rank, p in enumerate(parts):
            for m in range(p["%s/i" % loc].size):
                rows.append((int(p["%s/k" % loc][m]), int(p["%s/j" % loc][m]) + rank*jmax, int(p["%s/i" % loc][m]), rank, m))
        rows.sort()
        assert len(rows) == single["%s/i" % loc].size > 0 and all(p["%s/i" % loc].size > 0 for p in parts)
        for k in R.LISTS:
            shift = lambda a, rank: a + rank*jmax if k in ("j", "ip_j") else a                                # noqa: E731
            got = np.stack([shift(parts[rank]["%s/%s" % (loc, k)][m], rank) for _, _, _, rank, m in rows])
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(single["%s/%s" % (loc, k)]).view(np.uint8)), (loc, k)
    # within rounding of the plain single-rank run (the bound of tests/test_slab_gloo.py:69-72); the mask bit for bit
    for n in FIELDS:
        got = np.concatenate([p[n] for p in parts], axis=1)
        scale = np.abs(single[n]).max()
        assert np.abs(got - single[n]).max() <= 1e-10*scale, (n, np.abs(got - single[n]).max()/scale)
    assert np.array_equal(np.concatenate([p["mask"] for p in parts], axis=1), single["mask"])


def test_two_ranks_are_one_rank_on_the_slab_path(parts):
    one = _single(force_slab=True)
    jgc, jmax = one["jgc"], GRID[1]//len(parts)
    for n in FIELDS + ("mask",):
        got = np.concatenate([p[n] for p in parts], axis=1)
        assert np.array_equal(got.view(np.uint8), one[n].view(np.uint8)), n
    # the halos: a rank's array, ghost rows and columns included, is rows [rank*jmax, rank*jmax + jcells) of the one rank's array
    for n in WITH_HALOS:
        for rank, p in enumerate(parts):
            a = p[n + "/all"]
            want = one[n + "/all"][:, rank*jmax:rank*jmax + a.shape[1], :]
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (n, rank)
    # k_dem's north-south halos came through the communicator
    k0, k1 = parts[0]["k_dem"], parts[1]["k_dem"]
    assert np.array_equal(k0[jgc+jmax:], k1[jgc:2*jgc]) and np.array_equal(k1[:jgc], k0[jmax:jmax+jgc])
    assert np.array_equal(k0, one["k_dem"][:jmax + 2*jgc]) and np.array_equal(k1, one["k_dem"][jmax:])
