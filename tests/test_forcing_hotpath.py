"""HotPath(..., forcing=Forcing(...)): the means the switches read and the fused Buffer + Force pass between rhs() and pres()
(src/model.cxx:351,395,404), on one rank (emulation and GPU) and slab-decomposed over two ranks (emulation over gloo)."""
import math

import numpy as np
import pytest

import backends as B
import common as cm
from common import same_bits as same
from ranks import run_ranks

GRID = (32, 24, 16)           # the grid of the smoke run: the smallest the suite builds a drycblles pressure plan on
U = 2.0**-53


def _forcing(g, kind):
    from microhh_amd.forcing import Forcing
    rs = np.random.RandomState(3)
    ug, vg = (rs.random_sample(g.kcells) * 2 - 1 for _ in range(2))
    if kind == "gabls1":      # geostrophic wind + Coriolis, the sponge relaxing to the mean profiles
        return Forcing(swbuffer=True, zstart=0.7 * g.zsize, swupdate=True, swlspres="geo", fc=1.39e-4, ug=ug, vg=vg, utrans=0.1, vtrans=-0.2)
    # fixed mass flux, and a nudged scalar so that a mean profile is read as well
    return Forcing(swlspres="uflux", uflux=0.11, utrans=0.07, nudgeprofs={"s0": 300. + rs.random_sample(g.kcells)}, nudge_factor=np.full(g.kcells, 1e-3))


def _hotpath(backend, **kw):
    from microhh_amd.model import HotPath
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    return HotPath("drycblles", *GRID, dt=0.37, **kw)


def _state(hp):
    return [t.detach().cpu().numpy().copy() for t in (hp.ut, hp.vt, hp.wt, hp.st[0], hp.p)]


@pytest.mark.parametrize("backend", cm.BACKENDS)
@pytest.mark.parametrize("kind", ["gabls1", "moser600"])
def test_step_with_forcing_equals_the_manual_sequence(backend, kind):
    out = {}
    for how in ("step", "manual"):
        hp = _hotpath(backend)
        hp.close()
        hp = _hotpath(backend, forcing=_forcing(hp.grid, kind))
        if how == "step":
            hp.step()
        else:
            hp.cyclic_prognostic(); hp.exec_viscosity(); hp.rhs()
            before = _state(hp)
            hp.forcing_means(); hp.buffer_force()
            assert not same(_state(hp)[0], before[0])            # the pass acts on ut
            hp.pres()
        hp.sync()
        out[how] = _state(hp)
        hp.close()
    for a, b, nm in zip(out["step"], out["manual"], ("ut", "vt", "wt", "st", "p")):
        assert same(a, b), (kind, nm, cm.ulp_diff(a, b))


@pytest.mark.parametrize("backend", cm.BACKENDS)
def test_forcing_none_is_the_step_as_it_was(backend):
    out = []
    for kw in ({}, {"forcing": None}):
        hp = _hotpath(backend, **kw)
        assert hp.forcing is None
        hp.step(); hp.sync()
        out.append(_state(hp))
        hp.close()
    for a, b in zip(*out):
        assert same(a, b)


def test_a_profile_the_library_would_skip_is_refused():
    """The sponge acts on every prognostic field, and w has no large-scale or nudging slot: bind() raises instead of leaving a
    field out silently."""
    from microhh_amd.forcing import Forcing
    g = cm.grid_2nd(*GRID)
    prof = np.zeros(g.kcells)
    with pytest.raises(ValueError, match="bufferprofs holds no profile for w, s0"):
        _hotpath("emul", forcing=Forcing(swbuffer=True, zstart=0.7 * g.zsize, bufferprofs={"u": prof, "v": prof}))
    for kw in ({"lsprofs": {"w": prof}}, {"nudgeprofs": {"s7": prof}, "nudge_factor": prof}):
        with pytest.raises(ValueError, match="not u, v or one of this case's scalars"):
            _hotpath("emul", forcing=Forcing(**kw))
    hp = _hotpath("emul", forcing=Forcing(swbuffer=True, zstart=0.7 * g.zsize, bufferprofs={n: prof for n in ("u", "v", "w", "s0")}))
    assert all((hp.forcing.bparams.abuf_u, hp.forcing.bparams.abuf_v, hp.forcing.bparams.abuf_w, hp.forcing.bparams.abuf_s[0]))
    hp.close()


# ---- two slab ranks on the emulation ---------------------------------------------------------------------------------------------
MEANS = (0.0123456789, 3.21e-4)      # the two volume sums handed to both sides, so that the pass is compared and not the reduction


def _run(hp, out):
    import torch
    g = hp.grid
    hp.cyclic_prognostic(); hp.exec_viscosity(); hp.rhs()
    hp.forcing_means()
    out["prof"] = hp.forcing.mean_prof["s0"].cpu().numpy().copy()
    out["sums"] = hp.forcing.sums.cpu().numpy().copy()
    # sum |fl(fld*dz)| of this rank's interior, for the summation-order bound on the two volume sums
    dz = g.dz[g.kstart:g.kend, None, None]
    out["abs"] = [float(np.abs(t[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy() * dz).sum(dtype=np.float64)) for t in (hp.u, hp.ut)]
    hp.forcing.sums.copy_(torch.tensor(MEANS, dtype=torch.float64))
    hp.buffer_force()
    out["ut"] = hp.ut[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()


def _worker(rank, world, out):
    from microhh_amd.model import HotPath, synthetic_global
    lib = B.get("emul").lib
    hp = HotPath("drycblles", *GRID, dt=0.37, device="cpu", lib=lib, npy=world, rank=rank, overlap=False,
                 global_init=synthetic_global("drycblles", *GRID), forcing=_forcing(cm.grid_2nd(*GRID), "moser600"))
    _run(hp, out)
    hp.close()


def test_two_slab_ranks_sum_their_shares_and_apply_the_same_body_force():
    from microhh_amd.model import HotPath, synthetic_global
    gi = synthetic_global("drycblles", *GRID)
    hp = HotPath("drycblles", *GRID, dt=0.37, device="cpu", lib=B.get("emul").lib, global_init=gi, forcing=_forcing(cm.grid_2nd(*GRID), "moser600"))
    g = hp.grid
    ref = {}
    _run(hp, ref)
    hp.close()
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")
    N = GRID[0] * GRID[1]
    n = N
    gam = (n - 1) * U / (1 - (n - 1) * U)
    for p in parts:
        assert same(p["prof"], parts[0]["prof"]) and same(p["sums"], parts[0]["sums"])        # every rank holds the global values
    for k in range(g.kstart, g.kend):
        x = gi["s0"][k - g.kstart]
        mean = math.fsum(float(v) for v in x.ravel()) / N
        bound = gam * math.fsum(abs(float(v)) for v in x.ravel()) / N + float(np.spacing(abs(mean)))
        assert abs(float(parts[0]["prof"][k]) - float(ref["prof"][k])) <= 2 * bound, (k, parts[0]["prof"][k], ref["prof"][k], bound)
    # the volume sums: both sides add the same n3 values fl(fld*dz) in another order, each within gamma(n3) * sum|x| of the exact
    # sum. 1.001 covers the rounding of sum|x| itself (n3 * 2^-53 relative).
    n3 = N * GRID[2]
    gam3 = (n3 - 1) * U / (1 - (n3 - 1) * U)
    for m in range(2):
        assert abs(ref["abs"][m] - sum(p["abs"][m] for p in parts)) <= 1e-9 * ref["abs"][m]     # the ranks hold the same cells
        bound = 2 * gam3 * 1.001 * ref["abs"][m]
        assert abs(float(parts[0]["sums"][m]) - float(ref["sums"][m])) <= bound, (m, parts[0]["sums"][m], ref["sums"][m], bound)
    got = np.concatenate([p["ut"] for p in parts], axis=1)
    assert same(got, ref["ut"])                                # the uflux tendency, bit for bit with the same two means
