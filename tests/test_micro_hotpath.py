"""HotPath("rico", ..., thermo=Moist(pbot), micro=Warm2mom(Nc0)): Microphys_2mom_warm::exec behind thermo->exec and Limiter::exec
behind the pressure solve (src/model.cxx:369, :415) -- on one rank, on the emulation and on the GPU, as a captured graph (GPU), and
on two slab ranks against one."""
import numpy as np
import pytest

import backends as B
from common import same_bits as same

GRID = (64, 8, 32)
PBOT = 101540.
NC0 = 70.e6
DT_FULL = 6.
BACKENDS = [pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)]


def _hotpath(backend, micro=True, **kw):
    from microhh_amd.microphys import Warm2mom
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    if micro:
        kw["micro"] = Warm2mom(NC0, dt=DT_FULL)
    return HotPath("rico", *GRID, dt=2., thermo=Moist(PBOT), **kw)


def _state(hp):
    hp.sync()
    named = [("ut", hp.ut), ("vt", hp.vt), ("wt", hp.wt), ("p", hp.p), ("qr", hp.s[2]), ("nr", hp.s[3])] + [("st%d" % n, t) for n, t in enumerate(hp.st)]
    if hp.micro is not None:
        named.append(("rr_bot", hp.micro.rain_rate()))
    return {n: t.detach().cpu().numpy().copy() for n, t in named}


@pytest.mark.parametrize("backend", BACKENDS)
def test_step_equals_the_calls_issued_by_hand(backend):
    out = {}
    for how in ("step", "manual"):
        hp = _hotpath(backend)
        th, mi, g = hp.thermo, hp.micro, hp.grid
        assert mi.dt == DT_FULL and hp.dt == 2. and len(hp.s) == 4
        for _ in range(2):
            if how == "step":
                hp.step()
                continue
            hp.cyclic_prognostic()
            th.means()
            hp.exec_viscosity()
            hp.thermo_moist()
            before = [t.clone() for t in hp.st]
            mi.exec()
            assert all(not bool((a == b).all()) for a, b in zip(before, hp.st))          # every one of the four tendencies moved
            hp.rhs()
            hp.pres()
            before = [t.clone() for t in hp.st]
            mi.limit()
            assert all(bool((a == b).all()) == (n < 2) for n, (a, b) in enumerate(zip(before, hp.st)))      # limitlist = qr, nr
        out[how] = _state(hp)
        rr = out[how]["rr_bot"][g.jstart:g.jend, g.istart:g.iend]
        assert (rr >= 0).all() and 0.2 < np.count_nonzero(rr)/rr.size < 0.8 and np.isfinite(out[how]["st3"]).all()
        assert (out[how]["qr"][g.interior] >= 0).all()
        th.check()
        hp.close()
    for k in out["step"]:
        assert same(out["step"][k], out["manual"][k]), k


@pytest.mark.parametrize("backend", BACKENDS)
def test_without_micro_the_four_scalars_are_plain_scalars(backend):
    """micro= off: the step of the same fields leaves qr and nr as they were, negative values included, and calls neither entry."""
    hp = _hotpath(backend, micro=False)
    assert hp.micro is None
    hp.s[2][hp.grid.kstart, hp.grid.jstart, hp.grid.istart] = -1e-6
    qr0 = hp.s[2].clone()
    hp.step(); hp.sync()
    g = hp.grid
    assert bool((hp.s[2][g.interior] == qr0[g.interior]).all())
    hp.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_time_limit_and_forms(backend):
    """get_time_limit: idt * cflmax / cfl in the dtype, truncated; the two forms of exec give the same bits through the driver."""
    from microhh_amd import capi
    import ctypes as C
    hp = _hotpath(backend)
    mi = hp.micro
    cfl = mi.cfl(DT_FULL)
    out = C.c_double(0)
    capi.check(hp.lib.mhh_micro_2mom_warm_cfl(hp.G, hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.rhoref.data_ptr(), DT_FULL, hp.work.data_ptr(),
                                              C.byref(out), hp.stream), hp.lib)
    assert cfl == out.value and 1e-5 < cfl < 9.65*DT_FULL/125. + 1e-9           # dz = 125 m, w <= 9.65 m/s
    idt = 6000000000
    assert mi.time_limit(idt, DT_FULL) == int(np.float64(idt)*np.float64(2.)/np.float64(cfl))
    hp.cyclic_prognostic(); hp.thermo.means(); hp.exec_viscosity(); hp.thermo_moist()
    saved = [t.clone() for t in hp.st] + [hp.s[2].clone(), hp.s[3].clone()]
    res = {}
    for impl in (0, 1):
        for t, s in zip(hp.st + hp.s[2:4], saved):
            t.copy_(s)
        mi.exec(impl)
        res[impl] = _state(hp)
    for k in res[0]:
        assert same(res[0][k], res[1][k]), k
    hp.thermo.check(); hp.close()


@pytest.mark.gpu
def test_captured_step_replays_the_eager_step():
    eager = _hotpath("hip")
    eager.step(); eager.step()
    want = _state(eager); eager.thermo.check(); eager.close()
    hp = _hotpath("hip")
    graph = hp.capture_step()            # runs one eager step first
    graph.replay()
    got = _state(hp); hp.thermo.check(); hp.close()
    for k in want:
        assert same(got[k], want[k]), k


def test_refusals_name_their_reason():
    from microhh_amd.microphys import Warm2mom
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    kw = dict(device="cpu", lib=B.get("emul").lib)
    with pytest.raises(ValueError, match="needs thermo=Moist"):
        HotPath("rico", *GRID, micro=Warm2mom(NC0), **kw)
    with pytest.raises(ValueError, match="four scalars"):
        HotPath("bomex", 32, 8, 24, thermo=Moist(101500.), micro=Warm2mom(NC0), **kw)
    with pytest.raises(ValueError, match="four scalars"):
        HotPath("rico", *GRID, nscalars=5, thermo=Moist(PBOT), micro=Warm2mom(NC0), **kw)
    with pytest.raises(ValueError, match="Nc0"):
        Warm2mom(0.)
    with pytest.raises(ValueError, match="limit"):
        Warm2mom(NC0, limit=("qr", "qi"))


# ---- two slab ranks ---------------------------------------------------------------------------------------------------------
def _exact_init():
    """synthetic_global's RICO fields narrowed to values a float holds: the level sums of thl and qt over 64 x 8 = 512 columns are
    then exact in any order, so the mean profiles and the tables do not depend on how the rows are dealt to the ranks
    (tests/test_moist_hotpath.py)."""
    from microhh_amd.model import synthetic_global
    gi = synthetic_global("rico", *GRID)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in gi.items()}


def _slab_run(hp, out):
    g = hp.grid
    for _ in range(2):
        hp.cyclic_prognostic(); hp.thermo.means(); hp.exec_viscosity(); hp.thermo_moist(); hp.micro.exec(); hp.micro.limit()
    hp.sync()
    for n in range(4):
        out["st%d" % n] = hp.st[n][g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()
    out["rr_bot"] = hp.micro.rain_rate()[g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()
    out["limit"] = np.array([hp.micro.time_limit(6000000000, DT_FULL)])
    out["cfl"] = np.array([hp.micro.cfl(DT_FULL)])
    hp.thermo.check()


def _worker(rank, world, out):
    from microhh_amd.microphys import Warm2mom
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    gi = _exact_init()
    hp = HotPath("rico", *GRID, dt=2., device="cpu", lib=B.get("emul").lib, npy=world, rank=rank, overlap=False,
                 global_init=gi, thermo=Moist(PBOT), micro=Warm2mom(NC0, dt=DT_FULL))
    _slab_run(hp, out)
    out["local_cfl"] = np.array([_local_cfl(hp)])
    hp.close()


def _local_cfl(hp):
    import ctypes as C
    from microhh_amd import capi
    o = C.c_double(0)
    capi.check(hp.lib.mhh_micro_2mom_warm_cfl(hp.G, hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.rhoref.data_ptr(), DT_FULL, hp.work.data_ptr(),
                                              C.byref(o), hp.stream), hp.lib)
    return o.value


def test_two_slab_ranks_give_the_bits_of_one():
    """N = 2 against N = 1: the four tendencies behind microphys->exec and limiter->exec, the rain rate, the CFL number and the time
    limit (the maximum over the ranks through Master) have the single rank's bits; nothing else is exchanged."""
    from microhh_amd.microphys import Warm2mom
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    from ranks import run_ranks
    hp = HotPath("rico", *GRID, dt=2., device="cpu", lib=B.get("emul").lib, global_init=_exact_init(), thermo=Moist(PBOT),
                 micro=Warm2mom(NC0, dt=DT_FULL))
    ref = {}
    _slab_run(hp, ref)
    hp.close()
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")
    for k in ("st0", "st1", "st2", "st3", "rr_bot"):
        assert same(np.concatenate([p[k] for p in parts], axis=-2), ref[k]), k
    for p in parts:
        assert p["limit"][0] == ref["limit"][0] and p["cfl"][0] == ref["cfl"][0]
    assert max(p["local_cfl"][0] for p in parts) == ref["cfl"][0]
