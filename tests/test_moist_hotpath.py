"""HotPath("bomex", ..., thermo=Moist(pbot)): Thermo_moist in the sub-step -- the means of thl and qt, exec_viscosity with N2 from
thl and thvref, the base state on the device, the buoyancy tendency in front of the RHS pass (src/model.cxx:346-392) -- on one
rank, on the emulation and on the GPU, and as a captured graph (GPU)."""
import numpy as np
import pytest

import backends as B
import common as cm
from common import same_bits as same

GRID = (32, 8, 24)
PBOT = 101500.
BACKENDS = [pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)]


def _forcing(g):
    """BOMEX's large-scale terms in kind: subsidence on the mean profiles and a drying tendency of qt (both scalars' means are read)."""
    from microhh_amd.forcing import Forcing
    z = g.z.astype(np.float64)
    wls = -0.0065*np.minimum(z/1500., 1.)*np.clip((2100. - z)/600., 0., 1.)
    return Forcing(swwls="mean", wls=wls, lsprofs={"s1": -1.2e-8*np.clip((500. - z)/200. + 1., 0., 1.)})


def _hotpath(backend, moist=True, forcing=False, surface=False, **kw):
    from microhh_amd.model import HotPath
    from microhh_amd.surface import Surface
    from microhh_amd.thermo import Moist
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    args = dict(swupdatebasestate=kw.pop("update", True))
    if moist:
        kw["thermo"] = Moist(PBOT, **args)
    if surface:           # BOMEX: fixed ustar and the two surface fluxes; the moist hooks where thermo= is bound
        kw["surface"] = Surface(mbcbot="ustar", ustar=0.28, sbcbot="flux", sbot=[8e-3, 5.2e-5])
    if forcing:
        kw["forcing"] = _forcing(cm.Grid(*GRID, 6400., 6400., 3000., order=2, igc=3, jgc=3, kgc=1))
    return HotPath("bomex", *GRID, dt=0.37, **kw)


def _state(hp):
    hp.sync()
    out = {n: t.detach().cpu().numpy().copy() for n, t in (("ut", hp.ut), ("vt", hp.vt), ("wt", hp.wt), ("st0", hp.st[0]), ("st1", hp.st[1]),
                                                            ("p", hp.p), ("evisc", hp.evisc))}
    if hp.thermo is not None:
        out.update({n: t.detach().cpu().numpy().copy() for n, t in hp.thermo.tab.items()})
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("forcing,surface", [(False, False), (True, False), (True, True)], ids=["plain", "forcing", "forcing-surface"])
def test_step_equals_the_calls_issued_by_hand(backend, forcing, surface):
    out = {}
    for how in ("step", "manual"):
        hp = _hotpath(backend, forcing=forcing, surface=surface)
        assert (hp.surface is None) == (not surface) and (not surface or hp.surface.kind == 3)
        th = hp.thermo
        for _ in range(2):
            if how == "step":
                hp.step()
                continue
            hp.cyclic_prognostic()
            shared = th.means()
            assert shared == forcing                 # one evaluation of the means where Forcing reads both
            hp.exec_viscosity()
            th.update_base_state()
            before = hp.wt.clone()
            th.tend()
            assert not bool((hp.wt == before).all())
            if surface:
                hp.surface_layer()
            hp.rhs()
            if forcing:
                if not shared:
                    hp.forcing_means()
                hp.buffer_force()
            hp.pres()
        out[how] = _state(hp)
        if surface:
            out[how].update(hp.surface.outputs())
            assert np.isfinite(out[how]["obuk"]).all() and np.count_nonzero(out[how]["dbdz"]) > 0
        th.check()
        hp.close()
    for k in out["step"]:
        assert same(out["step"][k], out["manual"][k]), k


@pytest.mark.parametrize("backend", BACKENDS)
def test_tendency_before_the_rhs_and_the_base_state_update(backend):
    """swupdatebasestate off: wt in front of the RHS is the stand-alone tendency on the creation-time tables, and the tables stay.
    On: the second step's tables differ from the creation-time ones (the means are not the initial profiles), rhoref does not."""
    from microhh_amd import capi
    hp = _hotpath(backend, update=False)
    th, g = hp.thermo, hp.grid
    tab0 = {n: t.clone() for n, t in th.tab.items()}
    rho0 = hp.rhoref.clone()
    hp.cyclic_prognostic(); hp.exec_viscosity()
    want = hp.wt.clone()
    cnt = hp.torch.zeros(1, dtype=hp.torch.int32, device=hp.device)
    capi.check(hp.lib.mhh_thermo_moist_buoyancy_tend_impl(hp.G, 1, want.data_ptr(), hp.s[0].data_ptr(), hp.s[1].data_ptr(), tab0["prefh"].data_ptr(),
                                                          tab0["exnrefh"].data_ptr(), tab0["thvrefh"].data_ptr(), cnt.data_ptr(), hp.stream), hp.lib)
    hp.thermo_moist(); hp.sync()
    assert same(hp.wt.cpu().numpy(), want.cpu().numpy())
    assert all(bool((th.tab[n] == tab0[n]).all()) for n in tab0)
    ql = th.field("ql"); n2 = th.field("N2"); b = th.field("b")
    assert float(ql.max()) > 0 and float(ql.min()) == 0 and bool(hp.torch.isfinite(n2[g.kstart:g.kend]).all()) and float(b.abs().max()) > 0
    with pytest.raises(ValueError, match="get_thermo_field"):
        th.field("thv")
    th.check(); hp.close()
    hp = _hotpath(backend)
    th = hp.thermo
    hp.step(); hp.step(); hp.sync()
    assert not bool((th.tab["thvrefh"] == tab0["thvrefh"]).all()) and not bool((th.tab["prefh"] == tab0["prefh"]).all())
    assert bool((hp.rhoref == rho0).all())                       # fields.rhoref: set once
    assert bool(hp.torch.isfinite(th.tab["thvrefh"][g.kstart:g.kend+1]).all())
    th.check(); hp.close()


@pytest.mark.gpu
def test_captured_step_replays_the_eager_step():
    eager = _hotpath("hip", forcing=True, surface=True)
    eager.step(); eager.step()
    want = _state(eager); eager.thermo.check(); eager.close()
    hp = _hotpath("hip", forcing=True, surface=True)
    graph = hp.capture_step()            # runs one eager step first
    graph.replay()
    got = _state(hp); hp.thermo.check(); hp.close()
    for k in want:
        assert same(got[k], want[k]), k


def test_refusals_name_their_reason():
    from microhh_amd.model import HotPath
    from microhh_amd.surface import Surface
    from microhh_amd.thermo import Moist
    kw = dict(device="cpu", lib=B.get("emul").lib)
    with pytest.raises(ValueError, match="two scalars"):
        HotPath("bomex", *GRID, nscalars=1, thermo=Moist(PBOT), **kw)
    with pytest.raises(ValueError, match="two scalars"):
        HotPath("drycblles", *GRID, thermo=Moist(PBOT), **kw)
    with pytest.raises(ValueError, match="second order only"):
        HotPath("moser600", 16, 12, 12, nscalars=2, thermo=Moist(PBOT), **kw)
    with pytest.raises(ValueError, match="thvref0"):
        Moist(PBOT, swbasestate="boussinesq")
    with pytest.raises(ValueError, match="another kind of bottom bc"):
        HotPath("bomex", *GRID, thermo=Moist(PBOT), surface=Surface(mbcbot="noslip", sbcbot=["flux", "dirichlet"], sbot=[8e-3, 0.017]), **kw)
    with pytest.raises(ValueError, match="thermo = moist needs"):
        HotPath("bomex", *GRID, surface=Surface(mbcbot="ustar", ustar=0.28, sbcbot="flux", sbot=[8e-3, 5.2e-5], thermo="moist"), **kw)


@pytest.mark.parametrize("backend", BACKENDS)
def test_self_check_of_the_step_is_no_worse_with_the_thermodynamics(backend):
    """max |Pres::input| after the solve, as bench.py's self_check computes it, with and without thermo=. The residual is the
    solve's rounding, and it varies from run to run with the synthetic fields: the same case is run with four seeds without thermo=,
    and the factor between the largest and the smallest of the four residuals is the variation. The run with thermo= (first seed)
    must not exceed the plain run of the same seed by more than that factor. Repeating a run with one seed gives the same bits, so
    that repetition shows no variation at all. Measured at 32 x 8 x 24, fp64 (plain per seed; with thermo; factor):
      emulation  1.232e-16 8.903e-17 1.013e-16 1.347e-16;  1.373e-16;  1.513
      MI355X     2.978e-17 2.792e-17 2.762e-17 2.615e-17;  3.184e-17;  1.139"""
    seeds = (666, 667, 668, 669)
    plain = []
    for seed in seeds:
        hp = _hotpath(backend, moist=False, seed=seed)
        hp.step(); plain.append(hp.projected_divergence()[0]); hp.close()
    hp = _hotpath(backend, seed=seeds[0])
    hp.step(); moist, scale = hp.projected_divergence(); hp.close()
    factor = max(plain)/min(plain)
    print("max|Pres::input| after the solve on %s: plain %s, with thermo %.3e, factor %.3f (scale %.3e)"
          % (backend, " ".join("%.3e" % v for v in plain), moist, factor, scale))
    assert moist <= factor*plain[0]


# ---- two slab ranks ---------------------------------------------------------------------------------------------------------
def _exact_init():
    """synthetic_global's BOMEX fields narrowed to values a float holds: with 32 x 8 = 256 columns the double sums of a level are
    then exact in any order and the division by 256 is exact, so the mean profiles -- and with them the tables and wt -- do not
    depend on how the rows are dealt to the ranks. (A general field's means agree only to rounding between one rank and two:
    tests/test_forcing_hotpath.py bounds that.)"""
    from microhh_amd.model import synthetic_global
    gi = synthetic_global("bomex", *GRID)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in gi.items()}


def _slab_run(hp, out):
    g = hp.grid
    for _ in range(2):           # the second round starts from the tables the first one left
        hp.cyclic_prognostic(); hp.thermo.means(); hp.exec_viscosity(); hp.thermo_moist()
    hp.sync()
    out["wt"] = hp.wt[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()
    for n, t in hp.thermo.tab.items():
        out[n] = t.cpu().numpy().copy()
    out["thlmean"] = hp.thermo.mean[0].cpu().numpy().copy()
    hp.thermo.check()


def _worker(rank, world, out):
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    hp = HotPath("bomex", *GRID, dt=0.37, device="cpu", lib=B.get("emul").lib, npy=world, rank=rank, overlap=False,
                 global_init=_exact_init(), thermo=Moist(PBOT))
    _slab_run(hp, out)
    hp.close()


def test_two_slab_ranks_give_the_bits_of_one():
    """N = 2 against N = 1 with base-state updates on: the ranks sum their shares of the means through Master, every rank holds the
    same tables, and wt in front of the RHS and the tables have the single rank's bits."""
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    from ranks import run_ranks
    hp = HotPath("bomex", *GRID, dt=0.37, device="cpu", lib=B.get("emul").lib, global_init=_exact_init(), thermo=Moist(PBOT))
    ref = {}
    _slab_run(hp, ref)
    from microhh_amd import thermo
    g = hp.grid
    created = thermo.base_state(hp.lib, g, *thermo.bomex_profiles(g.z[g.kstart:g.kend]), PBOT)["thvrefh"]
    hp.close()
    assert not same(ref["thvrefh"], created)                      # the update moved the tables
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")
    for k in ref:
        if k == "wt":
            assert same(np.concatenate([p["wt"] for p in parts], axis=1), ref["wt"])
        else:
            for p in parts:
                assert same(p[k], ref[k]), k
