"""HotPath(..., source=Sources([...]), decay=Decay({...})): decay and source between Buffer and Force (src/model.cxx:395-404).

With forcing=, source= and decay= together step() runs mhh_buffer_exec, decay, source, mhh_force_exec. On the emulation with the
reference tree the scalar tendencies are those of the oracle sequence, bit for bit: the library's Buffer pass, the REFERENCE's
Decay::exec and Source::exec loops on the host (the shim of tests/source_ref.py), the library's Force pass. Where the tree is absent,
and on the GPU, the same test only checks the ORDER of the calls: the library's own two passes are called by hand between the two
halves (their values are compared with the golden file in tests/test_source_exec.py). Without the two arguments the step is the step as it was: the digests below were taken from the commit
before the arguments existed. On the GPU a captured graph of the step replays to the bits of the plain step.
"""
import numpy as np
import pytest

import backends as B
import common as cm
import source_ref as R
from common import same_bits as same
from refshim import digest

GRID = (32, 24, 16)
NSC = 3
DT = 0.37
DECAY = {1: 600., 2: 0.1}            # 0.1 < DT: the dt branch


def _sources(g):
    X, Y, Z = g.xsize, g.ysize, g.zsize
    # strengths that show beside tendencies of O(1) in fp32
    return [dict(scalar=1, x0=0.5*X, y0=0.5*Y, z0=0.3*Z, sigma_x=250., sigma_y=300., sigma_z=120., strength=3e8),
            dict(scalar=1, x0=0.55*X, y0=0.45*Y, z0=0.35*Z, sigma_x=200., sigma_y=280., sigma_z=100., strength=1.5e7, swvmr=True),
            dict(scalar=2, x0=0.2*X, y0=0.7*Y, z0=0.5*Z, sigma_x=220., sigma_y=270., sigma_z=110., strength=2e9, line_x=0.4*X),
            dict(scalar=0, x0=60., y0=Y - 50., z0=40., sigma_x=200., sigma_y=270., sigma_z=90., strength=1e8),
            dict(scalar=2, x0=0.6*X, y0=0.3*Y, z0=0., sigma_x=300., sigma_y=300., sigma_z=1., strength=4e8, profile_index=0)]


def _forcing(g):
    from microhh_amd.forcing import Forcing
    rs = np.random.RandomState(3)
    ug, vg = (rs.random_sample(g.kcells)*2 - 1 for _ in range(2))
    return Forcing(swbuffer=True, zstart=0.7*g.zsize, swupdate=True, swlspres="geo", fc=1.39e-4, ug=ug, vg=vg, utrans=0.1, vtrans=-0.2,
                   nudgeprofs={"s1": rs.random_sample(g.kcells)}, nudge_factor=np.full(g.kcells, 1e-3))


def _hotpath(backend, dtype=np.float64, with_sources=True, **kw):
    from microhh_amd.model import HotPath, synthetic_global
    from microhh_amd.source import Sources, Decay
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    g = cm.grid_2nd(*GRID, dtype=dtype)
    if with_sources:
        prof = R.profiles_of(g)
        kw.update(source=Sources(_sources(g), profiles=prof), decay=Decay(DECAY))
    return HotPath("drycblles", *GRID, dt=DT, dtype=dtype, nscalars=NSC, global_init=synthetic_global("drycblles", *GRID, dtype=dtype, nscalars=NSC),
                   forcing=_forcing(g), **kw)


def _state(hp):
    return [t.detach().cpu().numpy().copy() for t in [hp.ut, hp.vt, hp.wt] + hp.st + [hp.p]]


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("backend", cm.BACKENDS)
def test_step_is_buffer_decay_source_force(backend, dtype):
    torch = pytest.importorskip("torch")
    hp = _hotpath(backend, dtype)
    assert hp.source.handle.tiles > 0
    hp.step(); hp.sync()
    got = _state(hp)
    hp.close()
    # the sequence by hand on a HotPath without the two modules: the oracle's where the reference is here, else the library's own passes
    hp = _hotpath(backend, dtype, with_sources=False)
    g = hp.grid
    hp.cyclic_prognostic(); hp.exec_viscosity(); hp.rhs()
    hp.forcing_means(); hp.forcing.exec_buffer(); hp.sync()
    by_reference = backend == "emul" and R.have_reference()
    if by_reference:
        ref = R.Ref(g, R.profiles_of(g), hp.rhoref_h)
        st = [t.detach().cpu().numpy().copy() for t in hp.st]
        for n, ts in DECAY.items():
            ref.decay(st[n], np.ascontiguousarray(hp.s[n].detach().cpu().numpy()), ts, DT)
        before = [a.copy() for a in st]
        ref.exec(_sources(g), st)
        assert all(not same(a, b) for a, b in zip(st, before))                    # every scalar receives a source
        for t, a in zip(hp.st, st):
            t.copy_(torch.from_numpy(a))
    else:
        from microhh_amd.source import Sources, Decay
        Decay(DECAY).bind(hp).exec()
        Sources(_sources(g), profiles=R.profiles_of(g)).bind(hp).exec()
    hp.forcing.exec_force()
    hp.pres(); hp.sync()
    want = _state(hp)
    hp.close()
    for a, b, nm in zip(got, want, ("ut", "vt", "wt", "st0", "st1", "st2", "p")):
        assert same(a, b), (nm, cm.ulp_diff(a, b))


# sha-256 of st0..2 after one step() of _hotpath("emul", with_sources=False), taken with the driver of the commit before source= and
# decay= existed, where the whole state (ut, vt, wt, st0..2, p) had the bits it has now. The fields are drawn by numpy's seeded
# legacy generator, so every host draws the same; the scalar tendencies pass through no transform and no libm call per cell.
DIGEST_BEFORE = {"f64": "9bf64cd7e0334be38826760c67356a57a5ae4d6f95dbe2c22bfe8d2ee62de5ac",
                 "f32": "2209377e6179e1a1c2d59c9e7157cd418a9093e4394f6dcfcdc052c9587cb6fc"}


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
def test_without_the_arguments_the_step_is_the_step_as_it_was(dtype):
    out = []
    for kw in ({}, {"source": None, "decay": None}):
        hp = _hotpath("emul", dtype, with_sources=False, **kw)
        assert hp.source is None and hp.decay is None
        hp.step(); hp.sync()
        out.append(_state(hp))
        hp.close()
    assert all(same(a, b) for a, b in zip(*out))
    assert digest(*out[1][3:6]) == DIGEST_BEFORE[R.tag(dtype)]


def test_decay_or_source_alone_and_without_forcing():
    """Either argument alone, and no forcing=: the stage still runs after the RHS."""
    from microhh_amd.model import HotPath
    from microhh_amd.source import Sources, Decay
    lib = B.get("emul").lib
    g = cm.grid_2nd(*GRID)
    base = HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC)
    base.step()
    a = HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, decay=Decay({0: 50.}))
    a.step()
    b = HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, source=Sources(_sources(g)[:1]))
    b.step()
    st = lambda hp, n: hp.st[n].numpy()           # noqa: E731
    assert not same(st(a, 0), st(base, 0)) and same(st(a, 1), st(base, 1)) and same(st(a, 2), st(base, 2))
    assert not same(st(b, 1), st(base, 1)) and same(st(b, 0), st(base, 0)) and same(st(b, 2), st(base, 2))
    rate = 1./50.
    it = base.grid.interior
    assert same(st(a, 0)[it], st(base, 0)[it] - rate*base.s[0].numpy()[it])
    with pytest.raises(ValueError, match="scalar 3 of 3"):
        HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, decay=Decay({3: 50.}))
    with pytest.raises(ValueError, match="scalar 5 of 3"):
        HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, source=Sources([dict(_sources(g)[0], scalar=5)]))
    for hp in (base, a, b):
        hp.close()


def test_update_between_steps_moves_the_emission():
    """hp.source.update(): the next step emits from the new place with the new strength, as a HotPath created with them does."""
    from microhh_amd.model import HotPath
    from microhh_amd.source import Sources
    lib = B.get("emul").lib
    g = cm.grid_2nd(*GRID)
    src = _sources(g)[:3]
    moved = [dict(s, x0=s["x0"] + 333., strength=2.*s["strength"]) for s in src]
    hp = HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, source=Sources(src))
    hp.source.update(None, x0=[s["x0"] for s in moved], strength=[s["strength"] for s in moved])
    hp.step()
    fresh = HotPath("drycblles", *GRID, dt=DT, device="cpu", lib=lib, nscalars=NSC, source=Sources(moved))
    fresh.step()
    for n in range(NSC):
        assert same(hp.st[n].numpy(), fresh.st[n].numpy())
    assert [hp.source.ranges(n) for n in range(3)] == [fresh.source.ranges(n) for n in range(3)]
    assert [hp.source.norm(n) for n in range(3)] == [fresh.source.norm(n) for n in range(3)]
    hp.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
def test_a_captured_step_with_sources_replays_to_the_same_bits(dtype):
    """mhh_decay_exec and mhh_source_exec only enqueue: a step with both, captured into a hipGraph and replayed from the same inputs,
    equals the step launched call by call (the pattern of tests/test_fullsize_gpu.py)."""
    import torch
    from microhh_amd.model import HotPath
    from microhh_amd.source import Sources, Decay
    g = cm.grid_2nd(*GRID, dtype=dtype)
    hp = HotPath("drycblles", *GRID, dt=DT, dtype=dtype, nscalars=NSC, source=Sources(_sources(g), profiles=R.profiles_of(g)), decay=Decay(DECAY))
    state = [hp.ut, hp.vt, hp.wt, hp.p, hp.evisc] + list(hp.st)
    init = [t.clone() for t in state]

    def reset():
        for t, k in zip(state, init):
            t.copy_(k)
    reset(); hp.step(); hp.sync()
    eager = [t.clone() for t in state]
    hp.source = hp.decay = None
    reset(); hp.step(); hp.sync()
    assert not any(torch.equal(a, b) for a, b in zip(state[-NSC:], eager[-NSC:]))        # the two stages act on every scalar
    hp.close()
    hp = HotPath("drycblles", *GRID, dt=DT, dtype=dtype, nscalars=NSC, source=Sources(_sources(g), profiles=R.profiles_of(g)), decay=Decay(DECAY))
    state = [hp.ut, hp.vt, hp.wt, hp.p, hp.evisc] + list(hp.st)
    graph = hp.capture_step()
    for rep in range(2):
        reset(); graph.replay(); hp.sync()
        assert all(torch.equal(a, b) for a, b in zip(state, eager)), rep
    hp.close()


@pytest.mark.gpu
def test_update_resets_the_graphs_captured_before_it():
    """A graph captured before update() holds the old tables' address and launch size: update() resets it, so a replay raises on
    the host instead of launching, and a new capture works."""
    from microhh_amd.model import HotPath
    from microhh_amd.source import Sources
    g = cm.grid_2nd(*GRID)
    src = _sources(g)[:3]
    hp = HotPath("drycblles", *GRID, dt=DT, nscalars=NSC, source=Sources(src))
    graph = hp.capture_step()
    hp.source.update(0, x0=src[0]["x0"] + 500.)
    with pytest.raises(RuntimeError):
        graph.replay()
    again = hp.capture_step()
    again.replay(); hp.sync()
    hp.close()
