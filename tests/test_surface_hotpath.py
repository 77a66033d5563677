"""HotPath(..., surface=Surface(...)): the surface layer and the vertical ghost cells between exec_viscosity and the RHS
(src/model.cxx:346-392), on one rank (emulation and GPU), as a captured graph (GPU), and slab-decomposed (emulation: two gloo
ranks, and one rank through the slab code path)."""
import numpy as np
import pytest

import backends as B
import common as cm
import surface_ref as S
from common import same_bits as same
from ranks import run_ranks

GRID = (32, 16, 12)
SBOT = 0.1                       # drycblles: sbot[th] = 0.1 K m/s with sbcbot = flux


def _surface(**kw):
    from microhh_amd.surface import Surface
    args = dict(mbcbot="noslip", ubot=S.UBOT, vbot=S.VBOT, sbcbot="flux", sbot=SBOT, z0m=S.Z0M, z0h=S.Z0H,
                thref_kstart=S.THREF, threfh_kstart=S.THREFH)
    args.update(kw)
    return Surface(**args)


def _hotpath(backend, surface=True, **kw):
    from microhh_amd.model import HotPath
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    if surface:
        kw["surface"] = _surface()
    return HotPath("drycblles", *GRID, dt=0.37, **kw)


def _tend(hp):
    hp.sync()
    return {n: t.detach().cpu().numpy().copy() for n, t in (("ut", hp.ut), ("vt", hp.vt), ("wt", hp.wt), ("st", hp.st[0]), ("p", hp.p), ("evisc", hp.evisc))}


def _staged_step(hp):
    """step() spelled out with the library's own stage entry points."""
    hp.cyclic_prognostic(); hp.exec_viscosity()
    hp.surface.staged(); hp.surface.ghost_cells()
    hp.rhs(); hp.pres()


def _reference_step(hp, st, table):
    """The same sub-step on a HotPath WITHOUT surface=: the reference's Boundary_surface::exec on the host writes the arrays the
    operators read, and the same mhh_boundary_ghost_cells calls set the ghost cells from its gradients."""
    import torch
    g, lib = hp.grid, hp.lib
    hp.cyclic_prognostic(); hp.exec_viscosity(); hp.sync()
    case = S.SurfCase("flux", S.SMALL, g.np_dtype); case.g = g
    lev = lambda t: np.ascontiguousarray(t[g.kstart].cpu().numpy())                                          # noqa: E731
    inp = {"u": lev(hp.u), "v": lev(hp.v), "s0": lev(hp.s[0]), "sbot0": np.zeros(g.shape2), "sfluxbot0": np.full(g.shape2, SBOT)}
    r = S.ref_exec(case, inp, st, table)
    for k, name in (("u_fluxbot", "ufluxbot"), ("v_fluxbot", "vfluxbot"), ("dudz", "dudz"), ("dvdz", "dvdz"), ("dbdz", "dbdz")):
        hp.surf[k].copy_(torch.from_numpy(r[name]))
    hp.surf["s_fluxbot"].copy_(torch.from_numpy(r["sfluxbot0"]))
    t2 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hp.device)                                   # noqa: E731
    zero = torch.zeros(g.shape2, dtype=hp.td, device=hp.device)
    keep = [t2(np.full(g.shape2, S.UBOT)), t2(np.full(g.shape2, S.VBOT)), t2(r["sgradbot0"]), zero]
    gc = lib.mhh_boundary_ghost_cells
    for a, bot in ((hp.u, keep[0]), (hp.v, keep[1])):                  # noslip below, freeslip (zero gradient) above
        B.ok(B.get("emul"), gc(hp.G, 2, a.data_ptr(), 0, 1, bot.data_ptr(), None, zero.data_ptr(), zero.data_ptr(), hp.stream))
    B.ok(B.get("emul"), gc(hp.G, 2, hp.s[0].data_ptr(), 1, 1, None, keep[2].data_ptr(), zero.data_ptr(), zero.data_ptr(), hp.stream))
    hp.rhs(); hp.pres()
    return r


def test_two_steps_equal_the_reference_surface_layer_wired_by_hand():
    """emul, bit for bit: the wiring and the order. Where the reference tree is absent the by-hand run uses the library's stages."""
    hp = _hotpath("emul")
    hp.step(); first = hp.surface.outputs(); hp.step()
    got, surf = _tend(hp), hp.surface.outputs()
    assert not same(first["nobuk"], np.zeros_like(first["nobuk"]))                 # the walk moved, and the second call started from it
    hp.close()
    if S.have_reference():
        ref = _hotpath("emul", surface=False)
        ref.surf["s_fluxbot"].fill_(SBOT)
        case = S.SurfCase("flux", S.SMALL, np.float64); case.g = ref.grid
        table = S.lut(S.shim().ref_surface_lut, ref.grid, S.DIRICHLET, S.FLUX)
        st = case.state()
        for _ in range(2):
            r = _reference_step(ref, st, table)
        g = ref.grid
        core = (slice(g.jstart, g.jend), slice(g.istart, g.iend))
        for k in ("dutot", "ustar", "obuk", "nobuk", "ufluxbot", "vfluxbot", "sbot0", "sgradbot0", "ugradbot", "vgradbot"):
            assert same(surf[k], r[k]), k
        for k in ("dudz", "dvdz", "dbdz"):                    # written on the interior only, by both
            assert same(surf[k][core], r[k][core]), k
    else:
        ref = _hotpath("emul")
        _staged_step(ref); _staged_step(ref)
    want = _tend(ref)
    ref.close()
    for k in got:
        assert same(got[k], want[k]), (k, cm.ulp_diff(got[k], want[k]))


def test_the_surface_layer_changes_the_step_and_its_absence_does_not():
    """surface=None is the step as it was; with it the tendencies differ (the synthetic surface arrays are no longer what is read)."""
    out = []
    for kw in (dict(surface=False), dict(surface=False, ), dict(surface=True)):
        hp = _hotpath("emul", **kw)
        assert (hp.surface is not None) == kw["surface"]
        hp.step(); out.append(_tend(hp)); hp.close()
    assert all(same(out[0][k], out[1][k]) for k in out[0])
    assert not same(out[0]["ut"], out[2]["ut"]) and not same(out[0]["st"], out[2]["st"])


@pytest.mark.gpu
def test_two_steps_equal_the_staged_entry_points_on_the_gpu():
    a, b = _hotpath("hip"), _hotpath("hip")
    a.step(); a.step()
    _staged_step(b); _staged_step(b)
    ta, tb, sa, sb = _tend(a), _tend(b), a.surface.outputs(), b.surface.outputs()
    a.close(); b.close()
    for k in ta:
        assert same(ta[k], tb[k]), k
    for k in sa:
        assert same(sa[k], sb[k]), k
    assert np.isfinite(sa["ustar"]).all() and (sa["nobuk"] > 0).any()


@pytest.mark.gpu
def test_a_captured_step_with_the_surface_layer_replays_one_step():
    a, b = _hotpath("hip"), _hotpath("hip")
    graph = a.capture_step()                      # runs one step, then records one
    graph.replay()
    b.step(); b.step()
    ta, tb, sa, sb = _tend(a), _tend(b), a.surface.outputs(), b.surface.outputs()
    a.close(); b.close()
    for k in ta:
        assert same(ta[k], tb[k]), k
    for k in sa:
        assert same(sa[k], sb[k]), k


def test_bind_raises_on_what_the_library_refuses():
    from microhh_amd.model import HotPath
    lib = B.get("emul").lib
    for kw, word in ((dict(swconstantz0=False), "swconstantz0"), (dict(swcharnock=True), "swcharnock")):
        with pytest.raises(ValueError, match=word):
            HotPath("drycblles", *GRID, device="cpu", lib=lib, surface=_surface(**kw))
    with pytest.raises(ValueError, match="igc >= 2"):
        HotPath("taylorgreen", 16, 16, 8, device="cpu", lib=lib, surface=_surface(thermo="0"))      # gc (1, 1, 1)


# ---- the slab ------------------------------------------------------------------------------------------------------------------
def _surface_rows(hp):
    g = hp.grid
    out = {k: v[g.jstart:g.jend, g.istart:g.iend] for k, v in hp.surface.outputs().items()}
    # evisc of the second step has read the first step's dudz, dvdz, dbdz. (The tendencies after pres() are not compared: the slab
    # pressure solve is another sequence of transforms than the one-rank solve, tests/test_slab_gloo.py.)
    out["evisc"] = _tend(hp)["evisc"][g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend]
    return out


def _worker(rank, world, out):
    from microhh_amd.model import HotPath, synthetic_global
    hp = HotPath("drycblles", *GRID, dt=0.37, device="cpu", lib=B.get("emul").lib, npy=world, rank=rank,
                 global_init=synthetic_global("drycblles", *GRID), surface=_surface())
    hp.step(); hp.step()
    out.update(_surface_rows(hp))
    hp.close()


def test_slab_ranks_give_the_one_rank_surface_layer():
    """Two gloo ranks, and one rank through the slab code path: every surface output, and the eddy viscosity that read them, gathered
    over the ranks, is the one-rank run bit for bit. nobuk is never exchanged: a ghost row's walk has the history of its image."""
    from microhh_amd.model import HotPath, synthetic_global
    gi = synthetic_global("drycblles", *GRID)
    one = {}
    for slab in (False, True):
        hp = HotPath("drycblles", *GRID, dt=0.37, device="cpu", lib=B.get("emul").lib, global_init=gi, force_slab=slab, surface=_surface())
        hp.step(); hp.step()
        one[slab] = _surface_rows(hp)
        hp.close()
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo")
    for k, want in one[False].items():
        ax = want.ndim - 2
        assert same(one[True][k], want), ("force_slab", k)
        assert same(np.concatenate([p[k] for p in parts], axis=ax), want), ("two ranks", k)


# ---- mbcbot = ustar: the ghost cells leave the bottom level of u and v alone (bc -1) --------------------------------------------
@pytest.mark.parametrize("backend", cm.BACKENDS)
def test_ustar_runs_through_hotpath_and_leaves_the_bottom_ghost_level_of_u_and_v_alone(backend):
    """Boundary_type::Ustar_type matches neither branch of the reference's calc_ghost_cells_bot (src/boundary.cxx:686-710): with
    bc -1 mhh_boundary_ghost_cells writes the top level only, and what it writes there is what bc 0 / 1 below would have left."""
    from microhh_amd.model import HotPath
    kw = dict(device="cpu", lib=B.get("emul").lib) if backend == "emul" else {}
    mk = lambda: HotPath("drycblles", *GRID, dt=0.37, surface=_surface(mbcbot="ustar", ustar=0.3), **kw)      # noqa: E731
    a, b = mk(), mk()
    g = a.grid
    a.cyclic_prognostic(); a.sync()
    before = {n: t.detach().cpu().numpy().copy() for n, t in (("u", a.u), ("v", a.v), ("th", a.s[0]))}
    a.step(); a.step()
    _staged_step(b); _staged_step(b)
    ta, tb, sa, sb = _tend(a), _tend(b), a.surface.outputs(), b.surface.outputs()
    after = {n: t.detach().cpu().numpy().copy() for n, t in (("u", a.u), ("v", a.v), ("th", a.s[0]))}
    # the same top level from a call with a Dirichlet bottom: only the bottom level may differ
    lib, be = a.lib, B.get(backend)
    u2 = a.u.clone()
    B.ok(be, lib.mhh_boundary_ghost_cells(a.G, 2, u2.data_ptr(), 0, 1, a.surface.ubot_t.data_ptr(), None, None, a.surface.utop_t.data_ptr(), a.stream))
    a.sync()
    u2 = u2.detach().cpu().numpy()
    a.close(); b.close()
    ks, ke = g.kstart, g.kend
    for n in ("u", "v"):
        assert same(after[n][ks-1], before[n][ks-1]), n                      # bottom ghost level untouched
        assert same(after[n][ke], after[n][ke-1])                            # freeslip top: zero gradient
        assert same(after[n][ks:ke], before[n][ks:ke])
    assert same(u2[ke], after["u"][ke]) and not same(u2[ks-1], after["u"][ks-1])
    assert not same(after["th"][ks-1], before["th"][ks-1])                   # the flux scalar's ghost level comes from surfs' gradient
    assert (sa["ustar"] == sa["ustar"].flat[0]).all() and sa["ustar"].flat[0] == np.float64(0.3)     # fixed ustar is not overwritten
    assert np.isfinite(sa["obuk"]).all() and np.isfinite(sa["ufluxbot"][g.jstart:g.jend, g.istart:g.iend]).all()
    for k in ta:
        assert same(ta[k], tb[k]), k
    for k in sa:
        assert same(sa[k], sb[k]), k
