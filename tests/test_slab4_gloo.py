"""The 4th-order cases (advec_4 + diff_4 + pres_4: moser600) on the N > 1 path, on the CPU: world_size 2 and 4 over gloo, kernels
= the library's own sources executed by the test-only HIP stand-in (tests/emul). Every run is compared with the single-rank run on
the same global synthetic fields: RHS tendencies bit-exact, pressure-corrected tendencies and p to 1e-10 (the transform is split x / y
instead of 2-D, the 7-band solve multiplies by reciprocal pivots). nxh = 9 modes do not divide by 2 or 4 ranks: the padded x-mode
blocks are part of every run. One rank of the slab path is also checked against the oracle's Pres_4 input -> solve -> output."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
from common import ptr, dbl
from microhh_amd import capi
from microhh_amd.model import HotPath, synthetic_global
from ranks import run_ranks

CASE = "moser600"
GRID = (16, 32, 12)        # world 4: jmax = 8; nxh = 9


def _interior(hp, t):
    g = hp.grid
    return t[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].numpy().copy()


def _rhs(hp):
    hp.cyclic_prognostic()
    hp.exec_viscosity()
    hp.rhs()


def _run(hp, out):
    _rhs(hp)
    for n in ("ut", "vt", "wt"):
        out["rhs_" + n] = _interior(hp, getattr(hp, n))
    hp.pres()
    for n in ("ut", "vt", "wt", "p"):
        out[n] = _interior(hp, getattr(hp, n))
    out["div"] = np.array(hp.divergence())
    out["cfl"] = np.array(hp.cfl(0.5))


def _single(dtype=np.float64, **kw):
    lib = B.get("emul").lib
    out = {}
    hp = HotPath(CASE, *GRID, device="cpu", lib=lib, dtype=dtype, global_init=synthetic_global(CASE, *GRID, dtype=dtype), **kw)
    _run(hp, out)
    hp.close()
    return out


def _worker(rank, world, out, chunks, dtype):
    lib = B.get("emul").lib
    hp = HotPath(CASE, *GRID, device="cpu", lib=lib, dtype=dtype, npy=world, rank=rank, global_init=synthetic_global(CASE, *GRID, dtype=dtype),
                 pres_chunks=chunks)
    assert hp.pres_chunks == chunks and lib.mhh_pres_slab_order(hp.plan) == 4
    _run(hp, out)
    hp.close()


def _ranks(world, chunks, dtype=np.float64):
    parts = run_ranks(_worker, world, backend="gloo", tag="slab4-gloo", args=(chunks, dtype))
    return {k: (np.concatenate([p[k] for p in parts], axis=1) if parts[0][k].ndim == 3 else [float(p[k]) for p in parts]) for k in parts[0]}


def _close(got, ref, keys, tol):
    for key in keys:
        scale = np.abs(ref[key]).max()
        err = np.abs(got[key].astype(np.float64) - ref[key]).max() / scale
        assert err <= tol, (key, err)


@pytest.mark.parametrize("world,chunks", [(2, 1), (4, 1), (2, 2), (4, 2)], ids=["2", "4", "2-sliced", "4-sliced"])
def test_pres4_slab_ranks_match_single_rank(world, chunks):
    """Unsliced (mhh_pres_fwd_y_solve_bwd_y between whole transposes) and k-sliced (two slices, mhh_pres_solve_y between them,
    mhh_pres_unpack_slab after the last one) solves against the single-rank HotPath (the single-GPU pres_4 plan)."""
    ref = _single()
    got = _ranks(world, chunks)
    for key in ("rhs_ut", "rhs_vt", "rhs_wt"):
        assert np.array_equal(got[key], ref[key]), key
    _close(got, ref, ("ut", "vt", "wt", "p"), 1e-10)
    for cfl, div in zip(got["cfl"], got["div"]):
        assert cfl == float(ref["cfl"])
        assert abs(div - float(ref["div"])) <= 1e-12 * abs(float(ref["div"]))


def test_pres4_slab_ranks_fp32():
    ref = _single(np.float32)
    got = _ranks(2, 1, np.float32)
    for key in ("rhs_ut", "rhs_vt", "rhs_wt"):
        assert np.array_equal(got[key], ref[key]), key
    _close(got, ref, ("ut", "vt", "wt", "p"), 2e-4)


def test_pres4_one_slab_rank_matches_single_rank_and_oracle():
    """force_slab: the slab code path on one rank (exchanges degenerated to local copies) against the single-rank HotPath, and its
    pressure step against the oracle's Pres_4 input -> solve -> output on the same fields (the helpers of tests/test_parity.py)."""
    lib = B.get("emul").lib
    ref = _single()
    hp = HotPath(CASE, *GRID, device="cpu", lib=lib, global_init=synthetic_global(CASE, *GRID), force_slab=True, pres_chunks=1)
    assert lib.mhh_pres_slab_order(hp.plan) == 4
    _rhs(hp)
    g = hp.grid
    host = {n: getattr(hp, n).numpy().copy() for n in ("u", "v", "w", "ut", "vt", "wt")}
    hp.pres()
    got = {n: _interior(hp, getattr(hp, n)) for n in ("ut", "vt", "wt", "p")}
    _close(got, ref, ("ut", "vt", "wt", "p"), 1e-10)
    O = cm.oracle(); G = g.host_struct()
    p = np.zeros(g.shape3); pk = np.zeros((g.ktot, g.jtot, g.itot))
    O.orc_pres_exec(G, 4, ptr(p), ptr(pk), ptr(host["u"]), ptr(host["v"]), ptr(host["w"]), ptr(host["ut"]), ptr(host["vt"]), ptr(host["wt"]),
                    ptr(hp.rhoref_h), ptr(hp.rhorefh_h), dbl(hp.dt))
    pscale = np.abs(p).max()
    sl = (slice(g.kstart-2, g.kend+2), slice(g.jstart, g.jend), slice(g.istart, g.iend))      # the four mirrored ghost levels included
    assert np.abs(hp.p.numpy()[sl] - p[sl]).max() <= 1e-11 * pscale
    it = (slice(g.kstart, g.kend), slice(g.jstart, g.jend), slice(g.istart, g.iend))
    for n in ("ut", "vt", "wt"):
        want = host[n][it]
        assert np.abs(getattr(hp, n).numpy()[it] - want).max() <= 1e-11 * np.abs(want).max(), n
    hp.close()


def test_pres4_slab_abi():
    """The order-4 slab plan: its order, no LDS x stages, the order-2-only fused entry points refuse it with a message; an order-2
    plan made through the new entry point gives the bits of the old one."""
    lib = B.get("emul").lib
    hp = HotPath(CASE, *GRID, device="cpu", lib=lib, global_init=synthetic_global(CASE, *GRID), force_slab=True, pres_chunks=2)
    P, G, F, st = hp.plan, hp.G, C.byref(hp.fields), hp.stream
    assert lib.mhh_pres_slab_order(P) == 4 and lib.mhh_pres_slab_has_lds(P) == 0
    xb = hp.xrecv.data_ptr()
    for name, call in (("mhh_pres_bwd_x_unpack_output", lambda: lib.mhh_pres_bwd_x_unpack_output(P, G, xb, F, st)),
                       ("mhh_pres_unpack_output_slab", lambda: lib.mhh_pres_unpack_output_slab(P, G, F, st)),
                       ("mhh_pres_slab_lds_fwd", lambda: lib.mhh_pres_slab_lds_fwd(P, G, F, 1.0, xb, 0, st)),
                       ("mhh_pres_slab_lds_bwd", lambda: lib.mhh_pres_slab_lds_bwd(P, G, xb, F, 0, st)),
                       ("mhh_pres_slab_lds_fwd_y", lambda: lib.mhh_pres_slab_lds_fwd_y(P, G, xb, 0, st)),
                       ("mhh_pres_slab_lds_bwd_y", lambda: lib.mhh_pres_slab_lds_bwd_y(P, G, xb, 0, st))):
        assert call() != 0, name
        assert b"order == 2" in lib.mhh_last_error(), (name, lib.mhh_last_error())
    # order 4 needs two ghost cells in y and z
    g = hp.grid
    Gh = g.host_struct(); s = Gh.contents
    s.jgc = 1; s.jcells = s.jmax + 2; s.ijcells = s.icells*s.jcells; s.jstart = 1; s.jend = 1 + s.jmax; s.ncells = s.ijcells*s.kcells
    bad = capi.PLAN()
    assert lib.mhh_pres_slab_plan_create_order(Gh, 4, g.dz.ctypes.data, g.dzhi.ctypes.data, g.dzi4.ctypes.data, g.dzhi4.ctypes.data,
                                               hp.rhoref_h.ctypes.data, hp.rhorefh_h.ctypes.data, C.byref(bad)) != 0
    assert b"2 ghost cells" in lib.mhh_last_error()
    hp.close()

    # order 2 through both entry points: the same bits
    grid2 = (16, 32, 10)
    gi = synthetic_global("drycblles", *grid2)
    out = []
    for old in (False, True):
        hp = HotPath("drycblles", *grid2, device="cpu", lib=lib, global_init=gi, force_slab=True, pres_chunks=1)
        if old:
            g = hp.grid
            lib.mhh_pres_slab_plan_destroy(hp.plan)
            hp.plan = capi.PLAN()
            hp._ok(lib.mhh_pres_slab_plan_create(g.host_struct(), g.dz.ctypes.data, g.dzhi.ctypes.data, hp.rhoref_h.ctypes.data, hp.rhorefh_h.ctypes.data,
                                                 C.byref(hp.plan)))
        assert lib.mhh_pres_slab_order(hp.plan) == 2
        hp.cyclic_prognostic(); hp.exec_viscosity(); hp.rhs(); hp.pres()
        out.append({n: _interior(hp, getattr(hp, n)) for n in ("ut", "vt", "wt", "p")})
        hp.close()
    for n in ("ut", "vt", "wt", "p"):
        assert np.array_equal(out[0][n], out[1][n]), n


@pytest.mark.parametrize("case,grid", [("drycblles", (16, 32, 10)), (CASE, GRID)], ids=["order2-staged", "order4"])
def test_pres_slab_calls_without_slice_index(case, grid):
    """The entry points without a slice index are the per-slice ones on slice 0 of a one-slice plan: HotPath.pres (per-slice calls) and
    the same solve through mhh_pres_fwd_x_pack / fwd_y_solve_bwd_y / bwd_x_unpack[_output] give the same bits. On a plan with two
    slices they are refused, and the message names mhh_pres_slab_set_chunks."""
    lib = B.get("emul").lib
    gi = synthetic_global(case, *grid)
    out = []
    with cm.switches(MHH_PRES_SLAB_LDS="0"):
        for whole in (False, True):
            hp = HotPath(case, *grid, device="cpu", lib=lib, global_init=gi, force_slab=True, pres_chunks=1)
            P, G, F, st = hp.plan, hp.G, C.byref(hp.fields), hp.stream
            order = lib.mhh_pres_slab_order(P)
            assert lib.mhh_pres_slab_chunks(P) == 1 and lib.mhh_pres_slab_has_lds(P) == 0
            _rhs(hp)
            if not whole:
                hp.pres()
            else:
                hp.halo([hp.vt], *hp._pres_vt_rows)
                packed = lib.mhh_pres_slab_packed(P)
                hp._ok(lib.mhh_pres_input_packed(G, order, F, hp.dt, packed, st))
                hp._ok(lib.mhh_pres_fwd_x_pack(P, G, packed, hp.xsend.data_ptr(), st))
                hp.xrecv.copy_(hp.xsend)
                hp._ok(lib.mhh_pres_fwd_y_solve_bwd_y(P, G, hp.xrecv.data_ptr(), hp.xsend.data_ptr(), st))
                hp.xrecv.copy_(hp.xsend)
                if order == 2:
                    hp._ok(lib.mhh_pres_bwd_x_unpack_output(P, G, hp.xrecv.data_ptr(), F, st))
                    hp.halo([hp.p], rows_south=0, rows_north=1)
                    hp._ok(lib.mhh_pres_output_south_row(G, F, st))
                else:
                    hp._ok(lib.mhh_pres_bwd_x_unpack(P, G, hp.xrecv.data_ptr(), F, st))
                    hp.halo([hp.p], rows_south=1, rows_north=2)
                    hp._ok(lib.mhh_pres_output_order(G, 4, F, st))
            out.append({n: getattr(hp, n).numpy().copy() for n in ("ut", "vt", "wt", "p")})
            if whole:
                hp._ok(lib.mhh_pres_slab_set_chunks(P, 2))
                xs, xr = hp.xsend.data_ptr(), hp.xrecv.data_ptr()
                for name, call in (("mhh_pres_fwd_x_pack", lambda: lib.mhh_pres_fwd_x_pack(P, G, None, xs, st)),
                                   ("mhh_pres_fwd_y_solve_bwd_y", lambda: lib.mhh_pres_fwd_y_solve_bwd_y(P, G, xr, xs, st)),
                                   ("mhh_pres_bwd_x_unpack", lambda: lib.mhh_pres_bwd_x_unpack(P, G, xr, F, st))) + \
                                  ((("mhh_pres_bwd_x_unpack_output", lambda: lib.mhh_pres_bwd_x_unpack_output(P, G, xr, F, st)),) if order == 2 else ()):
                    assert call() != 0, name
                    assert b"set_chunks" in lib.mhh_last_error(), (name, lib.mhh_last_error())
                # refused before anything ran: the fields are as they were; and one slice again gives the calls back
                for n in ("ut", "vt", "wt", "p"):
                    assert np.array_equal(getattr(hp, n).numpy(), out[-1][n]), n
                hp._ok(lib.mhh_pres_slab_set_chunks(P, 1))
                hp._ok(lib.mhh_pres_fwd_x_pack(P, G, None, xs, st))
            hp.close()
    for n in ("ut", "vt", "wt", "p"):
        assert np.array_equal(out[0][n], out[1][n]), n
