"""The scalar pass of the marching (advec_2i5, diff_smag2) kernel: scalars 1, 2, ... of fields.st in batches, one k-march per
batch (microhh_amd/csrc/k_march.hip, rhs25_scalar_march_kernel), behind mhh_rhs_exec, mhh_advec_exec + mhh_diff_exec and the
row-wise forms. Every tendency must carry the oracle's bits, the per-field cell kernels' (MHH_SCALAR_IMPL=cell) as well.

Runs on the ``emul`` backend (the same kernel sources on the CPU) and on the ``hip`` backend (marked gpu)."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
from backends import be  # noqa: F401
from common import DTYPES

ADV, DIF = cm.ADVEC_2I5, cm.DIFF_SMAG2


def _svisc(n):
    """A different diffusivity per scalar: a batch that mixed up its scalars' coefficients would show."""
    return [1e-5 * (1 + 0.25*m) for m in range(n)]


def _dev(be, c, svisc, limited=()):
    d = B.DevCase(be, c); f = d.fields()
    for n, sv in enumerate(svisc):
        f.svisc[n] = sv
    for n in limited:
        f.s_fluxlimit[n] = 1
    return d, f


def _got(be, d):
    return cm.flat(cm.tendencies(be, d))


def _fused(be, c, sm, svisc, limited=()):
    d, f = _dev(be, c, svisc, limited)
    B.ok(be, be.lib.mhh_rhs_exec(d.G, ADV, DIF, C.byref(f), C.byref(cm.diff_params(sm)), be.stream))
    return _got(be, d)


def _unfused(be, c, sm, svisc, limited=()):
    d, f = _dev(be, c, svisc, limited)
    B.ok(be, be.lib.mhh_advec_exec(d.G, ADV, C.byref(f), be.stream))
    B.ok(be, be.lib.mhh_diff_exec(d.G, DIF, C.byref(f), C.byref(cm.diff_params(sm)), be.stream))
    return _got(be, d)


def _names(n):
    return ["ut", "vt", "wt"] + ["st%d" % m for m in range(n)]


def _check(got, want, tag):
    for a, b, nm in zip(got, want, _names(len(want) - 3)):
        assert np.array_equal(a, b), (tag, nm, cm.ulp_diff(a, b))


# (shape, ghost cells, extra environment): ragged tiles, tall columns over several k-chunks, rows not 16-byte aligned
# (4-byte copies), sixteen ghost cells in x (tile origins put on a 16-byte piece)
GRIDS = [((70, 9, 10), (3, 3, 1), {}),
         ((18, 5, 40), (3, 3, 1), {"MHH_MARCH_KC_RT": "8"}),
         ((17, 9, 8), (3, 3, 1), {}),
         ((16, 6, 12), (3, 3, 2), {"MHH_MARCH_DMA": "4"}),
         ((70, 6, 9), (16, 3, 1), {})]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nsc", [2, 3, 8])
def test_scalar_pass_bitexact_against_oracle(be, dtype, nsc):
    """mhh_rhs_exec and mhh_advec_exec + mhh_diff_exec with 2, 3 and 8 scalars (odd counts, a partial last batch): every
    tendency has the oracle's bits, with rho one and random, surface model 0 and 1, and one flux-limited scalar."""
    svisc = _svisc(nsc)
    for shape, gc, env in GRIDS:
        g = cm.grid_2nd(*shape, gc=gc, dtype=dtype)
        for rho, sm, limited in (("random", 1, ()), ("one", 0, ()), ("random", 0, (1,)), ("one", 1, (nsc - 1,))):
            c = cm.Case(g, nscalars=nsc, rho=rho, periodic=gc[0] > 3)
            want = cm.flat(cm.oracle_rhs(c, ADV, DIF, sm, svisc=svisc, limited=limited))
            # the pass must have run: the fused call launches it for the unlimited scalars >= 1, the unfused pair at least for
            # the diffusion of scalars >= 1 (which has no limiter)
            fused_runs = any(n not in limited for n in range(1, nsc))
            launches = be.lib.mhh_stat_scalar_march_launches
            with cm.switches(**env):
                n0 = launches()
                _check(_fused(be, c, sm, svisc, limited), want, ("fused", shape, gc, rho, sm, limited))
                n1 = launches()
                _check(_unfused(be, c, sm, svisc, limited), want, ("unfused", shape, gc, rho, sm, limited))
                n2 = launches()
            assert (n1 > n0) == fused_runs and n2 > n1, (shape, gc, rho, sm, limited, n0, n1, n2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_pass_equals_cell_kernels_and_one_per_launch(be, dtype):
    """The scalar pass, the same pass one scalar per launch (MHH_SCALAR_BATCH=1) and the per-field cell kernels
    (MHH_SCALAR_IMPL=cell) give the same bits, after each of the two unfused calls as well."""
    g = cm.grid_2nd(66, 7, 9, gc=(3, 3, 1), dtype=dtype)
    c = cm.Case(g, nscalars=4)
    svisc = _svisc(4)
    out = {}
    for form, env in (("pass", {}), ("single", {"MHH_SCALAR_BATCH": "1"}), ("cell", {"MHH_SCALAR_IMPL": "cell"})):
        with cm.switches(**env):
            d, f = _dev(be, c, svisc)
            B.ok(be, be.lib.mhh_advec_exec(d.G, ADV, C.byref(f), be.stream))
            adv = _got(be, d)
            B.ok(be, be.lib.mhh_diff_exec(d.G, DIF, C.byref(f), C.byref(cm.diff_params(1)), be.stream))
            out[form] = (adv, _got(be, d), _fused(be, c, 1, svisc))
    for form in ("single", "cell"):
        for stage in range(3):
            _check(out[form][stage], out["pass"][stage], (form, stage))


def test_scalar_pass_launch_counter(be):
    """mhh_stat_scalar_march_launches rises with every mhh_rhs_exec that has two or more unlimited scalars; it does not move
    with one scalar, nor under MHH_SCALAR_IMPL=cell."""
    g = cm.grid_2nd(16, 12, 10, gc=(3, 3, 1))
    lib = be.lib
    for nsc, env, rises in ((2, {}, True), (3, {}, True), (1, {}, False), (3, {"MHH_SCALAR_IMPL": "cell"}, False)):
        c = cm.Case(g, nscalars=nsc)
        with cm.switches(**env):
            n0 = lib.mhh_stat_scalar_march_launches()
            _fused(be, c, 1, _svisc(nsc))
            n1 = lib.mhh_stat_scalar_march_launches()
        assert (n1 - n0 >= 1) if rises else (n1 == n0), (nsc, env, n0, n1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_wise_forms_with_three_scalars(be, dtype):
    """mhh_rhs_exec_rows over [jstart+4, jend-4) and mhh_rhs_exec_rows2 over the two edge strips give the bits of the
    whole-domain mhh_rhs_exec with three scalars; a flux-limited scalar is still refused there."""
    for shape, sm in (((70, 14, 10), 1), ((17, 13, 8), 0)):
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype)
        c = cm.Case(g, nscalars=3)
        svisc = _svisc(3)
        want = _fused(be, c, sm, svisc)
        d, f = _dev(be, c, svisc)
        P = cm.diff_params(sm)
        ja, jb = g.jstart + 4, g.jend - 4
        B.ok(be, be.lib.mhh_rhs_exec_rows(d.G, ADV, DIF, C.byref(f), C.byref(P), ja, jb, be.stream))
        B.ok(be, be.lib.mhh_rhs_exec_rows2(d.G, ADV, DIF, C.byref(f), C.byref(P), g.jstart, ja, jb, g.jend, be.stream))
        _check(_got(be, d), want, ("rows", shape))
        d, f = _dev(be, c, svisc, limited=(2,))
        assert be.lib.mhh_rhs_exec_rows(d.G, ADV, DIF, C.byref(f), C.byref(P), ja, jb, be.stream) != 0
        assert b"at most one, unlimited scalar" in be.lib.mhh_last_error()


def _rhs_once(hp, fn, env):
    """The tendencies after one call of fn under env, the tendencies themselves put back as they were."""
    import torch
    tend = [hp.ut, hp.vt, hp.wt] + list(hp.st)
    keep = [t.clone() for t in tend]
    with cm.switches(**env):
        fn(); hp.sync()
    out = [t.clone() for t in tend]
    for t, k in zip(tend, keep):
        t.copy_(k)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_three_scalars_at_256_cubed_fused_unfused_and_cell_forms_agree():
    """drycblles 256^3 fp64 with three scalars: the fused path, the unfused path (mhh_advec_exec + mhh_diff_exec) and the
    cell path (MHH_SCALAR_IMPL=cell + MHH_RHS25_IMPL=cell) give the same tendencies, bit for bit."""
    import torch
    from microhh_amd.model import HotPath
    hp = HotPath("drycblles", 256, 256, 256, device="cuda:0", nscalars=3)
    hp.cyclic_prognostic(); hp.exec_viscosity(); hp.sync()
    n0 = hp.lib.mhh_stat_scalar_march_launches()
    fused = _rhs_once(hp, hp.rhs, {})
    assert hp.lib.mhh_stat_scalar_march_launches() > n0
    unfused = _rhs_once(hp, hp.rhs_unfused, {})
    cell = _rhs_once(hp, hp.rhs, {"MHH_SCALAR_IMPL": "cell", "MHH_RHS25_IMPL": "cell"})
    for form, other in (("unfused", unfused), ("cell", cell)):
        for a, b, nm in zip(fused, other, _names(3)):
            assert torch.equal(a, b), (form, nm, float((a - b).abs().max()))
    assert not torch.equal(fused[4], hp.st[1])                    # the pass did something
    hp.close()
