"""The scalar pass of the marching (advec_4, diff_4) kernel: every scalar of fields.st in batches, one k-march per batch
(microhh_amd/csrc/k_march4.hip, rhs44_scalar_march_kernel), behind mhh_rhs_exec, mhh_advec_exec and mhh_diff_exec. Every
tendency must carry the oracle's bits, the per-field cell kernels' (MHH_SCALAR_IMPL=cell) as well. The cell kernels give those
bits too, so every comparison also asserts that the pass ran (mhh_stat_scalar4_march_launches went up).

The pass is selected with MHH_SCALAR_IMPL=march (``PASS`` below); without it the per-field kernels run, which
``test_scalar_pass4_counters`` holds: the pass stays opt-in until timings on the device show it the faster form.

Runs on the ``emul`` backend (the same kernel sources on the CPU) and on the ``hip`` backend (marked gpu).

The copy form. The launcher takes 16-byte pieces only where the rows are whole pieces (icells % VEC == 0), the tile origin
istart - 3 lies on a piece ((igc - 3) % VEC == 0, VEC = cells per 16 bytes: 2 in fp64, 4 in fp32) and every copied array is 16-byte
aligned; everything else copies in 4-byte pieces. The grids below were chosen so that both forms occur in both precisions;
``_expected_piece`` restates the rule. For (16, 6, 10) with igc = 4 the rule gives 4-byte copies in BOTH precisions (the origin
is one cell into the row: 8 bytes in fp64, 4 bytes in fp32, neither a multiple of 16); with igc = 5 it gives 16-byte copies in
fp64 (origin 2 cells = 16 bytes) and 4-byte copies in fp32 (8 bytes). fp32 reaches 16-byte copies on the igc = 3 grids with
icells % 4 == 0, (70, 9, 12) among them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import backends as B
import common as cm
from backends import be  # noqa: F401
from common import DTYPES

sys.path.insert(0, os.path.join(cm.ROOT, "tests", "golden"))
import make_golden as mg  # noqa: E402

ADV, DIF = cm.ADVEC_4, cm.DIFF_4
PASS = {"MHH_SCALAR_IMPL": "march"}   # selects the pass
SCALARS4 = 4                       # mhh_stat_march_form: the scalar pass of the 4th-order kernel
GOLD = np.load(os.path.join(cm.ROOT, "tests", "golden", "ref_vectors.npz"))


def _svisc(n):
    """A different diffusivity per scalar: a batch that mixed up its scalars' coefficients would show."""
    return [1e-5 * (1 + 0.25*m) for m in range(n)]


def _dev(be, c, svisc):
    d = B.DevCase(be, c); f = d.fields()
    for n, sv in enumerate(svisc):
        f.svisc[n] = sv
    return d, f


def _got(be, d):
    return cm.flat(cm.tendencies(be, d))


def _fused(be, c, svisc, params=None):
    d, f = _dev(be, c, svisc)
    p = cm.diff_params(0) if params is None else params
    B.ok(be, be.lib.mhh_rhs_exec(d.G, ADV, DIF, C.byref(f), C.byref(p), be.stream))
    return _got(be, d)


def _unfused(be, c, svisc):
    """The tendencies after mhh_advec_exec, and after mhh_diff_exec on top of it."""
    d, f = _dev(be, c, svisc)
    B.ok(be, be.lib.mhh_advec_exec(d.G, ADV, C.byref(f), be.stream))
    adv = _got(be, d)
    B.ok(be, be.lib.mhh_diff_exec(d.G, DIF, C.byref(f), C.byref(cm.diff_params(0)), be.stream))
    return adv, _got(be, d)


def _names(n):
    return ["ut", "vt", "wt"] + ["st%d" % m for m in range(n)]


def _check(got, want, tag):
    assert len(got) == len(want)
    for a, b, nm in zip(got, want, _names(len(want) - 3)):
        assert np.array_equal(a, b), (tag, nm, cm.ulp_diff(a, b))


def _form(be):
    v = [C.c_int(0) for _ in range(4)]
    B.ok(be, be.lib.mhh_stat_march_form(SCALARS4, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _launches(be):
    return be.lib.mhh_stat_scalar4_march_launches()


def _expected_piece(g):
    """The launcher's rule for arrays that are 16-byte aligned (numpy's and torch's allocations are): rows of whole pieces, the
    tile origin istart - 3 on a piece, and (pieces16_clear_of_row_end, k_march_common.h, with off = reach = 3) no active lane
    reading the piece that is clamped at the end of a row: with the origin on a piece that needs igc >= 3."""
    vec = 16 // g.np_dtype.itemsize
    on_piece = g.icells % vec == 0 and (g.igc - 3) % vec == 0
    clear_of_row_end = on_piece and (g.istart - 3) % vec == 0 and g.igc >= 3
    return 16 if (on_piece and clear_of_row_end) else 4


# (shape, grid keywords, environment): what each reaches is in the table of the test below
GRIDS = [((70, 9, 12), {}, {}),
         ((18, 5, 20), {}, {"MHH_MARCH_KC_RT": "8"}),
         ((17, 6, 8), {}, {}),
         ((16, 6, 10), {"igc": 4}, {}),
         ((16, 6, 10), {"igc": 5}, {}),
         ((12, 1, 8), {}, {}),
         ((6, 4, 5), {}, {})]
_seen_forms = {}                   # (backend, dtype) -> the piece sizes the grids reached


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nsc", [1, 2, 3])
def test_scalar_pass4_bitexact_against_oracle(be, dtype, nsc):
    """mhh_rhs_exec and mhh_advec_exec + mhh_diff_exec with 1, 2 and 3 scalars (a batch of one, a full batch, a partial last
    batch), each with its own svisc: every tendency has the oracle's bits, and the pass ran. The grids, each the smallest that
    reaches its case:
      (70, 9, 12)            two tiles in x, the second with 6 cells; ragged tile rows
      (18, 5, 20), chunks of 8   three chunks, the last of 4 levels: the carried terms restart at a chunk
      (17, 6, 8)             rows not 16-byte aligned: 4-byte copies
      (16, 6, 10), igc = 4   tile origin off a piece in both precisions: 4-byte copies (see the module docstring)
      (16, 6, 10), igc = 5   tile origin on a piece in fp64 (16-byte copies), off one in fp32 (4-byte copies)
      (12, 1, 8)             jtot = 1: dim3 is false
      (6, 4, 5)              both walls inside one short column
    The copy form of every launch is the one the launcher's rule predicts, and 16-byte pieces never start off a piece."""
    svisc = _svisc(nsc)
    for shape, kw, env in GRIDS:
        g = cm.grid_4th(*shape, dtype=dtype, **kw)
        c = cm.Case(g, nscalars=nsc)
        want_adv = cm.flat(cm.oracle_rhs(c, ADV, None, 0))
        want = cm.flat(cm.oracle_rhs(c, ADV, DIF, 0, svisc=svisc))
        tag = (shape, kw, env)
        vec = 16 // g.np_dtype.itemsize
        with cm.switches(**PASS, **env):
            n0 = _launches(be)
            _check(_fused(be, c, svisc), want, ("fused",) + tag)
            n1 = _launches(be)
            forms = [_form(be)]
            adv, both = _unfused(be, c, svisc)
            n2 = _launches(be)
            forms.append(_form(be))
        _check(adv, want_adv, ("advec",) + tag)
        _check(both, want, ("advec + diff",) + tag)
        batches = (nsc + 1) // 2
        assert n1 - n0 == batches and n2 - n1 == 2*batches, (tag, n0, n1, n2)
        for pb, hx, ex, cw in forms:
            assert (pb, hx, ex, cw) == (_expected_piece(g), 3, 0, 1), (tag, pb, hx, ex, cw)
            assert pb == 4 or (g.icells % vec == 0 and (g.istart - hx) % vec == 0), (tag, "16-byte pieces off a piece")
            _seen_forms.setdefault((be.name, np.dtype(dtype).name), set()).add(pb)
    assert _seen_forms[(be.name, np.dtype(dtype).name)] == {4, 16}


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_pass4_forms_agree(be, dtype):
    """The pass, the pass one scalar per launch (MHH_SCALAR_BATCH=1), the per-field kernels (MHH_SCALAR_IMPL=cell) and the cell
    kernel (MHH_RHS44_IMPL=cell) give the same bits after each of the two unfused calls and after the fused call."""
    g = cm.grid_4th(66, 7, 9, dtype=dtype)
    c = cm.Case(g, nscalars=4)
    svisc = _svisc(4)
    out, ran = {}, {}
    for form, env in (("pass", PASS), ("single", dict(PASS, MHH_SCALAR_BATCH="1")), ("cell", {"MHH_SCALAR_IMPL": "cell"}), ("default", {}),
                      ("rhs44 cell", dict(PASS, MHH_RHS44_IMPL="cell"))):
        with cm.switches(**env):
            n0 = _launches(be)
            out[form] = _unfused(be, c, svisc) + (_fused(be, c, svisc),)
            ran[form] = _launches(be) - n0
    assert ran == {"pass": 6, "single": 12, "cell": 0, "default": 0, "rhs44 cell": 0}, ran
    for form in ("single", "cell", "default", "rhs44 cell"):
        for stage in range(3):
            _check(out[form][stage], out["pass"][stage], (form, stage))


def test_scalar_pass4_counters(be):
    """Under MHH_SCALAR_IMPL=march mhh_stat_scalar4_march_launches rises with scalars, one per batch; it stays put without scalars,
    without the switch, under MHH_SCALAR_IMPL=cell and under MHH_RHS44_IMPL=cell. mhh_stat_rhs44_march_launches still rises by exactly one per fused call (not under
    MHH_RHS44_IMPL=cell)."""
    g = cm.grid_4th(16, 12, 10)
    lib = be.lib
    for nsc, env, rise, rise44 in ((1, PASS, 1, 1), (2, PASS, 1, 1), (3, PASS, 2, 1), (3, dict(PASS, MHH_SCALAR_BATCH="1"), 3, 1), (0, PASS, 0, 1),
                                   (3, {}, 0, 1), (3, {"MHH_SCALAR_IMPL": "cell"}, 0, 1), (3, dict(PASS, MHH_RHS44_IMPL="cell"), 0, 0)):
        c = cm.Case(g, nscalars=nsc)
        with cm.switches(**env):
            n0, m0 = _launches(be), lib.mhh_stat_rhs44_march_launches()
            _fused(be, c, _svisc(nsc))
            n1, m1 = _launches(be), lib.mhh_stat_rhs44_march_launches()
        assert n1 - n0 == rise and m1 - m0 == rise44, (nsc, env, n0, n1, m0, m1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalar_pass4_chunks_and_batch_do_not_change_the_bits(be, dtype):
    """A column cut into chunks of 8 levels gives the bits of the column in one chunk (the carried terms restart at a chunk with
    the terms a level forms afresh), for three scalars; so does one scalar per launch (MHH_SCALAR_BATCH=1), in one chunk and cut."""
    g = cm.grid_4th(18, 5, 20, dtype=dtype)
    c = cm.Case(g, nscalars=3)
    svisc = _svisc(3)
    with cm.switches(**PASS):
        whole = _fused(be, c, svisc)
    for env, launches in (({"MHH_MARCH_KC_RT": "8"}, 2), ({"MHH_SCALAR_BATCH": "1"}, 3), ({"MHH_MARCH_KC_RT": "8", "MHH_SCALAR_BATCH": "1"}, 3)):
        with cm.switches(**PASS, **env):
            n0 = _launches(be)
            got = _fused(be, c, svisc)
            assert _launches(be) - n0 == launches, (env, launches)
        _check(got, whole, env)


def test_scalar_pass4_reproduces_reference_vectors(be):
    """The reference's own bits (tests/golden/ref_vectors.npz) on the fourth-order golden case, through the pass:
    mhh_advec_exec(ADVEC_4) with one scalar gives advec4_st; mhh_diff_exec(DIFF_4) with u handed in as the scalar, a copy of ut
    as its tendency and svisc = 1.3e-2 gives diff4_ut."""
    _, _, g4, c4 = mg.cases(GOLD["z2"], GOLD["z4"])
    d = B.DevCase(be, c4); f = d.fields()
    n0 = _launches(be)
    with cm.switches(**PASS):
        B.ok(be, be.lib.mhh_advec_exec(d.G, ADV, C.byref(f), be.stream))
    n1 = _launches(be)
    assert n1 - n0 == 1
    assert np.array_equal(be.host(d.st[0])[g4.interior], GOLD["advec4_st"])
    d = B.DevCase(be, c4); f = d.fields()
    t = be.arr(c4.ut)
    f.s[0] = be.ptr(d.u).value; f.st[0] = be.ptr(t).value; f.svisc[0] = 1.3e-2
    with cm.switches(**PASS):
        B.ok(be, be.lib.mhh_diff_exec(d.G, DIF, C.byref(f), C.byref(cm.diff_params(0)), be.stream))
    assert _launches(be) - n1 == 1
    assert np.array_equal(be.host(t)[g4.interior], GOLD["diff4_ut"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_buoyancy_fold_unchanged_by_the_scalar_pass(be, dtype):
    """Thermo_buoy's flat fourth-order buoyancy (buoyancy = 4, buoyancy_kind = 1, b = scalar 0) with a second, passive scalar:
    mhh_rhs_exec gives the bits it gives with the per-field scalar kernels (MHH_SCALAR_IMPL=cell), on a grid where the buoyancy
    is folded into the u, v, w kernel and on a jtot = 1 grid where it keeps its own launch; the pass ran."""
    for shape in ((16, 12, 12), (20, 1, 12)):
        g = cm.grid_4th(*shape, dtype=dtype)
        c = cm.Case(g, nscalars=2)
        svisc = _svisc(2)
        out = {}
        for form, env in (("pass", PASS), ("cell", {"MHH_SCALAR_IMPL": "cell"})):
            p = cm.diff_params(0, buoyancy=4, buoyancy_kind=1, th_for_N2=0)
            with cm.switches(**env):
                n0 = _launches(be)
                out[form] = _fused(be, c, svisc, p)
                assert _launches(be) - n0 == (1 if form == "pass" else 0), (shape, form)
        _check(out["pass"], out["cell"], ("buoyancy", shape))
        assert not np.array_equal(out["pass"][2], _fused(be, c, svisc)[2])         # the buoyancy was there


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
def test_drycbl_two_scalars_fused_unfused_and_cell_forms_agree():
    """drycbl 256 x 128 x 128 fp64 with two scalars (b with its folded buoyancy, and a passive one): the fused path, the unfused
    path (both with the scalar pass, MHH_SCALAR_IMPL=march) and the per-field scalar kernels (MHH_SCALAR_IMPL=cell) give the same tendencies, bit for bit."""
    import torch
    from microhh_amd.model import HotPath
    hp = HotPath("drycbl", 256, 128, 128, device="cuda:0", nscalars=2)
    hp.cyclic_prognostic(); hp.sync()
    n0 = hp.lib.mhh_stat_scalar4_march_launches()
    fused = _rhs_once(hp, hp.rhs, PASS)
    assert hp.lib.mhh_stat_scalar4_march_launches() == n0 + 1
    unfused = _rhs_once(hp, hp.rhs_unfused, PASS)
    assert hp.lib.mhh_stat_scalar4_march_launches() == n0 + 3
    cell = _rhs_once(hp, hp.rhs, {"MHH_SCALAR_IMPL": "cell"})
    assert hp.lib.mhh_stat_scalar4_march_launches() == n0 + 3
    for form, other in (("unfused", unfused), ("cell", cell)):
        for a, b, nm in zip(fused, other, _names(2)):
            assert torch.equal(a, b), (form, nm, float((a - b).abs().max()))
    assert not torch.equal(fused[4], hp.st[1])                    # the pass did something
    hp.close()
