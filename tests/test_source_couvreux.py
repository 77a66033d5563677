"""The couvreux mask of Decay::get_mask (src/decay.cxx:123-187): mhh_decay_couvreux_sums / _field and the built-in `couvreux` mask
of Stats, on the ragged 37 x 19 x 11 grid of tests/source_ref.py, both dtypes, emulation and GPU.

The reference is the restatement tests/source_ref.ref_couvreux (the loops are inline in a member that needs Fields and Stats, out of a
shim's reach), from the golden file on the GPU. Mean and variance profiles and the mask field within the bound DESIGN.md section 4.13
uses for level sums, 4 n 2^-53 S_k + ulp; the variance, a difference of two such quotients, within the sum of their bounds; the field,
mean plus nstd times the standard deviation, within the bounds those two carry into it. The mask words (field > 0, on full and half
levels) are compared on every cell whose |field| exceeds its bound; at most 1 % of a level may be left out. The seeded scalar holds
multiples of 1/16, so that the reference's own sequential TF sums are exact and stay inside the bound themselves; the share left out
by the reference is recorded in the golden file.
"""
import numpy as np
import pytest

import backends as B
import common as cm
import source_ref as R
from backends import be  # noqa: F401
from microhh_amd.stats import PLUS

CASES = [c for c in R.CASES if c[0] == R.SHAPES[1]]
IDS = [R.case_id(c) for c in CASES]


def run(be, g, s, nstd=R.NSTD):
    n = int(be.lib.mhh_decay_couvreux_scratch_elems(g.host_struct()))
    scratch, sums = be.zeros(n, np.float64), be.zeros((2, g.kcells), np.float64)
    out, outh = be.arr(np.full(g.shape3, 7., dtype=g.np_dtype)), be.arr(np.full(g.shape3, 7., dtype=g.np_dtype))
    sd = be.arr(s)
    G = be.grid(g)
    B.ok(be, be.lib.mhh_decay_couvreux_sums(G, be.ptr(sd), be.ptr(scratch), be.ptr(sums), be.stream))
    B.ok(be, be.lib.mhh_decay_couvreux_field(G, be.ptr(sd), be.ptr(sums), nstd, be.ptr(out), be.ptr(outh), be.stream))
    be.sync()
    return be.host(sums), be.host(out), be.host(outh)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_stays_inside_the_bound(case):
    """On the CPU: the seeded scalar's level sums are exact in the grid's dtype, and the recorded share is what this host finds."""
    g, s = R.grid_of(case), R.inputs(case).field("cv", 0)
    a = s[g.interior].astype(np.float64)
    mean, var, fld, _ = R.ref_couvreux(g, s)
    assert cm.same_bits(mean[g.kstart:g.kend].astype(np.float64), (a.sum(axis=(1, 2))/a[0].size).astype(g.np_dtype).astype(np.float64))
    share = R.couvreux_excluded(g, fld)
    assert share <= 0.01 and share == float(R.golden()["%s/cv_excluded" % R.case_id(case)][0])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_profiles_field_and_mask(be, case):
    g, s = R.grid_of(case), R.inputs(case).field("cv", 0)
    sums, out, outh = run(be, g, s)
    it, ks = g.interior, slice(g.kstart, g.kend)
    n = g.itot*g.jtot
    a = s[it].astype(np.float64)
    ulp = lambda x: np.spacing(np.abs(x).astype(g.np_dtype)).astype(np.float64)           # noqa: E731
    want_mean, want_var = R.ref(case, "cv_mean", be).astype(np.float64)[ks], R.ref(case, "cv_var", be).astype(np.float64)[ks]
    bm = R.level_bound(g, s[it]) + ulp(want_mean)
    bq = R.level_bound(g, (s[it]*s[it])) + ulp((a*a).sum(axis=(1, 2))/n)
    mean = (sums[0, ks]/n).astype(g.np_dtype).astype(np.float64)
    msq = (sums[1, ks]/n).astype(g.np_dtype)
    var = (msq - (mean.astype(g.np_dtype))**2).astype(np.float64)
    assert (np.abs(mean - want_mean) <= bm).all(), np.abs(mean - want_mean).max()
    # var = msq - mean^2: the bound of msq, 2 |mean| times that of mean, and the roundings of the product and the difference
    bv = bq + 2.*np.abs(want_mean)*bm + ulp(want_mean**2) + ulp(want_var)
    assert (np.abs(var - want_var) <= bv).all(), np.abs(var - want_var).max()
    assert (sums[:, :g.kstart] == 0).all() and (sums[:, g.kend:] == 0).all()
    # the field: s - mean - nstd*std; d std = d var / (2 std)
    std = np.sqrt(want_var)
    bf = bm + R.NSTD*(bv/(2.*std) + ulp(std)) + ulp(R.NSTD*std)
    want, wanth = R.ref(case, "cv_fld", be), R.ref(case, "cv_fldh", be)
    bcell = bf[:, None, None] + 2.*ulp(np.abs(want).max())
    err = np.abs(out[it].astype(np.float64) - want.astype(np.float64))
    assert (err <= bcell).all(), (err.max(), bcell.min())
    assert (out[:g.kstart] == 0).all() and (out[g.kend:] == 0).all() and (out[:, :g.jstart] == 0).all() and (out[:, :, g.iend:] == 0).all()
    half = (slice(g.kstart, g.kend+1), it[1], it[2])
    bh = np.zeros(g.kmax + 1); bh[:-1] += bf; bh[1:] += bf
    errh = np.abs(outh[half].astype(np.float64) - wanth.astype(np.float64))
    assert (errh <= bh[:, None, None] + 4.*ulp(np.abs(want).max())).all(), errh.max()
    # the mask words on every cell but those under the bound: at most 1 % of a level
    for got, ref_f, bits, bnd, name in ((out[it], want, "cv_mask", bcell, "full"), (outh[half], wanth, "cv_maskh", bh[:, None, None] + 4.*ulp(np.abs(want).max()), "half")):
        ref_mask = np.unpackbits(R.ref(case, bits, be))[:ref_f.size].reshape(ref_f.shape).astype(bool)
        assert np.array_equal(ref_mask, ref_f > 0)
        keep = np.abs(ref_f.astype(np.float64)) > bnd
        assert (1. - keep.mean(axis=(1, 2))).max() <= 0.01, name
        assert np.array_equal((got > 0)[keep], ref_mask[keep]), name
        assert 0.02 < ref_mask.mean() < 0.5, name                    # a mask that selects the tail, not nothing and not all


def _hotpath(backend, masks, decay, dtype=np.float64):
    from microhh_amd.model import HotPath
    from microhh_amd.stats import Stats
    kw = dict(device="cpu", lib=B.get("emul").lib) if backend == "emul" else {}
    return HotPath("drycblles", 32, 24, 16, dtype=dtype, nscalars=3, stats=Stats(masks=masks), decay=decay, **kw)


@pytest.mark.parametrize("backend", cm.BACKENDS)
def test_the_stats_mask_is_built_in(backend):
    """Stats(masks=("default", "couvreux")) with decay= carrying a scalar called couvreux: the mask words are set_mask_thres of the two
    fields at 0, Plus -- the same words as the caller's own registration of those fields under another name."""
    from microhh_amd.source import Decay
    dec = lambda: Decay({"couvreux": 600.}, nstd_couvreux=0.5, names={"couvreux": 2})            # noqa: E731
    hp = _hotpath(backend, ("default", "couvreux"), dec())
    assert hp.decay.timescales == {2: 600.} and hp.decay.has_mask("couvreux") and not hp.decay.has_mask("ql")
    hp.stats.enqueue(); hp.sync()
    got = hp.stats.sampler.mfield.detach().cpu().numpy().copy()
    fld = hp.decay.couvreux().detach().cpu().numpy().copy()
    hp.close()
    hp2 = _hotpath(backend, ("default", "mine"), dec())
    hp2.stats.mask_thres("mine", hp2.decay.couvreux, hp2.decay.couvreux_h, None, 0., PLUS)
    hp2.stats.enqueue(); hp2.sync()
    want = hp2.stats.sampler.mfield.detach().cpu().numpy().copy()
    hp2.close()
    assert cm.same_bits(got, want)
    g = hp.grid
    sel = fld[g.interior] > 0
    assert 0.05 < sel.mean() < 0.5                                   # half a standard deviation above the mean


def test_the_mask_raises_without_the_scalar():
    from microhh_amd.source import Decay
    for decay in (None, Decay({2: 600.})):
        with pytest.raises(ValueError, match="Couvreux mask not available without couvreux scalar"):
            _hotpath("emul", ("default", "couvreux"), decay)
    with pytest.raises(ValueError, match="no scalar called 'tracer'"):
        Decay({"tracer": 10.})
    d = Decay({"th": 10., "s1": 20., 2: 30.})
    assert d.timescales == {0: 10., 1: 20., 2: 30.}
