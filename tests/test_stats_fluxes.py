"""The resolved, diffusive and total fluxes of csrc/stats.h (_w, _diff, _flux) against the reference's own flux kernels:
advec_flux_u / _v / _s of advec_2 and advec_2i5, advec_flux_s_lim, Diff_smag2::diff_flux in both surface forms and Diff_2::diff_flux,
each included in place behind a shim of its own (tests/cpp/ref_stats_flux_*_shim.cpp), averaged by the reference's calc_mean under
flagh; or tests/golden/stats_ref.npz. The device is given the reference's own mean profiles of the variable and of w, so both sides
sum the same terms; per level |got - want| <= 4 n 2^-53 S_k + ulp(want), S_k the masked mean of |flux| from the reference's flux field.

One exclusion, with a cap: where a level's full-level mask is empty the reference subtracts the fill value as its mean, so _w and
_flux at a flux level whose stencil k-3 .. k+2 touches such a level are left out of the numeric comparison (the kernel still
evaluates them: the fill positions are compared everywhere). They may be at most a quarter of a case's _w pairs and none of the
default or sparse masks'."""
import numpy as np
import pytest

import common as cm
import stats_ref as SR
from backends import be  # noqa: F401
from microhh_amd import capi
from microhh_amd import stats as S

SEEDED = [c for c in SR.all_cases() if c[2] == "seeded"]
IDS = ["%s-gc%d%d%d" % ((SR.case_of(s, k).key,) + gc) for s, gc, k in SEEDED]
NM = len(SR.MASKS)


class FluxDev(SR.Dev):
    """The case's arrays with the horizontal ghost cells of the variable, w and evisc filled periodically."""

    def __init__(self, be, shape, gc, dtype):  # noqa: F811
        super().__init__(be, shape, gc, dtype)
        self.fh = SR.flux_host(self.c, self.g)
        self.fd = {k: self.tensor(v) for k, v in self.fh.items()}

    def w_job(self, c, mean, wmean):
        return (self.fd["a"], 0, S.FLUX_W, SR.FLUX_OFF, 0., mean, dict(kind=c[1], scheme=c[0], limit=c[2], w=self.fd["wh"], wmean=wmean))

    def d_job(self, c):
        return (self.fd["a"], 0, S.FLUX_DIFF, SR.FLUX_OFF, 0., None, dict(kind=c[1], scheme=c[0], surface_model=c[2], w=self.fd["wh"], evisc=self.fd["ev"],
                                                                      flux_bot=self.fd["fbot"], flux_top=self.fd["ftop"], visc=SR.VISC, tPr=SR.TPR))


def _compare(g, got, want, scale, nmaskh, excluded, what):
    ks, ke = g.kstart, g.kend + 1
    fill = S.fill_value(g.np_dtype)
    worst = 0.
    for m in range(NM):
        assert np.array_equal(got[m] == fill, nmaskh[m] == 0) and np.array_equal(want[m] == fill, nmaskh[m] == 0), (what, SR.MASKS[m])
        live = (nmaskh[m, ks:ke] > 0) & ~excluded[m, ks:ke]
        tol = SR.bound(g, want[m, ks:ke], scale[m, ks:ke])
        with np.errstate(over="ignore", invalid="ignore"):
            diff = np.abs(got[m, ks:ke].astype(np.float64) - want[m, ks:ke].astype(np.float64))
        if live.any():
            worst = max(worst, float((diff[live]/tol[live]).max()))
        assert np.all(diff[live] <= tol[live]), (what, SR.MASKS[m], worst)
    return worst


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
@pytest.mark.parametrize("shape,gc,kind", SEEDED, ids=IDS)
def test_fluxes_from_reference_means(be, shape, gc, kind, dtype):  # noqa: F811
    dev = FluxDev(be, shape, gc, dtype)
    dev.masks()
    g = dev.g
    r = lambda name: SR.ref(shape, gc, dtype, kind, name, be)      # noqa: E731
    nmask = r("nmask")
    nmaskh = nmask[:, 1]
    mean, wmean = dev.tensor(r(SR.FLUX_VAR)), dev.tensor(r("wh"))
    # the exclusion and its cap
    ex = SR.flux_excluded(g, nmask)
    pairs = NM*(g.kmax + 1)
    assert 0 < ex.sum() <= pairs/4 and not ex[SR.MASKS.index("default")].any() and not ex[SR.MASKS.index("sparse")].any()
    none = np.zeros_like(ex)
    jobs = [dev.w_job(c, mean, wmean) for c in SR.W_CASES] + [dev.d_job(c) for c in SR.D_CASES]
    out = dev.s.profiles(jobs).cpu().numpy()
    worst = 0.
    for n, c in enumerate(SR.W_CASES):
        key = SR.w_key(c)
        worst = max(worst, _compare(g, out[n], r("a_" + key), r("scale_" + key), nmaskh, ex, key))
    for n, c in enumerate(SR.D_CASES):
        key = SR.d_key(c)
        worst = max(worst, _compare(g, out[len(SR.W_CASES) + n], r("a_" + key), r("scale_" + key), nmaskh, none, key))
    # advec_2i5: no flux through either wall, whatever the mask
    ks, ke = g.kstart, g.kend
    for n, c in enumerate(SR.W_CASES):
        if c[0] == SR.ADVEC_2I5:
            assert np.all(out[n][nmaskh[:, ks] > 0, ks] == 0) and np.all(out[n][nmaskh[:, ke] > 0, ke] == 0), c
    # _flux = _w + _diff in the finish, the two jobs of the same call
    wc, dc = SR.SUM_CASE
    tot = dev.s.profiles([dev.w_job(wc, mean, wmean), dev.d_job(dc), (dev.fd["a"], 0, S.FLUX_SUM, 0., 0., None, dict(a=0, b=1))]).cpu().numpy()
    scale = r("scale_" + SR.w_key(wc)) + r("scale_" + SR.d_key(dc))
    worst = max(worst, _compare(g, tot[2], r("a_flux"), scale, nmaskh, ex, "flux"))
    assert np.array_equal(tot[0], out[SR.W_CASES.index(wc)]) and np.array_equal(tot[1], out[len(SR.W_CASES) + SR.D_CASES.index(dc)])
    with np.errstate(over="ignore", invalid="ignore"):
        both = (tot[0] + tot[1])[:, ks:ke+1]
    assert np.array_equal(tot[2][:, ks:ke+1][nmaskh[:, ks:ke+1] > 0], both[nmaskh[:, ks:ke+1] > 0])
    print("stats ratio %s %s %s: fluxes %.3g of the bound" % (be.name, SR.case_of(shape, kind).key, SR.tag(dtype), worst))


def test_flux_refusals(be):  # noqa: F811
    dev = FluxDev(be, SR.SHAPES[1], (1, 1, 1), np.float64)
    dev.masks()
    mean = dev.tensor(np.zeros((NM, dev.g.kcells)))
    ok = dev.w_job(SR.W_CASES[0], mean, mean)
    half = (ok[0], 1) + ok[2:]
    with pytest.raises(capi.MhhError, match="half-level variable"):       # w itself: the reference throws
        dev.s.sums([half])
    for scheme in (4, 41, 253):
        with pytest.raises(capi.MhhError, match="advection scheme %d is not built" % scheme):
            dev.s.sums([dev.w_job((scheme, 0, 0), mean, mean)])
    with pytest.raises(capi.MhhError, match="diffusion scheme 4 is not built"):
        dev.s.sums([dev.d_job((4, 0, 0))])
    with pytest.raises(capi.MhhError, match="advec_flux_s_lim is a scalar's"):
        dev.s.sums([dev.w_job((SR.ADVEC_2I5, 1, 1), mean, mean)])
    with pytest.raises(capi.MhhError, match="_flux adds"):
        dev.s.sums([ok, (dev.fd["a"], 0, S.FLUX_SUM, 0., 0., None, dict(a=0, b=0))])
    with pytest.raises(ValueError, match="half-level variable"):
        S.Stats().add("w", dev.fd["wh"], 1, ("mean", "w"), flux=dict(kind=0, visc=0.))
    with pytest.raises(ValueError, match="needs both"):
        S.Stats().add("a", dev.fd["a"], 0, ("mean", "w", "flux"), flux=dict(kind=0, visc=0.))
