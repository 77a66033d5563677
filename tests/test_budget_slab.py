"""Budget_2 on a slab (npy > 1): every rank sums its own rows; the double sums of the model profiles, of the mean profiles and of the
terms go through Master.sum_ between the sums kernels and the finish kernels. 2 ranks on the emulation (gloo) at 16 x 32 x 10 against
the single-rank sample of the same global fields. Always: counts equal; every rank holds the same finished values; the fill value
in the same places; the model profiles of the two runs within the bound of budget_ref.bound() with the masked mean of |f| as scale.
Where the reference tree exists also every term profile, within that bound plus what the difference of the two runs' model profiles
does to the terms, which is measured on the single rank (its own passes run once more with the slab's model and mean profiles); the
scale of that bound, the masked mean of |term|, comes from the reference's own term fields. uw_diff included: evisch[ijk+jj] is
unwritten on the DOMAIN's last row only, so the decomposition does not show in any profile."""
import numpy as np

import backends as B
import budget_ref as BR
import stats_ref as SR
from microhh_amd import budget as BU
from microhh_amd import stats as S
from microhh_amd.model import HotPath, synthetic_global
from ranks import run_ranks

GRID = (16, 32, 10)
MASKS = ("default", "wplus", "warm")
THRES = 300.2          # of scalar 0 (300 + 0.003 z +- 0.05 on 1200 m): the upper part of the domain is `warm`


def _make(lib, **kw):
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib, global_init=synthetic_global("drycblles", *GRID), stats=S.Stats(masks=MASKS),
                 budget=BU.Budget2(), **kw)
    hp.stats.mask_thres("warm", hp.s[0], hp.s[0], threshold=THRES)
    hp.cyclic_prognostic()
    # p and evisc as functions of the prognostic fields, cell by cell: the same global fields on every decomposition, ghost cells included
    hp.p.copy_(0.5*hp.u - hp.v)
    hp.evisc.copy_(0.1 + hp.u*hp.u)
    return hp


def _flat(r):
    return {"%s/%s" % (m, k): np.asarray(v) for m, rm in r.items() for k, v in rm.items()}


def _worker(rank, world, out):
    hp = _make(B.get("emul").lib, npy=world, rank=rank)
    out.update(_flat(hp.stats.sample()))
    bs = hp.budget.sampler
    out["model"] = bs.model_profiles(hp.u, hp.v, hp.w).numpy().copy()
    out["means"] = bs.mean_profiles(hp.budget.buoyancy(), hp.p).numpy().copy()
    hp.close()


def test_two_ranks_against_one():
    hp = _make(B.get("emul").lib)
    ref = _flat(hp.stats.sample())
    g, bud = hp.grid, hp.budget
    names = [n for n, _ in bud.names]
    mf, _ = hp.stats.sampler.host_words()
    a, b = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo", args=())
    for key in ref:                                    # every rank holds the same finished values
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(a["model"], b["model"]) and np.array_equal(a["means"], b["means"])
    # the single rank's passes with the slab's model and mean profiles: what their difference does to the terms
    bs = bud.sampler
    bf = bud.buoyancy()
    fields = dict(u=hp.u, v=hp.v, w=hp.w, p=hp.p, evisc=hp.evisc, b=bf, u_fluxbot=hp.surf["u_fluxbot"], v_fluxbot=hp.surf["v_fluxbot"])
    model, means = hp.torch.from_numpy(a["model"]), hp.torch.from_numpy(a["means"])
    given = bs.profiles(bs.desc(bud.groups, fields, model, means, diff_scheme=hp.cfg["diff"])).numpy()
    own_model = bs.model_profiles(hp.u, hp.v, hp.w).numpy()
    h = {k: v.numpy() for k, v in fields.items()}
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    fill = S.fill_value(g.np_dtype)
    worst, checked = 0., 0
    for m, mask in enumerate(MASKS):
        for name in ("nmask", "nmaskh", "area", "areah"):
            assert np.array_equal(a["%s/%s" % (mask, name)], ref["%s/%s" % (mask, name)]), (mask, name)
        nmk = ref["%s/nmask" % mask]
        inmask = (mf[:, js, ie] & SR.flags(m)[0]) != 0
        # the model profiles of the two runs: sums of the same values in another order
        for i, f in enumerate(("u", "v", "w")):
            cnt = ref["%s/%s" % (mask, "nmaskh" if i == 2 else "nmask")]
            fm = (mf[:, js, ie] & SR.flags(m)[1 if i == 2 else 0]) != 0
            sc = (np.abs(h[f][:, js, ie].astype(np.float64))*fm).sum(axis=(1, 2))/np.maximum(cnt, 1)
            assert np.all(np.abs(a["model"][i, m] - own_model[i, m]) <= BR.bound(g, own_model[i, m], sc)), (mask, f)
        for name in names:                                   # reference-free: the fill value in the same places
            key = "%s/%s" % (mask, name)
            assert np.array_equal(a[key] == fill, ref[key] == fill), key
        if not SR.have_reference():
            continue
        par = dict(utrans=0., vtrans=0., fc=0.)
        for name, fld in BR.term_fields(g, h, own_model[0, m], own_model[1, m], own_model[2, m], a["means"][0], a["means"][1], par, groups=bud.groups):
            key = "%s/%s" % (mask, name)
            scale = (np.abs(fld[:, js, ie].astype(np.float64))*inmask).sum(axis=(1, 2))/np.maximum(nmk, 1)
            cube = None
            if name in BR.CUBES:
                cube = np.array([(BR.cube_scale(g, h, own_model[2, m], k)[name]*inmask[k]).sum()/max(nmk[k], 1) if g.kstart <= k <= g.kend else 0.
                                 for k in range(g.kcells)])
            want, got = ref[key], a[key]
            tol = BR.bound(g, want, scale, cube) + np.abs(given[names.index(name), m].astype(np.float64) - want)
            live = want != fill
            ratio = (np.abs(got.astype(np.float64) - want)[live]/tol[live]).max() if live.any() else 0.
            assert ratio <= 1., (key, ratio)
            worst, checked = max(worst, ratio), checked + 1
    print("worst ratio to the bound: %.3g over %d profiles" % (worst, checked))
    assert checked == (3*len(names) if SR.have_reference() else 0)
    hp.close()
