"""Budget_2 on the device (csrc/budget_2.h) against the reference's own translation unit (tests/budget_ref.py).

Every profile of every group that is built, under the three masks of stats_ref.MASKS, in both dtypes: bit for bit on the exact
fixture, within the derived bound of budget_ref.bound on the seeded ones, with the reference's model profiles (which isolates the
term kernels) and with the library's own, end to end. The emulation backend runs against the live reference where its tree
exists; the hip backend (marked gpu) against tests/golden/budget_ref.npz.
"""
import numpy as np
import pytest

import common as cm
import backends as B
from backends import be  # noqa: F401
import budget_ref as BR
import stats_ref as R
from microhh_amd import budget as BU
from microhh_amd import capi
from microhh_amd import stats as S
from microhh_amd.grid import DIFF_SMAG2, DIFF_2

DTYPES = cm.DTYPES
GRAV = 9.81                    # Constants::grav of the reference
SEEDED = [pytest.param(s, gc, k, id="%dx%dx%d-%d%d%d" % (s + gc)) for s, gc, k in BR.LAYOUTS]


def test_record_golden():
    """MHH_RECORD_BUDGET_GOLDEN=1 writes tests/golden/budget_ref.npz from the shim; otherwise the file must match the cases."""
    BR.record_if_asked()
    z = BR.golden()
    assert z is not None, "tests/golden/budget_ref.npz is missing"
    for shape, gc, kind in BR.all_cases():
        c = BR.case_of(shape, kind)
        assert str(z["digest/%s" % c.key]) == c.digest(), "the golden file was recorded from other inputs"


@pytest.mark.skipif(not R.have_reference(), reason="reference tree not present on this machine")
def test_golden_is_the_reference():
    """The recorded profiles are what the reference gives here, bit for bit."""
    z, rec = BR.golden(), BR.computed()
    assert sorted(z.files) == sorted(rec)
    for k in rec:
        a, b = np.asarray(z[k]), np.asarray(rec[k])
        if a.dtype.kind == "f":
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        else:
            assert np.array_equal(a, b), k


def test_exact_fixture_is_exact():
    """The fixture proves itself: the reference's fp32 profiles, widened, are its fp64 profiles bit for bit, every group, default mask."""
    shape, gc, kind = BR.EXACT
    for names in BR.GROUPS.values():
        for name in names:
            a = BR.ref(shape, gc, np.float64, kind, name)[0]
            b = BR.ref(shape, gc, np.float32, kind, name)[0]
            assert np.array_equal(a, b.astype(np.float64)), name
            assert np.abs(a).max() < 1.e30                          # no level of the default mask is empty


def device_profiles(dev, own_model, groups=BR.ALL, ref_args=None):
    """{name: [nmasks][kcells]} and the model profiles; own_model: the library's calc_mask_mean_profile and mean profiles, else the
    reference's."""
    be_, bs, par = dev.be, dev.b, BR.PARAMS[dev.kind]
    f = dev.fields()
    if own_model:
        model, means = bs.model_profiles(f["u"], f["v"], f["w"]), bs.mean_profiles(f["b"], f["p"])
    else:
        shape, gc, dtype, kind = ref_args
        model = dev.tensor(np.stack([BR.ref(shape, gc, dtype, kind, n, be_) for n in ("umodel", "vmodel", "wmodel")]))
        means = dev.tensor(np.stack([BR.ref(shape, gc, dtype, kind, n, be_) for n in ("bmean", "pmean")]))
    d = bs.desc(groups, f, model, means, utrans=par["utrans"], vtrans=par["vtrans"], fc=par["fc"], diff_scheme=DIFF_SMAG2)
    out = bs.profiles(d)
    be_.sync()
    out, names = out.cpu().numpy(), bs.names(groups)
    return {n: out[i] for i, (n, _) in enumerate(names)}, model.cpu().numpy(), means.cpu().numpy()


def test_names(be):
    """The name table is Budget_2::create's, with its z / zh tags, in the order of the groups."""
    dev = BR.Dev(be, *BR.EXACT[:2], np.float64, "exact")
    names = dev.b.names(BR.ALL)
    assert [n for n, _ in names] == [n for G in sorted(BR.GROUPS) for n in BR.GROUPS[G]]
    zh = {n for n, loc in names if loc == "zh"}
    assert zh == {"uw_shear", "vw_shear", "w2_turb", "uw_turb", "vw_turb", "uw_cor", "vw_cor", "w2_pres", "uw_pres", "vw_pres", "w2_rdstr", "uw_rdstr",
                  "vw_rdstr", "w2_diff", "uw_diff", "vw_diff", "w2_buoy", "uw_buoy", "vw_buoy", "bw_buoy", "bw_shear", "bw_turb", "bw_pres", "bw_rdstr"}
    for G, ns in BR.GROUPS.items():
        assert [n for n, _ in dev.b.names(1 << G)] == list(ns)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact(be, dtype):
    """Bit for bit under the default mask: every operand, sign, level range and quirk, the cubes included (an exactly representable
    cube comes out of pow exact)."""
    shape, gc, kind = BR.EXACT
    dev = BR.Dev(be, shape, gc, dtype, kind)
    dev.masks()
    assert np.array_equal(dev.s.nmask.cpu().numpy(), BR.ref(shape, gc, dtype, kind, "nmask", be))
    got, model, means = device_profiles(dev, True)
    for i, n in enumerate(("umodel", "vmodel", "wmodel")):
        assert np.array_equal(model[i][0], BR.ref(shape, gc, dtype, kind, n, be)[0]), n
    for i, n in enumerate(("bmean", "pmean")):
        assert np.array_equal(means[i], BR.ref(shape, gc, dtype, kind, n, be)), n
    bad = [n for n in got if not np.array_equal(got[n][0], BR.ref(shape, gc, dtype, kind, n, be)[0])]
    assert not bad, bad


@pytest.mark.parametrize("own_model", [False, True], ids=["refmodel", "ownmodel"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,gc,kind", SEEDED)
def test_seeded(be, shape, gc, kind, dtype, own_model):
    """All three masks, every group, every (mask, level) pair: the fill value in the same places, elsewhere within the bound."""
    dev = BR.Dev(be, shape, gc, dtype, kind)
    dev.masks()
    g = dev.g
    nmask = BR.ref(shape, gc, dtype, kind, "nmask", be)
    assert np.array_equal(dev.s.nmask.cpu().numpy(), nmask)
    got, model, means = device_profiles(dev, own_model, ref_args=(shape, gc, dtype, kind))
    fill = S.fill_value(dtype)
    worst = {}
    words = dev.s.host_words()[0][:, g.jstart:g.jend, g.istart:g.iend]
    if own_model:
        # calc_mask_mean_profile over 0 .. kcells-1 and the unmasked means: sums of n values in another order
        for i, n in enumerate(("umodel", "vmodel", "wmodel", "bmean", "pmean")):
            want = BR.ref(shape, gc, dtype, kind, n, be)
            have = model[i] if i < 3 else means[i-3]
            fld = np.abs(dev.hb[n[0]][:, g.jstart:g.jend, g.istart:g.iend].astype(np.float64))
            if i < 3:                                          # S_k: the masked mean of |f|, u and v under flag, w under flagh
                half = 1 if i == 2 else 0
                scale = np.stack([(fld*((words & R.flags(m)[half]) != 0)).sum(axis=(1, 2))/np.maximum(nmask[m, half], 1) for m in range(len(BR.MASKS))])
            else:
                scale = fld.mean(axis=(1, 2))
            ratio = np.abs(have.astype(np.float64) - want)/BR.bound(g, want, scale)
            worst[n] = ratio.max()
    for G, names in BR.GROUPS.items():
        for name in names:
            want = BR.ref(shape, gc, dtype, kind, name, be)
            assert np.array_equal(got[name] == fill, want == fill), name
            assert np.array_equal(want == fill, nmask[:, 0] == 0), name
            scale = BR.ref(shape, gc, dtype, kind, "scale_" + name, be)
            cube = BR.ref(shape, gc, dtype, kind, "cube_" + name, be) if name in BR.CUBES else None
            ok = want != fill
            with np.errstate(over="ignore", invalid="ignore"):
                ratio = np.where(ok, np.abs(got[name].astype(np.float64) - want)/BR.bound(g, want, scale, cube), 0.)
            worst[G] = max(worst.get(G, 0.), ratio.max())
    print("worst ratio to the bound %s %s %s: " % (shape, R.tag(dtype), "own" if own_model else "ref") + ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert all(v <= 1. for v in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic(be, dtype):
    """Two runs on the same inputs give the same bits."""
    shape, gc, kind = BR.LAYOUTS[2]
    dev = BR.Dev(be, shape, gc, dtype, kind)
    dev.masks()
    a, ma, _ = device_profiles(dev, True)
    b, mb, _ = device_profiles(dev, True)
    assert np.array_equal(ma.view(np.uint8), mb.view(np.uint8))
    for n in a:
        assert np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)), n


def test_refusals(be):
    """MHH_EINVAL with a message: a fourth-order grid; the LES diffusion group with one ghost cell, with another scheme, without
    evisc; the buoyancy groups without b; an unknown group bit."""
    shape, gc, kind = BR.LAYOUTS[0]
    dev = BR.Dev(be, shape, gc, np.float64, kind)
    dev.masks()
    bs, f = dev.b, dev.fields()
    model, means = bs.model_profiles(f["u"], f["v"], f["w"]), bs.mean_profiles(f["b"], f["p"])

    def refused(match, **kw):
        args = dict(groups=BU.KE, fields=f, model=model, means=means, diff_scheme=DIFF_SMAG2)
        args.update(kw)
        with pytest.raises(capi.MhhError, match=match):
            bs.profiles(bs.desc(**args))
    refused("second-order", order=4)
    refused("diff_smag2 only", groups=BU.DIFF, diff_scheme=DIFF_2)
    refused("needs evisc", groups=BU.DIFF, fields={k: v for k, v in f.items() if k != "evisc"})
    refused("need b", groups=BU.BUOY, fields={k: v for k, v in f.items() if k != "b"})
    refused("need b", groups=BU.PRES_S, fields={k: v for k, v in f.items() if k != "b"})
    refused("unknown group bit", groups=1 << 11)
    refused("unknown group bit", groups=0)
    one = BR.Dev(be, shape, (1, 1, 1), np.float64, kind)
    one.masks()
    f1 = one.fields()
    with pytest.raises(capi.MhhError, match="two horizontal ghost cells"):
        one.b.profiles(one.b.desc(BU.DIFF, f1, one.b.model_profiles(f1["u"], f1["v"], f1["w"]), diff_scheme=DIFF_SMAG2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dry_buoyancy(be, dtype):
    """mhh_thermo_dry_buoyancy: calc_buoyancy (src/thermo_dry.cxx:51-63), one expression, restated in the dtype: bit for bit on all
    kcells levels of the interior columns."""
    shape, gc, kind = BR.LAYOUTS[0]
    g = BR.grid_of(shape, gc, dtype, kind)
    t = g.np_dtype
    th = (300. + BR.case_of(shape, kind).host(g)["b"]).astype(t)
    thref = (300. + 0.01*np.arange(g.kcells)).astype(t)
    b, dth, dthref = be.zeros(g.shape3, dtype), be.arr(th), be.arr(thref)         # held until the call has run: ptr keeps no reference
    B.ok(be, be.lib.mhh_thermo_dry_buoyancy(be.grid(g), be.ptr(b), be.ptr(dth), be.ptr(dthref), GRAV, be.stream))
    be.sync()
    want = (t.type(GRAV)/thref)[:, None, None] * (th - thref[:, None, None])
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    assert np.array_equal(be.host(b)[:, js, ie], want.astype(t)[:, js, ie])
