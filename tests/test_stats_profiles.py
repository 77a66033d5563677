"""The profiles and time series of csrc/stats.h against the reference's own kernels (src/stats.cxx behind tests/cpp/ref_stats_shim.cpp,
or tests/golden/stats_ref.npz).

Bit for bit on every backend: frac and cover (sums of zeros and ones), the fill-value positions of every profile, and every profile
of the exact fixture, whose partial sums are exact in any order. Within the derived bound of stats_ref.bound(): pass A against the
reference's means; pass B, GIVEN the reference's own mean profiles as its input means so that both sides sum the same terms. path:
the reference accumulates serially in the dtype, so its bound is m eps sum|t| / nmask_proj, m the number of terms.
Every test prints the largest ratio of difference to bound it saw (pytest -s shows it)."""
import numpy as np
import pytest

import common as cm
import stats_ref as SR
from backends import be  # noqa: F401
from microhh_amd import stats as S

SEEDED = [c for c in SR.all_cases() if c[2] == "seeded"]
IDS = ["%s-gc%d%d%d" % ((SR.case_of(s, k).key,) + gc) for s, gc, k in SEEDED]
NM = len(SR.MASKS)


def _jobs(dev, r, ops):
    """The jobs of VARS restricted to `ops`, moments fed the reference's means: (names, job tuples)."""
    names, jobs = [], []
    for var, loc, off, thr, vops in SR.VARS:
        for op in vops:
            if op in ops:
                mean = dev.tensor(r(var)) if op in ("2", "3", "4") else None
                names.append((var, loc, off, op)); jobs.append((dev.d[var], loc, SR.OPCODE[op], off, thr, mean))
    return names, jobs


def _check(dev, r, names, got, exact=False, masks=range(NM)):
    """got[job][mask][kcells] against the reference over kstart .. kend; returns the largest |difference| / bound."""
    g = dev.g
    ks, ke = g.kstart, g.kend + 1
    mf, nmask = r("mfield").astype(np.uint32), r("nmask")
    fill = S.fill_value(g.np_dtype)
    worst = 0.
    for n, (var, loc, off, op) in enumerate(names):
        want = r(S.prof_name(var, op))
        assert got[n].dtype == want.dtype
        for m in masks:
            half = (1 - loc) if op == "grad" else loc
            gk, wk = got[n, m, ks:ke], want[m, ks:ke]
            what = "%s of %s under %s" % (op, var, SR.MASKS[m])
            assert np.array_equal(gk == fill, wk == fill) and np.array_equal(wk == fill, nmask[m, half, ks:ke] == 0), what     # fill positions
            assert np.array_equal(got[n, m] == fill, nmask[m, half] == 0), what                                               # over all levels
            outside = np.r_[0:g.kstart, g.kend + 1:g.kcells]                # a mean carries its offset there too (stats.cxx:1635), over zero
            assert np.array_equal(got[n, m][outside], want[m][outside]), what
            if exact or op == "frac":
                assert np.array_equal(gk, wk), what
                continue
            live = wk != fill
            mean = r(var)[m] if op in ("2", "3", "4") else None
            scale = SR.term_scale(dev.h, g, var, op, off, mean, mf, SR.flags(m)[half], nmask[m, half])[ks:ke]
            tol = SR.bound(g, wk, scale)
            diff = np.abs(gk.astype(np.float64) - wk.astype(np.float64))
            ratio = float((diff[live]/tol[live]).max()) if live.any() else 0.
            worst = max(worst, ratio)
            assert np.all(diff[live] <= tol[live]), "%s: %.3g of the bound" % (what, ratio)
    return worst


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
@pytest.mark.parametrize("shape,gc,kind", SEEDED, ids=IDS)
def test_pass_a_means_and_pass_b_from_reference_means(be, shape, gc, kind, dtype):  # noqa: F811
    dev = SR.Dev(be, shape, gc, dtype, kind)
    dev.masks()
    r = lambda name: SR.ref(shape, gc, dtype, kind, name, be)      # noqa: E731
    na, ja = _jobs(dev, r, ("mean",))
    ja.append((dev.d["bot"], 0, S.MEAN2D, SR.BOT_OFFSET, 0., None))
    outa = dev.s.profiles(ja).cpu().numpy()
    wa = _check(dev, r, na, outa)
    # calc_stats_2d: one value per mask, every mask the same
    want = r("bot")[0]
    got = outa[len(na), :, 0]
    n = dev.g.itot*dev.g.jtot
    tol = 4.*n*2.**-53*np.abs(dev.h["bot"][dev.g.jstart:dev.g.jend, dev.g.istart:dev.g.iend]).mean() + np.spacing(dev.g.np_dtype.type(abs(want)))
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol) and np.all(got == got[0])
    nb, jb = _jobs(dev, r, ("2", "3", "4", "frac", "grad"))
    outb = dev.s.profiles(jb).cpu().numpy()
    wb = _check(dev, r, nb, outb)
    print("stats ratio %s %s %s: pass A %.3g, pass B %.3g of the bound" % (be.name, SR.case_of(shape, kind).key, SR.tag(dtype), wa, wb))


def _columns(dev, r):
    var, loc, off, thr, _ = SR.VARS[2]
    return dev.s.columns(dev.d[var], loc, off, thr, dev.d["rho"]).cpu().numpy(), r(var + "_columns")


def _path_tol(dev, r, m):
    """m eps sum|t| / nmask_proj of mask m: the terms are data*rho*dz of the masked cells."""
    g = dev.g
    var, loc = SR.VARS[2][0], SR.VARS[2][1]
    inner = g.interior
    mk = (r("mfield").astype(np.uint32)[inner] & SR.flags(m)[loc]) != 0
    t = np.abs(dev.h[var][inner].astype(np.float64)*dev.h["rho"][g.kstart:g.kend, None, None]*g.dz[g.kstart:g.kend, None, None])[mk]
    ncol = int(mk.any(axis=0).sum())
    eps = 2.**-53 if g.np_dtype == np.float64 else 2.**-24
    return (t.size*eps*t.sum()/ncol if ncol else 0.), ncol


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
@pytest.mark.parametrize("shape,gc,kind", SEEDED, ids=IDS)
def test_cover_bit_for_bit_and_path_within_its_bound(be, shape, gc, kind, dtype):  # noqa: F811
    dev = SR.Dev(be, shape, gc, dtype, kind)
    dev.masks()
    r = lambda name: SR.ref(shape, gc, dtype, kind, name, be)      # noqa: E731
    got, want = _columns(dev, r)
    assert got.dtype == want.dtype and np.array_equal(got[:, 0], want[:, 0])
    worst = 0.
    for m in range(NM):
        tol, ncol = _path_tol(dev, r, m)
        assert ncol == int(want[m, 2]) and ncol > 0
        diff = abs(float(got[m, 1]) - float(want[m, 1]))
        worst = max(worst, diff/tol)
        assert diff <= tol, "path under %s: %.3g of the bound" % (SR.MASKS[m], diff/tol)
    print("stats ratio %s %s %s: path %.3g of the bound" % (be.name, SR.case_of(shape, kind).key, SR.tag(dtype), worst))


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
def test_path_quirk_and_the_mask_without_a_column(be, dtype):  # noqa: F811
    """calc_path lets every column at or after the first non-empty one in, and those add their masked cells alone: a mask whose first
    non-empty column is neither the first nor in the first row gives the reference's value; a mask without a column gives 0 / 0."""
    shape, gc = SR.QUIRK
    dev = SR.Dev(be, shape, gc, dtype, "quirk")
    dev.masks()
    r = lambda name: SR.ref(shape, gc, dtype, "quirk", name, be)      # noqa: E731
    g = dev.g
    got, want = _columns(dev, r)
    none, late = SR.MASKS.index("sparse"), SR.MASKS.index("topless")
    assert r("nmask")[none].max() == 0 and want[none, 2] == 0
    assert np.isnan(want[none, 1]) and np.isnan(got[none, 1]) and got[none, 0] == 0 and want[none, 0] == 0
    mk = (r("mfield").astype(np.uint32)[g.interior] & SR.flags(late)[0]) != 0
    first = int(np.flatnonzero(mk.any(axis=0).reshape(-1))[0])
    assert first >= 2*g.itot + 3 and first % g.itot != 0                       # not the first column, not in the first row
    assert np.array_equal(got[:, 0], want[:, 0])
    for m in (0, late):
        tol, ncol = _path_tol(dev, r, m)
        assert ncol == int(want[m, 2]) and abs(float(got[m, 1]) - float(want[m, 1])) <= tol
    # the profiles of the empty mask are fill values throughout, those of the others stay within the bound
    na, ja = _jobs(dev, r, ("mean",))
    outa = dev.s.profiles(ja).cpu().numpy()
    _check(dev, r, na, outa)
    assert np.all(outa[:, none] == S.fill_value(dtype))


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
def test_exact_fixture_bit_for_bit(be, dtype):  # noqa: F811
    """Multiples of 1/4 on a power-of-two grid: every partial sum is exact in any order, so every profile, the time series of the 2-D
    field, cover and path have the reference's bits. Means and what does not read a mean: every mask; moments: the default mask (under
    the others a mean is no longer a short binary fraction)."""
    shape, gc = SR.EXACT
    dev = SR.Dev(be, shape, gc, dtype, "exact")
    dev.masks()
    r = lambda name: SR.ref(shape, gc, dtype, "exact", name, be)      # noqa: E731
    na, ja = _jobs(dev, r, ("mean",))
    ja.append((dev.d["bot"], 0, S.MEAN2D, SR.BOT_OFFSET, 0., None))
    outa = dev.s.profiles(ja)
    _check(dev, r, na, outa.cpu().numpy(), exact=True)
    assert outa.cpu().numpy()[len(na), 0, 0] == r("bot")[0]
    nb, jb = _jobs(dev, r, ("frac", "grad"))
    _check(dev, r, nb, dev.s.profiles(jb).cpu().numpy(), exact=True)
    # the moments from the DEVICE's own means: the two passes chained as sample() chains them
    names, jobs = [], []
    for n, (var, loc, off, op) in enumerate(na):
        for p in ("2", "3", "4"):
            if p in [v for v in SR.VARS if v[0] == var][0][4]:
                names.append((var, loc, off, p)); jobs.append((dev.d[var], loc, SR.OPCODE[p], off, 0., outa[n]))
    _check(dev, r, names, dev.s.profiles(jobs).cpu().numpy(), exact=True, masks=[0])
    got, want = _columns(dev, r)
    assert np.array_equal(got, want[:, :2])


def test_the_same_bits_on_every_run(be):  # noqa: F811
    """No floating-point atomics: two runs of every pass give the same bits (two row chunks, the second ragged)."""
    shape, gc = SR.SHAPES[3], (1, 1, 1)
    dev = SR.Dev(be, shape, gc, np.float32)
    r = lambda name: SR.ref(shape, gc, np.float32, "seeded", name, be)      # noqa: E731
    runs = []
    for _ in range(2):
        dev.masks()
        na, ja = _jobs(dev, r, ("mean",))
        nb, jb = _jobs(dev, r, ("2", "3", "4", "frac", "grad"))
        runs.append([dev.s.profiles(ja).cpu().numpy(), dev.s.profiles(jb).cpu().numpy(), _columns(dev, r)[0], dev.s.nmask.cpu().numpy()])
    for a, b in zip(*runs):
        assert np.array_equal(a, b, equal_nan=True)
    assert be.lib.mhh_stats_chunk_rows() < shape[1] < 2*be.lib.mhh_stats_chunk_rows()
