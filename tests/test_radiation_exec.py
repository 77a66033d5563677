"""mhh_radiation_gcss_exec and mhh_radiation_gcss_zenith_host (csrc/radiation_gcss.h) against the reference's CPU path.

The reference is the reference's own source behind tests/cpp/ref_radiation_shim.cpp where that tree exists,
tests/golden/radiation_ref.npz elsewhere (tests/radiation_ref.py). With the shim built on this host the emulation build agrees bit
for bit, through exp, pow and sqrt too: thlt from non-zero tendencies with each part and both, lflx, sflx. On the MI355X the device's
exp and pow differ from the host's C library by a few ulp: the bound, relative to each array's largest value, is 8 times the
difference measured against the golden file (profiles/radiation_gcss.md), the factor tests/test_micro_exec.py uses.
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import micro_ref as MR
import moist_ref as M
import radiation_ref as R
from backends import be  # noqa: F401
from microhh_amd import capi

CASES = [(s, gc) for s in R.SHAPES for gc in R.GCS]
IDS = ["%dx%dx%d-gc%d%d%d" % (s + gc) for s, gc in CASES]
# 8 x the largest difference measured on the MI355X against the golden file, relative to the array's maximum, per array
# (profiles/radiation_gcss.md; 150 figures over every run of the golden file and the three ghost layouts). thlt is a difference of
# neighbouring fluxes of 20 to 1000 W m-2 that differ by a few per cent, hence its larger figure. sflx stays four orders below the
# 1e-12 of sw0 that would have asked for a look at the two-stream solution's cancellation.
MEASURED = {np.float64: {"thlt": 8.771e-15, "lflx": 7.723e-17, "sflx": 2.205e-16}, np.float32: {"thlt": 6.838e-6, "lflx": 6.220e-8, "sflx": 1.776e-7}}
BOUND = {dt: {n: 8*v for n, v in m.items()} for dt, m in MEASURED.items()}


def outside(g):
    mask = np.ones(g.shape3, dtype=bool)
    mask[g.interior] = False
    return mask


def check_outside(x, out, day):
    """Nothing outside the interior is written, except sflx's zero fill over all cells; thlt keeps level kstart too."""
    g = x.g
    m = outside(g)
    assert cm.same_bits(out["thlt"][m], x.h["thlt"][m])
    assert cm.same_bits(out["thlt"][g.kstart], x.h["thlt"][g.kstart])
    assert cm.same_bits(out["lflx"][m], x.h["lflx"][m])
    assert cm.same_bits(out["sflx"][m], np.zeros_like(out["sflx"][m]))
    if not day:
        assert cm.same_bits(out["sflx"], np.zeros_like(out["sflx"]))


def test_golden_file_matches_the_cases():
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/radiation_ref.npz"
    for shape in R.SHAPES:
        assert str(z["digest/%s" % R.cloud_case(shape).key]) == R.cloud_case(shape).digest(), "the seeded inputs differ from the recorded ones"
    for dt in cm.DTYPES:
        t = np.dtype(dt).type
        assert t(z["mu/day/%s" % R.tag(dt)][0]) > 0.9 and t(0.035) < t(z["mu/low/%s" % R.tag(dt)][0]) < t(0.06) and t(z["mu/night/%s" % R.tag(dt)][0]) < 0


def test_inputs_cover_the_branches():
    for shape in R.SHAPES:
        c = R.cloud_case(shape)
        ql, qt, kind = c.ql, c.qt, c.kind[0]
        ktot = shape[2]
        for dt in cm.DTYPES:
            t = np.dtype(dt).type
            q = ql.astype(dt)
            pbl = (q > t(0.01E-3)) & (qt.astype(dt) >= t(0.008))
            ki = np.where(pbl.any(axis=0), ktot - 1 - np.argmax(pbl[::-1], axis=0), ktot)     # as an interior index; ktot is kend
            thick = q.astype(np.float64) > 1.E-5
            assert (kind == R.CLEAR).any() and (ki[kind == R.CLEAR] == ktot).all() and not thick[:, kind == R.CLEAR].any()      # clear columns
            assert ((ki == ktot - 1) & ~pbl[:-1].any(axis=0)).any()                           # cloud in the top level only
            assert ((ki == 0) & ~pbl[1:].any(axis=0)).any()                                   # cloud in the bottom level only
            dry = (kind == R.DRYQT)
            assert dry.any() and (ki[dry] == ktot).all() and thick[:, dry].any(axis=0).all()  # qt < 0.008 throughout: ki = kend, lwp > 0
            assert ((ql > 0) & (ql < 1e-5)).any() and (ql < 0).any()
            # float32(1e-5) = 9.99999975e-06 rounds DOWN: a ql equal to it is not above the double 1.E-5 (no optical depth) and not
            # above TF(0.01E-3) in either dtype; the next float up is above the double 1.E-5 and above float32(0.01E-3). Between the
            # two no float lies, so the double and the float comparison part the floats at the same place.
            edge = ql == float(np.float32(1e-5))
            assert edge.any() and not (ql[edge] > 1.E-5).any() and not (q[edge] > t(0.01E-3)).any()
            up = ql == float(np.nextafter(np.float32(1e-5), np.float32(1.)))
            assert up.any() and (ql[up] > 1.E-5).all() and (np.float32(ql[up]) > np.float32(0.01E-3)).all()
            two = kind == R.TWO
            layer = (q > t(5.e-5)).astype(int)           # the cloud proper (1e-4 and more), not the single cells around 1e-5
            runs = (np.diff(np.concatenate([np.zeros((1,) + layer.shape[1:], dtype=int), layer]), axis=0) == 1).sum(axis=0)
            assert two.any() and (runs[two] == 2).all()                                       # two cloud layers with a gap
            assert ((ki > 0) & (ki < ktot - 1)).mean() > 0.5                                  # levels above the inversion in most columns
        assert (kind == R.BAND).mean() > 0.3


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES + [R.KGC2], ids=IDS + ["17x9x8-gc112"])
def test_exec_is_the_references(be, shape, gc, dtype):  # noqa: F811
    """With the shim on this host: every run with LW, SW and both from non-zero tendencies, lflx and sflx, bit for bit, nothing
    written outside the interior; gc = (1, 1, 2) pins the literal-1 layer depth. Elsewhere the runs of the golden file within BOUND."""
    g = R.grid_of(shape, gc, dtype)
    t = np.dtype(dtype).type
    if R.exact_here(be):
        for run in R.RUNS:
            mu = R.mu_of(run[1], dtype, be)
            day = t(mu) > t(0.035)
            assert day == (run[1] in ("day", "low"))
            for parts in (R.LW, R.SW, R.LW | R.SW):
                x = R.Dev(be, shape, gc, dtype)
                got = x.exec(run[0], mu, parts)
                want = R.ref_exec(shape, dtype, run[0], mu, parts, gc=gc)
                check_outside(x, got, day)
                for n in R.OUT:
                    a, b = got[n][g.interior], want[n][g.interior]
                    assert cm.same_bits(a, b), (run, parts, n, M.rel(a, b))
                changed = not cm.same_bits(got["thlt"], x.h["thlt"])
                assert changed == bool(parts & R.LW or day), (run, parts)
                assert x.count() == 0
        return
    figures = []
    for run in R.RUNS:
        names = R.stored(shape, run, gc)
        if not names:
            continue
        mu = R.mu_of(run[1], dtype, be)
        day = t(mu) > t(0.035)
        x = R.Dev(be, shape, gc, dtype, zero_tend=True)
        got = x.exec(run[0], mu)
        check_outside(x, got, day)
        assert x.count() == 0
        for n in names:
            want = R.ref(R.run_key(shape, run, dtype, gc) + n, be)
            have = got[n][g.interior]
            if n == "sflx" and not day:
                assert cm.same_bits(have, want)
                continue
            assert np.max(np.abs(want)) > 0, (run, n)
            e = M.rel(have, want)
            # every figure is printed before any is held against its bound
            print("radiation exec %s%s %s %s: rel %.3e (max %.6g)" % (R.run_key(shape, run, dtype, gc), "gc%d%d%d" % gc, be.name, n, e, np.max(np.abs(want))))
            figures.append((run, n, e))
    assert figures
    for run, n, e in figures:
        assert e <= BOUND[dtype][n], (run, n, e)


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=["%dx%dx%d" % s for s in R.SHAPES])
def test_sweep_and_plain_forms_agree(be, shape, dtype):  # noqa: F811
    """Bit for bit on both backends: the default entry, the sweep form by name and the plain form; each part, fields only, and with
    ql from the saturation adjustment where the plain form's short-wave flux overwrites it."""
    for run in (("dycoms", "day"), ("dycoms", "night")):
        mu = R.mu_of(run[1], dtype, be)
        for parts, kw in ((R.LW | R.SW, {}), (R.LW, {}), (R.SW, {}), (R.LW | R.SW, dict(lflx=False, sflx=False)), (R.LW | R.SW, dict(thlt=False))):
            out = {}
            for impl in (None, R.SWEEP, R.PLAIN):
                x = R.Dev(be, shape, (3, 3, 1), dtype)
                out[impl] = x.exec(run[0], mu, parts, impl, **kw)
                if not kw:
                    check_outside(x, out[impl], run[1] == "day")
            for n in R.OUT:
                assert cm.same_bits(out[None][n], out[R.SWEEP][n]), (run, parts, kw, n)
                assert cm.same_bits(out[R.PLAIN][n], out[R.SWEEP][n]), (run, parts, kw, n, M.rel(out[R.PLAIN][n], out[R.SWEEP][n]))


def moist_inputs(be, shape, gc, dtype):
    """thl, qt and the tables of the warm-rain case of this shape (tests/micro_ref.py): cloud by saturation adjustment."""
    c = MR.rain_case(shape)
    g = MR.grid_of(shape, gc, dtype)
    h = c.inputs(g)
    return g, h, {n: be.arr(h[n]) for n in ("thl", "qt", "p", "exn", "rho")}


@pytest.mark.parametrize("impl", [R.SWEEP, R.PLAIN], ids=["sweep", "plain"])
@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_null_ql_is_the_saturation_adjustment(be, dtype, impl):  # noqa: F811
    """ql = NULL equals the same call fed with mhh_thermo_moist_fields' ql, bit for bit, and nonconv stays 0."""
    shape, gc = (70, 9, 10), (3, 3, 1)
    g, h, d = moist_inputs(be, shape, gc, dtype)
    G = be.grid(g)
    ql = be.arr(np.full(g.shape3, 2.e-3, dtype=dtype))
    B.ok(be, be.lib.mhh_thermo_moist_fields(G, be.ptr(d["thl"]), be.ptr(d["qt"]), be.ptr(d["p"]), be.ptr(d["exn"]), None,
                                            None, be.ptr(ql), None, None, None, be.stream))
    be.sync()
    assert (be.host(ql).reshape(g.shape3)[g.interior] > 1e-5).mean() > 0.02
    mu = R.mu_of("day", dtype, be)
    p = capi.MhhRadiationGcssParams(85., 70., 22., 3.75e-6, mu, R.LW | R.SW)
    out = {}
    for fed in (True, False):
        thlt = be.arr(np.asarray(h["thlt"]))
        lflx, sflx = be.arr(np.full(g.shape3, 555., dtype=dtype)), be.arr(np.full(g.shape3, 444., dtype=dtype))
        scratch = [be.arr(np.full(g.ncells, -9.e9, dtype=dtype)) for _ in range(2)]
        sp = (C.c_void_p*2)(*[be.ptr(a).value for a in scratch])
        keep, cptr, count = M.counter(be)
        B.ok(be, be.lib.mhh_radiation_gcss_exec_impl(G, impl, C.byref(p), be.ptr(thlt), be.ptr(ql) if fed else None, be.ptr(d["thl"]), be.ptr(d["qt"]),
                                                     be.ptr(d["rho"]), be.ptr(d["p"]), be.ptr(d["exn"]), be.ptr(lflx), be.ptr(sflx), sp, cptr, be.stream))
        be.sync()
        assert count() == 0
        out[fed] = [be.host(a).reshape(g.shape3) for a in (thlt, lflx, sflx)]
    for a, b in zip(out[True], out[False]):
        assert cm.same_bits(a, b)
    assert not cm.same_bits(out[True][0], h["thlt"]) and out[True][2][g.interior].max() > 100.


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_zenith_host(be, dtype):  # noqa: F811
    """calc_zenith: bit for bit with the shim on this host; within 4 ulp of the golden mu elsewhere (libm bits do not travel)."""
    t = np.dtype(dtype).type
    for day in R.ZENITH_DAYS:
        for lon in R.ZENITH_LONS:
            mu = C.c_double(0)
            B.ok(be, be.lib.mhh_radiation_gcss_zenith_host(M.code(dtype), R.LAT, lon, day, C.byref(mu)))
            assert float(t(mu.value)) == mu.value, "a value of the dtype"
            want = float(R.ref(R.zenith_key(dtype, lon, day), be)[0])
            print("zenith %s day %g lon %g %s: got %.17g want %.17g" % (R.tag(dtype), day, lon, be.name, mu.value, want))
            if R.exact_here(be):
                assert mu.value == want
            else:
                assert abs(mu.value - want) <= 4*np.spacing(t(abs(want)))
    assert abs(float(R.ref(R.zenith_key(dtype, 0., 160.5), be)[0]) - 0.9867) < 1e-3          # noon at 32.5 N in June
    assert be.lib.mhh_radiation_gcss_zenith_host(M.code(dtype), R.LAT, 0., 160.5, None) != 0 and b"mu" in be.lib.mhh_last_error()


def test_refusals_leave_the_arrays_untouched(be):  # noqa: F811
    shape, gc, dtype = (20, 1, 12), (1, 1, 1), np.float64
    x = R.Dev(be, shape, gc, dtype)
    g, h, d = moist_inputs(be, shape, gc, dtype)
    lib = be.lib
    mu = R.mu_of("day", dtype, be)
    p = x.params("dycoms", mu, R.LW | R.SW)
    a = x.args()
    moist = [be.ptr(d["thl"]), be.ptr(d["qt"]), be.ptr(d["rho"]), be.ptr(d["p"]), be.ptr(d["exn"])]

    def untouched():
        be.sync()
        out = x.out()
        return all(cm.same_bits(out[n], x.h[n]) for n in R.OUT) and all((be.host(s) == -9.e9).all() for s in x.scratch)
    # a NULL ql without thl / pref / exnref
    for drop in (0, 3, 4):
        m = list(moist); m[drop] = None
        assert lib.mhh_radiation_gcss_exec(x.G, C.byref(p), a[0], None, *m, *a[7:]) != 0 and b"without ql" in lib.mhh_last_error()
        assert untouched()
    # no scratch
    assert lib.mhh_radiation_gcss_exec(x.G, C.byref(p), *a[:9], None, *a[10:]) != 0 and b"scratch" in lib.mhh_last_error()
    assert untouched()
    half = (C.c_void_p*2)(be.ptr(x.scratch[0]).value, None)
    assert lib.mhh_radiation_gcss_exec(x.G, C.byref(p), *a[:9], half, *a[10:]) != 0 and b"scratch" in lib.mhh_last_error()
    assert untouched()
    # parts
    for parts in (0, 4, 7):
        assert lib.mhh_radiation_gcss_exec(x.G, C.byref(x.params("dycoms", mu, parts)), *a) != 0 and b"parts" in lib.mhh_last_error()
        assert untouched()
    assert lib.mhh_radiation_gcss_exec_impl(x.G, 5, C.byref(p), *a) != 0 and b"impl" in lib.mhh_last_error()
    assert lib.mhh_radiation_gcss_exec(x.G, None, *a) != 0 and b"params" in lib.mhh_last_error()
    assert lib.mhh_radiation_gcss_exec(x.G, C.byref(p), None, *a[1:7], None, None, *a[9:]) != 0 and b"no output" in lib.mhh_last_error()
    assert untouched()
    B.ok(be, lib.mhh_radiation_gcss_exec(x.G, C.byref(p), *a))
    assert not untouched()
