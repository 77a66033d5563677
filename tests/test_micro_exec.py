"""Microphys_2mom_warm::exec, its sedimentation CFL number and Limiter (csrc/microphys_2mom_warm.h) against the reference.

The reference is the reference's own source behind tests/cpp/ref_micro_shim.cpp where that tree exists, tests/golden/micro_ref.npz
elsewhere (tests/micro_ref.py). With the shim built on this host the emulation build agrees bit for bit, through pow, exp and sqrt
too: every process alone through the mask, all together, from non-zero tendencies, rr_bot and the CFL number. On the MI355X the
device's pow and exp differ from the host's C library by a few ulp: the bound, relative to each array's largest value, is 8 times
the difference measured against the golden file (profiles/microphys_2mom_warm.md). Cells whose REFERENCE drop diameter lies within a
relative 1e-12 (fp64) / 1e-5 (fp32) of a jump of the breakup term (0.35 mm, 0.9 mm) are left out of the nrt comparison; the
recording step asserts that the seeded inputs put none there, so the lists in the golden file are empty.
"""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import micro_ref as R
import moist_ref as M
from backends import be  # noqa: F401
from microhh_amd import capi

CASES = [(s, gc) for s in R.SHAPES for gc in R.GCS]
IDS = ["%dx%dx%d-gc%d%d%d" % (s + gc) for s, gc in CASES]
# 8 x the largest difference measured on the MI355X against the golden file, relative to the array's maximum
# (profiles/microphys_2mom_warm.md: 1.33e-15 in fp64, 1.16e-6 in fp32, both on nrt; every other array and the CFL number lie below)
BOUND = {np.float64: 8*1.33e-15, np.float32: 8*1.16e-6}


def kc_of(shape):
    return cm.switches(MHH_MARCH_KC_RT=8 if shape[2] == 40 else None)


def interior2(g):
    return (slice(g.jstart, g.jend), slice(g.istart, g.iend))


def check_outside(x, out):
    """Nothing outside the interior is written: the sentinel of the horizontal ghost cells, the ghost levels, rr_bot's rim."""
    g = x.g
    for n in ("qr", "nr") + R.OUT:
        mask = np.ones(g.shape3, dtype=bool); mask[g.interior] = False
        assert cm.same_bits(out[n][mask], x.h[n][mask]), n
    rim = np.ones(g.shape2, dtype=bool); rim[interior2(g)] = False
    assert cm.same_bits(out["rr_bot"][rim], x.h["rr_bot"][rim])


def test_golden_file_matches_the_cases():
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/micro_ref.npz"
    for shape in R.SHAPES:
        assert str(z["digest/%s" % R.rain_case(shape).key]) == R.rain_case(shape).digest(), "the seeded inputs differ from the recorded ones"
    for k in z.files:
        if k.endswith("excluded"):
            assert z[k].size == 0


def test_inputs_cover_the_branches():
    c = R.rain_case((70, 9, 10))
    inner = (slice(1, -1),)
    qr, nr = c.qr[inner], c.nr[inner]
    rain = qr > 1e-15
    cols = rain.any(axis=0)
    assert 0.3 < cols.mean() < 0.7
    assert (rain[-1] & ~rain[:-1].any(axis=0)).any() and (rain[0] & ~rain[1:].any(axis=0)).any()       # top only, bottom only
    assert (qr < 0).any() and (nr < 0).any() and ((nr > 0) & (nr < 1) & rain).any() and ((qr > 0) & (qr <= 1e-15)).any()
    mr = c.rho[1:-1, None, None]*qr/np.maximum(nr, 1.)
    assert (mr[rain] < 2.6e-10).any() and (mr[rain] > 3e-6).any()


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES, ids=IDS)
def test_exec_is_the_references(be, shape, gc, dtype):  # noqa: F811
    """Every process alone and all together. With the shim on this host: from non-zero tendencies, both steps, bit for bit. Elsewhere
    the runs of the golden file (from zero tendencies) within BOUND."""
    g = R.grid_of(shape, gc, dtype)
    c = R.rain_case(shape)
    worst = {}
    with kc_of(shape):
        if R.exact_here(be):
            for name, mask in list(R.PROCESSES.items()) + [("all", R.ALL)]:
                for dtname in (R.CFLS if mask & R.SEDI else ("hi",)):
                    m = mask | R.CLIP
                    x = R.Dev(be, shape, gc, dtype)
                    got = x.exec(m, c.dt[dtname])
                    want = R.ref_exec(shape, dtype, m, dtname, gc=gc)
                    for n in ("qr", "nr") + R.OUT + ("rr_bot",):
                        assert cm.same_bits(got[n], want[n]), (name, dtname, n, M.rel(got[n], want[n]))
                    for n in R.OUT + ("rr_bot",):
                        if n in R.WRITES[mask]:
                            assert not cm.same_bits(got[n], x.h[n]), (name, n, "the process wrote nothing")
                        else:
                            assert cm.same_bits(got[n], x.h[n]), (name, n, "not this process's to write")
                    assert x.count() == 0
            return
        for s, name, mask, dtname in R.golden_runs():
            if s != shape:
                continue
            x = R.Dev(be, shape, gc, dtype, zero_tend=True)
            got = x.exec(mask, c.dt[dtname])
            check_outside(x, got)
            key = R.run_key(shape, name, dtname, dtype)
            excluded = R.ref(key + "excluded", be)
            for n in R.stored(shape, mask):
                want = R.ref(key + n, be)
                have = got[n][interior2(g)] if n == "rr_bot" else got[n][g.interior]
                if n == "nrt" and excluded.size:
                    assert excluded.size <= 1e-3*np.count_nonzero(got["qr"][g.interior] > 1e-15)
                    have, want = have.copy(), want.copy()
                    have.reshape(-1)[excluded] = 0; want.reshape(-1)[excluded] = 0
                e = M.rel(have, want)
                worst[n] = max(worst.get(n, 0.), e)
                print("micro exec %s %s %s %s %s: rel %.3e" % (R.run_key(shape, name, dtname, dtype), "gc%d%d%d" % gc, be.name, n, "max", e))
                assert np.max(np.abs(want)) > 0, (name, n)
                assert e <= BOUND[dtype], (name, dtname, n, e)
            assert x.count() == 0


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=["%dx%dx%d" % s for s in R.SHAPES])
def test_marching_and_cell_forms_agree(be, shape, dtype):  # noqa: F811
    """Bit for bit on both backends: the default entry, the marching form by name and the cell form, everything at once and (on the
    small shapes) each process alone."""
    c = R.rain_case(shape)
    masks = [R.ALL] + ([m | R.CLIP for m in R.PROCESSES.values()] + [R.SEDI, R.EVAP | R.SCBR] if shape in R.SMALL else [])
    with kc_of(shape):
        for mask in masks:
            out = {}
            for impl in (None, R.MARCH, R.CELL):
                x = R.Dev(be, shape, (3, 3, 1), dtype)
                out[impl] = x.exec(mask, c.dt["hi"], impl)
                check_outside(x, out[impl])
            for n in ("qr", "nr") + R.OUT + ("rr_bot",):
                assert cm.same_bits(out[None][n], out[R.MARCH][n]), (mask, n)
                assert cm.same_bits(out[R.CELL][n], out[R.MARCH][n]), (mask, n, M.rel(out[R.CELL][n], out[R.MARCH][n]))


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_clipping_and_untouched_cells(be, dtype):  # noqa: F811
    """remove_negative_values alone: max(0, .) on the interior of qr and nr, nothing else. With the local processes: a cell with
    ql <= ql_min and qr <= qr_min keeps the bits of its four tendencies."""
    shape, gc = (70, 9, 10), (3, 3, 1)
    c = R.rain_case(shape)
    x = R.Dev(be, shape, gc, dtype)
    g = x.g
    got = x.exec(R.CLIP, c.dt["hi"])
    for n in ("qr", "nr"):
        want = x.h[n].copy()
        want[g.interior] = np.maximum(dtype(0.), want[g.interior])
        assert cm.same_bits(got[n], want), n
        assert (x.h[n][g.interior] < 0).any() and (want[0] < 0).any() and (want[-1] < 0).any()       # negative ghost levels stay
    for n in R.OUT:
        assert cm.same_bits(got[n], x.h[n]), n
    # ql from the library's own diagnostic (the warm branch: max(0, qt - qs), bit-exact on both backends)
    ql = be.zeros(g.shape3, dtype)
    B.ok(be, be.lib.mhh_thermo_moist_fields(x.G, be.ptr(x.d["thl"]), be.ptr(x.d["qt"]), be.ptr(x.d["p"]), be.ptr(x.d["exn"]), None,
                                            None, be.ptr(ql), None, None, None, be.stream))
    be.sync()
    ql = be.host(ql).reshape(g.shape3)[g.interior]
    y = R.Dev(be, shape, gc, dtype)
    got = y.exec(R.AUTO | R.ACCR | R.EVAP | R.SCBR | R.CLIP, c.dt["hi"])
    idle = (ql <= 1e-6) & (got["qr"][g.interior] <= 1e-15)
    busy = (ql > 1e-6) & (got["qr"][g.interior] > 1e-15)
    assert idle.mean() > 0.2 and busy.mean() > 0.02
    for n in R.OUT:
        assert cm.same_bits(got[n][g.interior][idle], y.h[n][g.interior][idle]), n
        assert (got[n][g.interior][busy] != y.h[n][g.interior][busy]).any(), n
    assert y.count() == 0


@pytest.mark.parametrize("dtype", cm.DTYPES)
def test_local_processes_move_water_between_qt_and_qr(be, dtype):  # noqa: F811
    """With SEDI off and zero tendencies qtt == -qrt: each of autoconversion, accretion and evaporation adds x to one and subtracts
    it from the other."""
    shape = (17, 9, 8)
    x = R.Dev(be, shape, (1, 1, 1), dtype, zero_tend=True)
    got = x.exec(R.AUTO | R.ACCR | R.EVAP | R.SCBR | R.CLIP, R.rain_case(shape).dt["hi"])
    g = x.g
    assert np.array_equal(got["qtt"][g.interior], -got["qrt"][g.interior])
    assert np.count_nonzero(got["qrt"][g.interior]) > 0.2*got["qrt"][g.interior].size


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("dtname", list(R.CFLS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=["%dx%dx%d" % s for s in R.SHAPES])
def test_sedimentation_conserves_and_never_overdraws(be, shape, dtname, dtype):  # noqa: F811
    """Sedimentation alone from zero tendencies. The flux form telescopes and the flux at kend is zero: per column
    sum_k rho dz qrt == -rr_bot within ktot x eps x the largest term. The limiter of the flux keeps qr + dt qrt >= 0: within
    ktot x eps of what the level holds and receives (its content plus everything that entered the column above it, as a mixing
    ratio of the level: the magnitudes the update is rounded at)."""
    c = R.rain_case(shape)
    dt = c.dt[dtname]
    with kc_of(shape):
        x = R.Dev(be, shape, (3, 3, 1), dtype, zero_tend=True)
        got = x.exec(R.SEDI | R.CLIP, dt)
    g = x.g
    eps = np.finfo(dtype).eps
    rdz = (x.h["rho"].astype(np.float64)*g.dz.astype(np.float64))[g.kstart:g.kend, None, None]
    for n, rate in (("qr", got["rr_bot"][interior2(g)].astype(np.float64)), ("nr", None)):
        tend = got[n + "t"][g.interior].astype(np.float64)
        a = got[n][g.interior].astype(np.float64)
        terms = rdz*tend
        if rate is not None:
            assert (rate >= 0).all() and rate.max() > 0
            bound = g.kmax*eps*np.maximum(np.abs(terms).max(axis=0), np.abs(rate))
            assert (np.abs(terms.sum(axis=0) + rate) <= bound).all(), float(np.max(np.abs(terms.sum(axis=0) + rate) - bound))
        moved = np.cumsum(np.abs(terms)[::-1], axis=0)[::-1]
        scale = a + dt*moved/rdz
        assert (a + dt*tend >= -g.kmax*eps*scale).all(), n
    assert np.count_nonzero(got["qrt"][g.interior]) > 0.1*got["qrt"][g.interior].size
    if dtname == "hi":          # the step the limiter is for: somewhere a level is emptied
        a, tend = got["qr"][g.interior].astype(np.float64), got["qrt"][g.interior].astype(np.float64)
        assert ((a > 1e-15) & (a + dt*tend <= 8*eps*a)).any()


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES, ids=IDS)
def test_sedimentation_cfl(be, shape, gc, dtype):  # noqa: F811
    """calc_max_sedimentation_cfl for both steps, and its floor of 1e-5 on a field without rain."""
    c = R.rain_case(shape)
    x = R.Dev(be, shape, gc, dtype)
    for dtname in R.CFLS:
        got = x.cfl(c.dt[dtname])
        want = float(R.ref("cfl/%dx%dx%d/%s/%s" % (shape + (dtname, R.tag(dtype))), be)[0])
        print("micro cfl %s %s %s: got %.17g want %.17g rel %.3e" % (c.key, dtname, be.name, got, want, abs(got - want)/want))
        if R.exact_here(be):
            assert got == want
        else:
            assert abs(got - want) <= BOUND[dtype]*want
        assert 0.8*R.CFLS[dtname] < want < 1.2*R.CFLS[dtname]
    h = c.inputs(x.g)
    h["qr"][:] = 0
    dry = R.Dev(be, shape, gc, dtype, host=h)
    assert dry.cfl(1.0) == float(dtype(1e-5))


def limiter_numpy(g, at, a, dt):
    """tendency_limiter in numpy's own IEEE arithmetic of the dtype: + - * / only, one rounding per operation."""
    t = g.np_dtype.type
    dt = t(dt)
    dti = t(1.)/dt
    eps = t(np.finfo(np.float64).eps)
    out = at.copy()
    i = g.interior
    a_new = a[i] + dt*at[i]
    out[i] = at[i] + np.where(a_new < 0, (-a_new + eps)*dti, t(0.))
    return out


@pytest.mark.parametrize("dtype", cm.DTYPES)
@pytest.mark.parametrize("shape,gc", CASES[:6], ids=IDS[:6])
def test_limiter_is_bit_exact(be, shape, gc, dtype):  # noqa: F811
    c = R.rain_case(shape)
    g = R.grid_of(shape, gc, dtype)
    a = c.embed(np.asarray(c.qr, dtype=dtype), g)
    at = c.embed(np.asarray(-40.*c.tend0["qrt"] - 1.e-7, dtype=dtype), g)
    dt = 2.5
    want = limiter_numpy(g, at, a, dt)
    if R.have_reference():
        assert cm.same_bits(want, R.ref_limiter(g, at, a, dt))
    d_at, d_a = be.arr(at), be.arr(a)
    B.ok(be, be.lib.mhh_limiter_exec(be.grid(g), be.ptr(d_at), be.ptr(d_a), dt, be.stream))
    be.sync()
    got = be.host(d_at).reshape(g.shape3)
    assert cm.same_bits(got, want)
    i = g.interior
    changed = got[i] != at[i]
    assert 0.1 < changed.mean() < 0.9
    assert (a[i][changed].astype(np.float64) + dt*got[i][changed].astype(np.float64) > -1e-6*np.abs(a[i][changed]) - 1e-12).all()


def test_refusals_name_their_reason(be):  # noqa: F811
    x = R.Dev(be, (20, 1, 12), (1, 1, 1), np.float64)
    d = x.d
    a = [be.ptr(d[n]) for n in ("qr", "nr", "thl", "qt", "qrt", "nrt", "thlt", "qtt", "rr_bot", "rho", "p", "exn")] + [x.scratch_ptrs, None, be.stream]
    p = capi.MhhMicroParams(R.NC0, 10., R.ALL)
    lib = be.lib
    assert lib.mhh_micro_2mom_warm_exec_impl(x.G, 7, C.byref(p), *a) != 0 and b"impl" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(p), None, *a[1:]) != 0 and b"null field" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(p), *a[:12], None, None, be.stream) != 0 and b"scratch" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(p), *a[:2], None, *a[3:]) != 0 and b"local processes" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(capi.MhhMicroParams(R.NC0, 10., 64)), *a) != 0 and b"processes" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(capi.MhhMicroParams(R.NC0, 0., R.ALL)), *a) != 0 and b"dt" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_exec(x.G, C.byref(capi.MhhMicroParams(0., 10., R.ALL)), *a) != 0 and b"Nc0" in lib.mhh_last_error()
    assert lib.mhh_limiter_exec(x.G, a[4], a[0], 0., be.stream) != 0 and b"dt" in lib.mhh_last_error()
    assert lib.mhh_micro_2mom_warm_cfl(x.G, a[0], a[1], a[9], 1., None, None, be.stream) != 0 and b"work" in lib.mhh_last_error()
    # sedimentation off: no scratch and no rr_bot needed
    p = capi.MhhMicroParams(R.NC0, 10., R.ALL & ~R.SEDI)
    B.ok(be, lib.mhh_micro_2mom_warm_exec(x.G, C.byref(p), *a[:8], None, *a[9:12], None, None, be.stream))
    be.sync()
