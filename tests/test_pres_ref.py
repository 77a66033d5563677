"""Pin the pressure solver, the cyclic fills and the horizontal means to the reference's own code (tests/pres_ref.py).

Two halves. (1) The ORACLE against the reference, bit for bit, fp64 and fp32: the coefficient tables of Pres_2 / Pres_4::set_values;
Pres::input with its ghost-cell side effects; Pres::solve with transforms that do nothing (the Thomas sweep, hdma and its wall rows,
the wave-number-zero row, the Neumann ghost levels and the cyclic fill of p with no FFT in the way); input -> solve -> output with the
oracle's DFT in the reference's FFT seam; calc_divergence; Boundary_cyclic::exec / exec_2d in their TF and unsigned int forms. Each runs
against the reference itself where its tree exists (src = reference) and against tests/golden/pres_ref.npz everywhere (src = golden).
(2) The LIBRARY against the golden file alone, on both backends: the stages bit for bit, the solve within the stated pressure
tolerance (1e-11 fp64 / 2e-4 fp32 of max|p|, tendencies scaled as in test_pres2_lds_transform_form), staged and with the transforms
in LDS; and its deterministic means against Field3d_operators::calc_mean_profile.

Pres_4::input / output are run as Pres_4::exec chooses them (dim3 = jtot > 1): the oracle models that choice only.
Record with  MHH_RECORD_PRES_GOLDEN=1 python -m pytest tests/test_pres_ref.py  where the reference tree exists."""
import ctypes as C

import numpy as np
import pytest

import backends as B
import common as cm
import pres_ref as R
import force_common as FB
import means_common as FM
from backends import be  # noqa: F401
from common import DTYPES, ptr, dbl
from pres_ref import CASES, EXEC_CASES, LIB_CASES, CYCLIC_CASES, MEAN_SHAPES, THERMO_SHAPES, GRAV, DT, tag, case_id

if R.RECORD and not R.have_reference():
    raise RuntimeError("recording tests/golden/pres_ref.npz needs the reference tree")

SRC = [pytest.param("reference", marks=pytest.mark.skipif(not R.have_reference(), reason="reference tree not present on this machine")),
       pytest.param("golden", marks=pytest.mark.skipif(R.RECORD, reason="the golden file is being recorded"))]
case_param = pytest.mark.parametrize("case", CASES, ids=case_id)
EDGES = {"ew": cm.EDGE_EW, "ns": cm.EDGE_NS, "both": cm.EDGE_BOTH}
# measured here (profiles/reference_pins.md): the reference's loop-order double sum and the library's chunked one, in units of
# eps(TF) * sqrt(itot*jtot) * max|field|, largest over MEAN_SHAPES, both fields and every level; the assertion is 8 times that
MEAN_MEASURED = {"f64": 0.1121, "f32": 0}        # fp32: equal bit for bit, asserted as such


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    if R.RECORD:
        R.write_record()


def nbands(order):
    return 2 if order == 2 else 7


# ---- (1) the oracle against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@case_param
def test_oracle_coefficients(case, src, dtype):
    """bmati, bmatj and a, c / m1..m7 of set_values, in TF: the fp32 tables mix double and float (2.*pi*(TF)j/(TF)jtot)."""
    order = case[0]
    g, c = R.inputs(case, dtype)
    got = [np.zeros(g.itot, dtype), np.zeros(g.jtot, dtype), np.zeros((nbands(order), g.kmax), dtype)]
    cm.oracle().orc_pres_coeffs(g.host_struct(), order, ptr(c.rhorefh), *[ptr(a) for a in got])
    key = "coeffs/%s/%s/" % (case_id(case), tag(dtype))
    want = None

    def run_ref(n):
        nonlocal want
        if want is None:
            want = [np.zeros_like(a) for a in got]
            R.shim().ref_pres_set_values(g.host_struct(), order, ptr(c.rhorefh), *[ptr(a) for a in want])
        return want[n]
    for n, name in enumerate(("bmati", "bmatj", "bands")):
        stored = R.expect_values(src, key + name, lambda: run_ref(n))              # the values travel too (tests/test_oracle_pres.py)
        assert cm.same(got[n], stored) and got[n].dtype == stored.dtype, (key + name, cm.ulp_diff(got[n], stored))
    assert got[0][0] == 0 and got[0][1:].max() < 0 and np.abs(got[2]).max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@case_param
def test_oracle_input(case, src, dtype):
    """Pres::input: packed p and the ghost cells it leaves in ut, vt (Edge East_west, North_south) and wt (pres_4's mirror)."""
    order = case[0]
    g, c = R.inputs(case, dtype)
    pk = np.zeros((g.ktot, g.jtot, g.itot), dtype)
    t = [c.ut.copy(), c.vt.copy(), c.wt.copy()]
    cm.oracle().orc_pres_input(g.host_struct(), order, ptr(pk), ptr(c.u), ptr(c.v), ptr(c.w), *[ptr(a) for a in t], ptr(c.rhoref), ptr(c.rhorefh), dbl(DT))
    want = None

    def run_ref(n):
        nonlocal want
        if want is None:
            p = np.zeros(g.ncells, dtype)
            want = [c.ut.copy(), c.vt.copy(), c.wt.copy()]
            R.shim().ref_pres_input(g.host_struct(), order, -1, ptr(p), ptr(c.u), ptr(c.v), ptr(c.w), *[ptr(a) for a in want], ptr(c.rhoref), ptr(c.rhorefh), dbl(DT))
            want.append(p[:pk.size].reshape(pk.shape).copy())
        return want[n]
    key = "input/%s/%s/" % (case_id(case), tag(dtype))
    for n, (name, a) in enumerate(zip(("ut", "vt", "wt", "p"), t + [pk])):
        ok, why = R.expect_bits(src, key + name, a, lambda: run_ref(n))
        assert ok, why
    assert not cm.same(t[0], c.ut) and np.abs(pk).max() > 0


def oracle_solve_identity(case, dtype, packed):
    g, c = R.inputs(case, dtype)
    pk = packed.copy()
    cm.oracle().orc_pres_spectral_solve(g.host_struct(), case[0], ptr(pk), ptr(c.rhoref), ptr(c.rhorefh))
    p = np.zeros(g.shape3, dtype)
    cm.oracle().orc_pres_unpack(g.host_struct(), case[0], ptr(p), ptr(pk))
    return R.masked(p, g, case[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@case_param
def test_oracle_solve_without_transforms(case, src, dtype):
    """Pres::solve on random packed data with transforms that do nothing, against the oracle's spectral solve and unpack: every cell
    of p the reference writes (pres_ref.written)."""
    g, c = R.inputs(case, dtype)
    packed = R.packed_random(g)
    got = oracle_solve_identity(case, dtype, packed)

    def run_ref():
        p = R.field_with_packed(g, packed)
        with R.transforms("identity") as lib:
            lib.ref_pres_solve(g.host_struct(), case[0], ptr(p), ptr(c.rhoref), ptr(c.rhorefh))
        return R.masked(p.reshape(g.shape3), g, case[0])
    ok, why = R.expect_bits(src, "solve_identity/%s/%s/p" % (case_id(case), tag(dtype)), got, run_ref)
    assert ok, why
    it = got[g.interior]
    assert np.isfinite(got).all() and np.abs(it).max() > 0
    assert cm.same(got[g.kstart-1][g.jstart:g.jend], got[g.kstart][g.jstart:g.jend])            # the Neumann ghost level
    assert cm.same(got[g.interior[0], g.jstart:g.jend, :g.igc], got[g.interior[0], g.jstart:g.jend, g.iend-g.igc:g.iend])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@case_param
def test_oracle_exec(case, src, dtype):
    """input -> solve -> output of the reference, its FFT seam filled with the oracle's DFT, against orc_pres_exec: p and the three
    tendencies. The interior of the reference's p (and of its tendencies for the shapes of mhh_pres_exec) goes into the golden file."""
    order = case[0]
    g, c = R.inputs(case, dtype)
    p = np.zeros(g.shape3, dtype); pk = np.zeros((g.ktot, g.jtot, g.itot), dtype)
    t = [c.ut.copy(), c.vt.copy(), c.wt.copy()]
    cm.oracle().orc_pres_exec(g.host_struct(), order, ptr(p), ptr(pk), ptr(c.u), ptr(c.v), ptr(c.w), *[ptr(a) for a in t], ptr(c.rhoref), ptr(c.rhorefh), dbl(DT))
    want = None

    def run_ref(n):
        nonlocal want
        if want is None:
            want = list(R.ref_exec(case, dtype))
            want[0] = R.masked(want[0], g, order)
        return want[n]
    key = "exec/%s/%s/" % (case_id(case), tag(dtype))
    for n, (name, a) in enumerate(zip(("p_written", "ut_all", "vt_all", "wt_all"), [R.masked(p, g, order)] + t)):
        ok, why = R.expect_bits(src, key + name, a, lambda: run_ref(n))
        assert ok, why
    stored = R.expect_values(src, key + "p", lambda: run_ref(0)[g.interior])
    assert cm.same(p[g.interior], stored)
    if case in EXEC_CASES:
        for n, name in enumerate(("ut", "vt", "wt")):
            stored = R.expect_values(src, key + name, lambda: run_ref(n + 1)[g.interior])
            assert cm.same(t[n][g.interior], stored)
    assert not cm.same(t[0][g.interior], c.ut[g.interior]) and (g.ktot == 1 or not cm.same(t[2][g.interior], c.wt[g.interior]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@case_param
def test_oracle_divergence(case, src, dtype):
    g, c = R.inputs(case, dtype)
    got = cm.oracle().orc_pres_divergence(g.host_struct(), case[0], ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))
    ok, why = R.expect_bits(src, "divergence/%s/%s" % (case_id(case), tag(dtype)), np.array([got]),
                            lambda: np.array([R.shim().ref_pres_divergence(g.host_struct(), case[0], ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))]))
    assert ok and got > 0, why


def cyclic_inputs(shape, gc, dtype):
    g = cm.grid_2nd(*shape, gc=gc, dtype=dtype, stretched=False)
    rs = np.random.RandomState(11)
    return g, rs.random_sample(g.shape3).astype(dtype), rs.random_sample(g.shape2).astype(dtype), \
        rs.randint(0, 2**32, size=g.shape3, dtype=np.uint64).astype(np.uint32), rs.randint(0, 2**32, size=g.shape2, dtype=np.uint64).astype(np.uint32)


def cyclic_key(shape, gc, dtype, what):
    return "cyclic/%dx%dx%d-gc%d%d%d/%s/%s" % (shape + gc + (tag(dtype), what))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("shape,gc", CYCLIC_CASES)
def test_oracle_boundary_cyclic(shape, gc, src, dtype):
    """Boundary_cyclic::exec over the three edges, exec_2d, and both in their unsigned int forms; jtot == 1 (its own branch: the one row
    replicated, interior levels only) and one to three ghost cells a side."""
    O = cm.oracle()
    g, a3, a2, u3, u2 = cyclic_inputs(shape, gc, dtype)
    G = g.host_struct()

    def both(key, a, orc, ref):
        got = a.copy(); orc(got)

        def run_ref():
            want = a.copy(); ref(R.shim(), want)
            return want
        ok, why = R.expect_bits(src, cyclic_key(shape, gc, dtype, key), got, run_ref)
        assert ok and not cm.same(got, a), why
    for name, edge in EDGES.items():
        both(name, a3, lambda x: O.orc_boundary_cyclic(G, ptr(x), edge), lambda L, x: L.ref_boundary_cyclic(G, ptr(x), edge))
        both("uint_" + name, u3, lambda x: O.orc_boundary_cyclic_uint(G, ptr(x), edge), lambda L, x: L.ref_boundary_cyclic_uint(G, ptr(x), edge))
    both("2d", a2, lambda x: O.orc_boundary_cyclic_2d(G, ptr(x)), lambda L, x: L.ref_boundary_cyclic_2d(G, ptr(x)))
    both("uint_2d", u2, lambda x: O.orc_boundary_cyclic_2d_uint(G, ptr(x)), lambda L, x: L.ref_boundary_cyclic_2d_uint(G, ptr(x)))


# ---- (2) the library against the golden file ----------------------------------------------------------------------------------------------
lib_case_param = pytest.mark.parametrize("case", LIB_CASES, ids=case_id)


@pytest.mark.parametrize("dtype", DTYPES)
@lib_case_param
def test_library_pres_input_and_output(be, case, dtype):
    """mhh_pres_input: packed p and the tendencies with their ghost cells; mhh_pres_output started from the golden p with every ghost
    cell the reference writes: the three tendencies. Bit for bit against the recorded reference outputs."""
    order = case[0]
    g, c = R.inputs(case, dtype)
    d = B.DevCase(be, c); f = d.fields()
    key_in = "input/%s/%s/" % (case_id(case), tag(dtype))
    key_ex = "exec/%s/%s/" % (case_id(case), tag(dtype))
    with B.pres_plan(be, g, c, order) as plan:
        pk = be.zeros((g.ktot, g.jtot, g.itot), dtype)
        B.ok(be, be.lib.mhh_pres_input(plan, d.G, C.byref(f), DT, be.ptr(pk), be.stream))
        for name, a in (("p", pk), ("ut", d.ut), ("vt", d.vt), ("wt", d.wt)):
            ok, why = R.same_as_golden(key_in + name, be.host(a))
            assert ok, why
        p, _ = R.golden_exec(case, dtype)
        dp = be.arr(p); f2 = d.fields(); f2.p = be.ptr(dp).value
        B.ok(be, be.lib.mhh_pres_output(plan, d.G, C.byref(f2), be.stream))
        for name, a in (("ut_all", d.ut), ("vt_all", d.vt), ("wt_all", d.wt)):
            ok, why = R.same_as_golden(key_ex + name, be.host(a))
            assert ok, why


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["staged", "lds"])
@pytest.mark.parametrize("case", EXEC_CASES, ids=case_id)
def test_library_pres_exec(be, case, form, dtype):
    """mhh_pres_exec, staged and with the transforms in LDS, against the reference's own solve: p on every cell the reference writes
    within 1e-11 (fp64) / 2e-4 (fp32) of max|p|, the tendencies within the same tolerance of max(|t|, max|p| / min(dx, dy))."""
    order = case[0]
    g, c = R.inputs(case, dtype)
    tol = 1e-11 if dtype == np.float64 else 2e-4
    p_want, (ut, vt, wt) = R.golden_exec(case, dtype)
    d = B.DevCase(be, c); f = d.fields()
    with B.pres_plan(be, g, c, order) as plan, cm.switches(MHH_PRES_LDS="1" if form == "lds" else "0"):
        if form == "lds":
            assert be.lib.mhh_pres_plan_has_lds_form(plan) == 1                 # the shapes of EXEC_CASES are those that have it
        assert be.lib.mhh_pres_exec_form(plan) == (1 if form == "lds" else 0)
        B.ok(be, be.lib.mhh_pres_exec(plan, d.G, C.byref(f), DT, be.stream))
    be.sync()
    pscale = float(np.abs(p_want).max())
    err_p = float(np.abs(R.masked(be.host(d.p), g, order).astype(np.float64) - p_want).max()) / pscale
    errs = {}
    for name, got, want in (("ut", d.ut, ut), ("vt", d.vt, vt), ("wt", d.wt, wt)):
        scale = max(float(np.abs(want).max()), pscale/float(min(g.dx, g.dy)))
        errs[name] = float(np.abs(be.host(got)[g.interior].astype(np.float64) - want).max()) / scale
    print("PRESREF %s %s %s %s p %.3e of %.0e tendencies %.3e" % (be.name, form, case_id(case), tag(dtype), err_p, tol, max(errs.values())))
    assert err_p <= tol, (case, form, err_p)
    assert max(errs.values()) <= tol, (case, form, errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,gc", CYCLIC_CASES)
def test_library_boundary_cyclic(be, shape, gc, dtype):
    g, a3, a2, u3, u2 = cyclic_inputs(shape, gc, dtype)
    G = be.grid(g)
    for name, edge in EDGES.items():
        d = be.arr(a3)
        B.ok(be, be.lib.mhh_boundary_cyclic(G, be.ptr(d), edge, be.stream))
        ok, why = R.same_as_golden(cyclic_key(shape, gc, dtype, name), be.host(d))
        assert ok, why
        d = be.arr(u3.view(np.int32))
        B.ok(be, be.lib.mhh_boundary_cyclic_u32(G, be.ptr(d), edge, be.stream))
        ok, why = R.same_as_golden(cyclic_key(shape, gc, dtype, "uint_" + name), be.host(d).view(np.uint32))
        assert ok, why
    d = be.arr(a2)
    B.ok(be, be.lib.mhh_boundary_cyclic_2d(G, be.ptr(d), be.stream))
    ok, why = R.same_as_golden(cyclic_key(shape, gc, dtype, "2d"), be.host(d))
    assert ok, why
    d = be.arr(u2.view(np.int32))
    B.ok(be, be.lib.mhh_boundary_cyclic_2d_u32(G, be.ptr(d), be.stream))
    ok, why = R.same_as_golden(cyclic_key(shape, gc, dtype, "uint_2d"), be.host(d).view(np.uint32))
    assert ok, why


# ---- the means -------------------------------------------------------------------------------------------------------------------------
def mean_fields(shape, dtype):
    """The fields of tests/test_field_means.py: 1e30 in the i and j ghost cells, which neither sum may read."""
    g = FM.grid(shape, dtype)
    return g, FM.fields(g, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("shape", MEAN_SHAPES)
def test_reference_mean_profile_is_within_its_own_summation_bound(shape, src, dtype):
    """Field3d_operators::calc_mean_profile (recorded as values) against math.fsum with the bound of tests/test_field_means.py; and
    subtract_mean_profile and calc_mean_profile_nogc against numpy on the reference's profile (one rounding per cell / per level)."""
    g, host = mean_fields(shape, dtype)
    N = g.itot*g.jtot
    for n in range(2):
        key = "mean/%dx%dx%d/%s/%d" % (shape + (tag(dtype), n))

        def run_ref():
            prof = np.zeros(g.kcells, dtype)
            R.shim().ref_mean_profile(g.host_struct(), ptr(prof), ptr(host[n]))
            return prof
        prof = R.expect_values(src, key, run_ref)
        assert prof.dtype == g.np_dtype
        for k in range(g.kcells):
            ref, bound = FM.profile_bound(host[n][k, g.jstart:g.jend, g.istart:g.iend], N, dtype)
            assert abs(float(prof[k]) - ref) <= bound, (shape, n, k)
        if src == "reference":
            a = host[n].copy()
            R.shim().ref_subtract_mean_profile(g.host_struct(), ptr(a), ptr(prof))
            want = host[n].copy(); want[:, g.jstart:g.jend, g.istart:g.iend] -= prof[:, None, None]
            assert cm.same(a, want)
            nogc = np.ascontiguousarray(host[n][g.kstart:g.kend+1, g.jstart:g.jend, g.istart:g.iend])
            pn = np.zeros(g.ktot+1, dtype)
            R.shim().ref_mean_profile_nogc(g.host_struct(), ptr(pn), ptr(nogc), 1)
            assert cm.same(pn, prof[g.kstart:g.kend+1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MEAN_SHAPES)
def test_library_mean_profile(be, shape, dtype):
    """mhh_field_mean_profile against the recorded Field3d_operators::calc_mean_profile: the library adds the same doubles in another
    order, so the two differ by summation order alone."""
    g, host = mean_fields(shape, dtype)
    G = be.grid(g)
    got = FM.profiles(be, g, G, [be.arr(a) for a in host])
    z = R.golden()
    worst = 0.
    for n in range(2):
        want = z["mean/%dx%dx%d/%s/%d" % (shape + (tag(dtype), n))]
        unit = float(np.finfo(dtype).eps) * np.sqrt(g.itot*g.jtot) * float(np.abs(host[n][:, g.jstart:g.jend, g.istart:g.iend]).max())
        worst = max(worst, float(np.abs(got[n].astype(np.float64) - want.astype(np.float64)).max()) / unit)
        if MEAN_MEASURED[tag(dtype)] == 0:
            assert cm.same(got[n], want), (shape, n)
    print("PRESREF %s mean %dx%dx%d %s reference - library = %.3e units" % ((be.name,) + shape + (tag(dtype), worst)))
    assert worst <= 8*MEAN_MEASURED[tag(dtype)], (shape, worst)


# the same for the volume mean: TF(mhh_field_mean_sum / (itot*jtot*zsize)) against Field3d_operators::calc_mean, in units of
# eps(TF) * (itot*jtot*ktot) * max|fld*dz| / (itot*jtot*zsize), largest over MEAN_SHAPES and both fields; asserted at 8 times that. (n, not
# sqrt(n): the reference adds all n products into one double in loop order, and for a field of one sign the partial sums grow with n.)
VOLUME_MEAN_MEASURED = {"f64": 3.521, "f32": 0}          # fp32: equal bit for bit, asserted as such


def volume_mean_fields(shape, dtype):
    g = cm.grid_2nd(*shape, gc=(2, 2, 1), dtype=dtype, z=R.zprofile(shape[2], 1200.))
    return g, FM.fields(g, 2)


def volume_mean_key(shape, dtype):
    return "calc_mean/%dx%dx%d/%s" % (shape + (tag(dtype),))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("shape", MEAN_SHAPES)
def test_reference_calc_mean_is_within_its_own_summation_bound(shape, src, dtype):
    """Field3d_operators::calc_mean (recorded as values) against math.fsum of fl(fld*dz) with the bound of tests/test_field_means.py."""
    import math
    g, host = volume_mean_fields(shape, dtype)
    got = R.expect_values(src, volume_mean_key(shape, dtype), lambda: np.array([R.shim().ref_calc_mean(g.host_struct(), ptr(a)) for a in host], dtype=dtype))
    den = float(g.itot * g.jtot) * g.zsize
    for n in range(2):
        x = host[n][g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend] * g.dz[g.kstart:g.kend, None, None]
        xs = [float(v) for v in x.ravel()]
        ref = math.fsum(xs) / den
        bound = FM.gamma(len(xs)) * math.fsum(abs(v) for v in xs) / den + 2*FM.ulp(ref, dtype)
        assert abs(float(got[n]) - ref) <= bound, (shape, n, float(got[n]), ref, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MEAN_SHAPES)
def test_library_mean_sum(be, shape, dtype):
    """mhh_field_mean_sum, divided and narrowed as Force does it, against the recorded Field3d_operators::calc_mean."""
    g, host = volume_mean_fields(shape, dtype)
    G = be.grid(g)
    T = g.np_dtype.type
    S = FM.sums(be, g, G, [be.arr(a) for a in host])
    den = np.float64(T(g.itot * g.jtot) * T(g.zsize))
    want = R.golden()[volume_mean_key(shape, dtype)]
    worst = 0.
    for n in range(2):
        got = T(np.float64(S[n]) / den)
        x = host[n][g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend] * g.dz[g.kstart:g.kend, None, None]
        unit = float(np.finfo(dtype).eps) * (g.itot*g.jtot*g.ktot) * float(np.abs(x).max()) / float(den)
        worst = max(worst, abs(float(got) - float(want[n])) / unit)
        if VOLUME_MEAN_MEASURED[tag(dtype)] == 0:
            assert got == want[n], (shape, n)
    print("PRESREF %s volume mean %dx%dx%d %s reference - library = %.3e units" % ((be.name,) + shape + (tag(dtype), worst)))
    assert worst <= 8*VOLUME_MEAN_MEASURED[tag(dtype)], (shape, worst)


# ---- Thermo_dry's buoyancy kernels and the evisc kernels of Diff_smag2 --------------------------------------------------------------------
def thermo_inputs(shape, order, dtype):
    g = cm.grid_2nd(*shape, gc=(2, 2, 2), dtype=dtype, z=R.zprofile(shape[2], 1200.)) if order == 2 else \
        cm.grid_4th(*shape, dtype=dtype, z=R.zprofile(shape[2], 2.))
    c = cm.Case(g, seed=668)
    th = (dtype(300.) + c.s[0]).astype(dtype)
    thref = (300. + 0.41*np.arange(g.kcells)).astype(dtype)
    threfh = (300. + 0.37*np.arange(g.kcells)).astype(dtype)
    return g, c, th, thref, threfh


def thermo_key(shape, order, dtype, what):
    return "thermo_dry/%dx%dx%d/o%d/%s/%s" % (shape + (order, tag(dtype), what))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", THERMO_SHAPES)
def test_oracle_dry_buoyancy(shape, order, src, dtype):
    """calc_buoyancy_tend_2nd / _4th and calc_N2 against the oracle; calc_buoyancy_bot and calc_buoyancy_fluxbot, which the oracle
    does not have, against the same expression in numpy (one division, one product: the same roundings)."""
    O = cm.oracle()
    g, c, th, thref, threfh = thermo_inputs(shape, order, dtype)
    G = g.host_struct()
    if src == "reference":
        assert R.shim().ref_thermo_dry_grav() == GRAV
    wt = c.wt.copy(); O.orc_buoyancy_tend(G, order, ptr(wt), ptr(th), ptr(threfh), dbl(GRAV))

    def ref_tend():
        want = c.wt.copy(); R.shim().ref_buoyancy_tend(G, order, ptr(want), ptr(th), ptr(threfh))
        return want
    ok, why = R.expect_bits(src, thermo_key(shape, order, dtype, "wt"), wt, ref_tend)
    assert ok and not cm.same(wt, c.wt), why
    n2 = np.zeros(g.shape3, dtype); O.orc_calc_N2(G, ptr(n2), ptr(th), ptr(thref), dbl(GRAV))

    def ref_n2():
        want = np.zeros(g.shape3, dtype); R.shim().ref_calc_N2(G, ptr(want), ptr(th), ptr(thref))
        return want
    ok, why = R.expect_bits(src, thermo_key(shape, order, dtype, "N2"), n2, ref_n2)
    assert ok and np.abs(n2).max() > 0, why
    if src == "reference":
        T = dtype
        b = np.zeros(g.shape3, dtype); bbot = np.zeros(g.shape2, dtype); bflux = np.zeros(g.shape2, dtype)
        R.shim().ref_buoyancy_bot(G, ptr(b), ptr(bbot), ptr(th), ptr(c.dudz), ptr(thref), ptr(threfh))
        R.shim().ref_buoyancy_fluxbot(G, ptr(bflux), ptr(c.dvdz), ptr(threfh))
        ks = g.kstart
        assert cm.same(bbot, T(GRAV)/threfh[ks] * (c.dudz - threfh[ks])) and cm.same(bflux, T(GRAV)/threfh[ks] * c.dvdz)
        assert cm.same(b[ks], T(GRAV)/thref[ks] * (th[ks] - thref[ks])) and not b[ks+1:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("shape", THERMO_SHAPES)
def test_library_dry_buoyancy(be, shape, order, dtype):
    """mhh_thermo_dry_buoyancy_tend and mhh_calc_N2 against the recorded outputs of the reference's kernels, bit for bit."""
    g, c, th, thref, threfh = thermo_inputs(shape, order, dtype)
    G = be.grid(g)
    dth = be.arr(th)
    t = be.arr(c.wt); dh = be.arr(threfh)
    B.ok(be, be.lib.mhh_thermo_dry_buoyancy_tend(G, order, be.ptr(t), be.ptr(dth), be.ptr(dh), GRAV, be.stream))
    ok, why = R.same_as_golden(thermo_key(shape, order, dtype, "wt"), be.host(t))
    assert ok, why
    n2 = be.zeros(g.shape3, dtype); dr = be.arr(thref)
    B.ok(be, be.lib.mhh_calc_N2(G, be.ptr(n2), be.ptr(dth), be.ptr(dr), dtype(GRAV), be.stream))
    ok, why = R.same_as_golden(thermo_key(shape, order, dtype, "N2"), be.host(n2))
    assert ok, why


EVISC_ULP = {(1, 0): 8, (0, 0): 8, (1, 1): 8, (0, 1): 64}          # sqrt and the Mason length; van Driest (pow 1/4, exp)


@pytest.mark.skipif(not R.have_reference(), reason="reference tree not present on this machine")
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sm,neutral", sorted(EVISC_ULP))
def test_oracle_evisc(sm, neutral, dtype):
    """calc_evisc / calc_evisc_neutral (their Boundary_cyclic tail included) against the oracle, at the ulp bounds of DESIGN.md section 3.
    Both sides call this host's libm, so the recorded bits would not travel: this comparison runs only where the reference tree is."""
    O = cm.oracle()
    worst = 0.
    for g in (cm.grid_2nd(16, 12, 10, gc=(3, 3, 1), dtype=dtype), cm.grid_2nd(70, 9, 8, gc=(3, 3, 2), dtype=dtype), cm.grid_2nd(12, 1, 8, gc=(3, 3, 1), dtype=dtype)):
        c = cm.Case(g, periodic=True); G = g.host_struct()
        cs, tPr, visc = 0.23, 1./3., 1e-5
        s2 = np.zeros(g.shape3, dtype)
        O.orc_smag2_strain2(G, sm, ptr(s2), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.dudz), ptr(c.dvdz))
        got, want = s2.copy(), s2.copy()
        if neutral:
            O.orc_smag2_evisc_neutral(G, sm, ptr(got), ptr(c.u), ptr(c.v), ptr(c.z0m), dbl(cs), dbl(visc))
            R.shim().ref_smag2_evisc_neutral(G, sm, ptr(want), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.u_fluxbot), ptr(c.v_fluxbot), ptr(c.z0m), dbl(cs), dbl(visc))
        else:
            O.orc_smag2_evisc(G, sm, ptr(got), ptr(c.N2), ptr(c.dbdz), ptr(c.z0m), dbl(cs), dbl(tPr))
            R.shim().ref_smag2_evisc(G, sm, ptr(want), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.N2), ptr(c.dbdz), ptr(c.z0m), dbl(cs), dbl(tPr))
        k0, k1 = (g.kstart, g.kend) if sm else (g.kstart-1, g.kend+1)
        jj = slice(None) if g.jtot > 1 else slice(g.jstart, g.jend)
        assert np.isfinite(want[k0:k1, jj]).all() and want[g.interior].min() >= 0 and want[g.interior].max() > 0
        worst = max(worst, cm.ulp_diff(got[k0:k1, jj], want[k0:k1, jj]))
    print("PRESREF evisc sm %d neutral %d %s oracle - reference = %g ulp" % (sm, neutral, tag(dtype), worst))
    assert worst <= EVISC_ULP[(sm, neutral)], worst


# ---- Force and Buffer ------------------------------------------------------------------------------------------------------------------
needs_reference = pytest.mark.skipif(not R.have_reference(), reason="reference tree not present on this machine")
MEAN_NAMES = ("u", "v", "s0", "s1")                                 # the fields whose mean profile Force reads


def force_grid(shape, order, dtype):
    """The grids of tests/test_force_buffer.py on the stored z profiles."""
    if order == 2:
        return cm.grid_2nd(*shape, gc=(1, 1, 1), dtype=dtype, z=R.zprofile(shape[2], 1200.))
    return cm.grid_4th(*shape, dtype=dtype, igc=2, jgc=2, kgc=3, z=R.zprofile(shape[2], 2.))


def force_key(shape, term, order, dtype, name):
    return "force/%dx%dx%d/%s/o%d/%s/%s" % (shape + (term, order, tag(dtype), name))


def sum_for_mean(g, mean):
    """The double that mhh_force_params::uflux_sums has to hold for the library to arrive at the reference's mean. Force::exec reads
    u_mean = calc_mean(u), a TF; the library reads the global sum of u*dz and forms TF(sum / (itot*jtot*zsize)) itself. The sum is an
    input of mhh_force_exec: this picks the double nearest mean*den whose quotient narrows to `mean` exactly, so that what the library
    computes from its input and what the reference's calc_mean returned are one number, and the tendencies can be held bit for bit."""
    T = g.np_dtype.type
    den = np.float64(T(g.itot * g.jtot) * T(g.zsize))
    s = np.float64(mean) * den
    up, down = np.nextafter(s, np.inf), np.nextafter(s, -np.inf)
    for cand in (s, up, down, np.nextafter(up, np.inf), np.nextafter(down, -np.inf)):
        if T(cand / den) == T(mean):
            return float(cand)
    raise AssertionError("no double within two ulp of mean*den gives the mean back")


def force_inputs(src, shape, order, dtype):
    """(grid, Case, mean profiles {name: TF[kcells]}, (u_mean, ut_mean)) of a shape: the reference's own calc_mean_profile and calc_mean
    of the seeded fields (src 'reference', recorded when asked) or their recorded values (src 'golden')."""
    g = force_grid(shape, order, dtype)
    c = cm.Case(g, nscalars=2, periodic=True)
    key = "force_in/%dx%dx%d/o%d/%s/" % (shape + (order, tag(dtype)))

    def profile(n):
        prof = np.zeros(g.kcells, dtype)
        R.shim().ref_mean_profile(g.host_struct(), ptr(prof), ptr(FB.field(c, n)))
        return prof
    means = {n: R.expect_values(src, key + "mean_" + n, lambda: profile(n)) for n in MEAN_NAMES}
    vol = R.expect_values(src, key + "calc_mean", lambda: np.array([R.shim().ref_calc_mean(g.host_struct(), ptr(a)) for a in (c.u, c.ut)], dtype=dtype))
    return g, c, means, (dtype(vol[0]), dtype(vol[1]))


def reference_force(g, c, P, means, vol):
    """The kernels of force.cxx in the order of Force::exec (src/force.cxx:581-729). means: calc_mean_profile of each field (fld_mean);
    vol: calc_mean of u and of ut, as exec obtains them before enforce_fixed_flux."""
    L = R.shim(); G = g.host_struct()
    tend = FB.host_tend(c)
    lp = P.get("swlspres")
    if lp == "dpdx":
        L.ref_force_dpdx(G, ptr(tend["u"]), dbl(P["dpdx"]))
    elif lp == "uflux":
        L.ref_force_fixed_flux(G, ptr(tend["u"]), dbl(P["uflux"]), dbl(vol[0]), dbl(vol[1]), dbl(P["utrans"]), dbl(P["dt"]))
    elif lp == "geo":
        L.ref_force_coriolis(G, P["order"], ptr(tend["u"]), ptr(tend["v"]), ptr(c.u), ptr(c.v), ptr(P["ug"]), ptr(P["vg"]), dbl(P["fc"]),
                             dbl(P["utrans"]), dbl(P["vtrans"]))
    for n, ls in P.get("ls", {}).items():
        L.ref_force_large_scale_source(G, ptr(tend[n]), ptr(ls))
    scalars = [n for n in FB.NAMES if n[0] == "s"]
    if P.get("swwls") == "mean":
        for n in (["u", "v"] if P.get("mom") else []) + scalars:
            L.ref_force_wls(G, 0, ptr(tend[n]), ptr(means[n]), ptr(P["wls"]))
    elif P.get("swwls") == "local":
        for n in (["u", "v"] if P.get("mom") else []) + scalars:
            L.ref_force_wls(G, 1, ptr(tend[n]), ptr(FB.field(c, n)), ptr(P["wls"]))
        if P.get("mom"):
            L.ref_force_wls(G, 2, ptr(tend["w"]), ptr(c.w), ptr(P["wls"]))
    for n, ref in P.get("nudge", {}).items():
        L.ref_force_nudging(G, ptr(tend[n]), ptr(means[n]), ptr(ref), ptr(P["nfac"]))
    return tend


def library_force(be, g, c, P, means, vol):
    """mhh_force_exec with the reference's mean profiles and (through sum_for_mean) volume means as its pointer inputs."""
    dv = FB.Dev(be, g, c, P=P, means=means, sums=[sum_for_mean(g, vol[0]), sum_for_mean(g, vol[1])])
    B.ok(be, dv.force())
    return dv.tendencies()


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("term,order", FB.TERM_ORDERS)
def test_library_force_against_the_reference_kernels(term, order, dtype):
    """mhh_force_exec on the emulation backend against add_pressure_force, enforce_fixed_flux, calc_coriolis_2nd / _4th,
    calc_large_scale_source, advec_wls_2nd_mean / _local / _local_w and calc_nudging_tendency of the reference, bit for bit, every term
    of tests/test_force_buffer.py on its shapes. The means come from the reference's own calc_mean_profile and calc_mean on both sides;
    the reference's outputs are recorded for the device."""
    be = B.get("emul")
    for shape in FB.SHAPES:
        g, c, means, vol = force_inputs("reference", shape, order, dtype)
        P = FB.force_setup(g, term, order)
        want = reference_force(g, c, P, means, vol)
        got = library_force(be, g, c, P, means, vol)
        FB.assert_same(got, want, (shape, term, order))
        assert any(not cm.same(want[n], FB.field(c, n, tend=True)) for n in FB.NAMES)
        if R.RECORD:
            for n in FB.NAMES:
                R.REC["digests"][force_key(shape, term, order, dtype, n)] = R.digest(want[n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("term,order", FB.TERM_ORDERS)
def test_library_force_against_the_golden_file(be, term, order, dtype):
    """Every term on both backends against the recorded outputs of the reference's kernels, bit for bit; the mean profiles and the
    volume means that enter are the recorded ones of the reference."""
    for shape in FB.SHAPES:
        g, c, means, vol = force_inputs("golden", shape, order, dtype)
        got = library_force(be, g, c, FB.force_setup(g, term, order), means, vol)
        for n in FB.NAMES:
            ok, why = R.same_as_golden(force_key(shape, term, order, dtype, n), got[n])
            assert ok, (why, shape, term, order, n)


BUFFER_SIGMA, BUFFER_BETA = 2., 2.3                                 # tests/force_common.py::buffer_setup


def buffer_zstart(g):
    k = g.kstart + (2 * g.kmax) // 3
    return 0.5 * (float(g.zh[k]) + float(g.z[k]))


def reference_buffer(g, c, Bf):
    """calc_buffer with the argument lists of Buffer::exec (src/buffer.cxx:163-206): zh and bufferkstarth for w."""
    L = R.shim(); G = g.host_struct()
    tend = FB.host_tend(c)
    for n in FB.NAMES:
        half = int(n == "w")
        L.ref_buffer(G, half, ptr(tend[n]), ptr(FB.field(c, n)), ptr(Bf["abuf"][n]), dbl(buffer_zstart(g)), dbl(BUFFER_BETA), dbl(BUFFER_SIGMA),
                     Bf["ksh"] if half else Bf["ks"])
    return tend


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("swupdate", [False, True], ids=["fixed", "swupdate"])
def test_library_buffer_against_the_reference_kernel(swupdate, dtype):
    """mhh_buffer_exec on the emulation backend against calc_buffer, which raises its own powers: bit for bit (the sponge table of the
    library comes from this host's pow as well)."""
    be = B.get("emul")
    for shape in FB.SHAPES:
        g = force_grid(shape, 2, dtype)
        c = cm.Case(g, nscalars=2)
        Bf = FB.buffer_setup(be, g, swupdate)
        dv = FB.Dev(be, g, c, Bf=Bf)
        B.ok(be, dv.buffer())
        got = dv.tendencies()
        want = reference_buffer(g, c, Bf)
        FB.assert_same(got, want, (shape, "buffer", swupdate))
        assert not cm.same(want["w"], c.wt)
        if R.RECORD and not swupdate:
            key = "buffer/%dx%dx%d/%s/" % (shape + (tag(dtype),))
            R.REC["arrays"][key + "sigma"], R.REC["arrays"][key + "sigmah"] = Bf["sigma"], Bf["sigmah"]
            for n in FB.NAMES:
                R.REC["digests"][key + n] = R.digest(want[n])


@pytest.mark.parametrize("dtype", DTYPES)
def test_library_buffer_against_the_golden_file(be, dtype):
    """The sponge tables are the recorded ones (pow's last bits follow the host), everything else is seeded."""
    for shape in FB.SHAPES:
        g = force_grid(shape, 2, dtype)
        c = cm.Case(g, nscalars=2)
        key = "buffer/%dx%dx%d/%s/" % (shape + (tag(dtype),))
        Bf = FB.buffer_setup(be, g, False)
        Bf["sigma"], Bf["sigmah"] = R.golden()[key + "sigma"], R.golden()[key + "sigmah"]
        dv = FB.Dev(be, g, c, Bf=Bf)
        B.ok(be, dv.buffer())
        got = dv.tendencies()
        for n in FB.NAMES:
            ok, why = R.same_as_golden(key + n, got[n])
            assert ok, why


# ---- the pressure solve of the slab code path on one rank ------------------------------------------------------------------------------
SLAB_SHAPE = (16, 12, 10)                                           # tests/test_parity.py::test_slab_code_path_on_one_rank


def slab_hotpaths(be, dtype, forms):
    from microhh_amd.model import HotPath, synthetic_global
    gi = synthetic_global("drycblles", *SLAB_SHAPE, dtype=dtype)
    dev = "cuda:0" if be.name == "hip" else "cpu"
    return gi, [HotPath("drycblles", *SLAB_SHAPE, dtype=dtype, device=dev, lib=be.lib, global_init=gi, force_slab=slab) for slab in forms]


def slab_host_inputs(g, gi):
    """What HotPath holds before its pressure solve, rebuilt on the host: the interior of synthetic_global, w and wt zero at and
    outside the walls, the cyclic fill of u, v, w (HotPath.cyclic_prognostic)."""
    a = {}
    for n in ("u", "v", "w", "ut", "vt", "wt"):
        a[n] = np.zeros(g.shape3, g.np_dtype); a[n][g.interior] = gi[n]
    for n in ("w", "wt"):
        a[n][:g.kstart+1] = 0; a[n][g.kend:] = 0
    for n in ("u", "v", "w"):
        cm.oracle().orc_boundary_cyclic(g.host_struct(), ptr(a[n]), cm.EDGE_BOTH)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src", SRC)
def test_oracle_exec_on_the_slab_case(src, dtype):
    """The reference's input -> solve -> output on the fields of the one-rank slab test (uniform grid, rhoref = 1), recorded as values."""
    gi, (hp,) = slab_hotpaths(B.get("emul"), dtype, [False])
    g, dt = hp.grid, hp.dt
    hp.close()
    a = slab_host_inputs(g, gi)
    ones = np.ones(g.kcells, dtype)
    p = np.zeros(g.shape3, dtype); pk = np.zeros((g.ktot, g.jtot, g.itot), dtype)
    t = [a["ut"].copy(), a["vt"].copy(), a["wt"].copy()]
    cm.oracle().orc_pres_exec(g.host_struct(), 2, ptr(p), ptr(pk), ptr(a["u"]), ptr(a["v"]), ptr(a["w"]), *[ptr(x) for x in t], ptr(ones), ptr(ones), dbl(dt))
    want = None

    def run_ref(n):
        nonlocal want
        if want is None:
            rp = np.zeros(g.ncells, dtype)
            want = [None, a["ut"].copy(), a["vt"].copy(), a["wt"].copy()]
            with R.transforms("oracle") as L:
                L.ref_pres_exec(g.host_struct(), 2, ptr(rp), ptr(a["u"]), ptr(a["v"]), ptr(a["w"]), *[ptr(x) for x in want[1:]], ptr(ones), ptr(ones), dbl(dt))
            want[0] = rp.reshape(g.shape3)
        return want[n][g.interior]
    for n, (name, got) in enumerate(zip(("p", "ut", "vt", "wt"), [p] + t)):
        stored = R.expect_values(src, "slab/%s/%s" % (tag(dtype), name), lambda: run_ref(n))
        assert cm.same(got[g.interior], stored), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_library_slab_pressure(be, dtype):
    """Pressure through mhh_pres_exec and through the slab path on one rank (mhh_pres_slab_*, the exchanges local copies) against the
    recorded reference solve: interior of p and of the tendencies within the stated pressure tolerance. The case is a uniform grid
    with rhoref = 1, where the two off-diagonals of the solve are equal: it holds the call sequence of the slab path, not the tables of
    its plan. Stretched grids, density profiles and more than one rank: tests/test_slab_vranks.py."""
    tol = 1e-11 if dtype == np.float64 else 2e-4
    gi, hps = slab_hotpaths(be, dtype, [False, True])
    z = R.golden()
    for form, hp in zip(("exec", "slab"), hps):
        g = hp.grid
        hp.cyclic_prognostic(); hp.pres(); hp.sync()
        want = {n: z["slab/%s/%s" % (tag(dtype), n)] for n in ("p", "ut", "vt", "wt")}
        pscale = float(np.abs(want["p"]).max())
        errs = {}
        for n in ("p", "ut", "vt", "wt"):
            scale = pscale if n == "p" else max(float(np.abs(want[n]).max()), pscale/float(min(g.dx, g.dy)))
            errs[n] = float(np.abs(be.host(getattr(hp, n))[g.interior].astype(np.float64) - want[n]).max()) / scale
        print("PRESREF %s %s 16x12x10 %s p %.3e of %.0e tendencies %.3e" % (be.name, form, tag(dtype), errs["p"], tol, max(errs["ut"], errs["vt"], errs["wt"])))
        assert max(errs.values()) <= tol, (form, errs)
        hp.close()
