"""Thermo_buoy (swthermo=buoy, src/thermo_buoy.cxx) on the device: the stand-alone kernels mhh_thermo_buoy_tend and
mhh_thermo_buoy_N2, the N2 of b evaluated inside exec_viscosity (buoyancy_kind = 1), and the flat buoyancy folded into the
fused RHS passes.

There is no oracle function for Thermo_buoy, so the reference is a numpy restatement of the cited lines in their expression
order (numpy does not contract; the library builds with -ffp-contract=off): bit for bit. sin(alpha) and cos(alpha) come from
the C library in the grid's dtype, as std::sin / std::cos of a TF do in the reference.

Runs on the ``emul`` backend (the same kernel sources on the CPU) and on the ``hip`` backend (marked gpu)."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import backends as B
import common as cm
from backends import be  # noqa: F401
from common import DTYPES, same_bits as same
from microhh_amd import capi

SHAPES = [(70, 9, 10), (17, 9, 8), (20, 1, 12)]          # ragged 3-D sizes and jtot = 1
# (alpha, N2, utrans): flat form, stratified (N2 != 0, alpha = 0), sloped (the prandtlslope set-up)
FORMS = {"flat": (0., 0., 0.), "stratified": (0., 0.7, 0.), "sloped": (0.5235, 1., 0.13)}

_libm = C.CDLL(ctypes.util.find_library("m"))
for _n, _t in (("sin", C.c_double), ("cos", C.c_double), ("sinf", C.c_float), ("cosf", C.c_float)):
    getattr(_libm, _n).restype = _t
    getattr(_libm, _n).argtypes = [_t]


def sincos(alpha, T):
    if T == np.float32:
        a = float(np.float32(alpha))
        return np.float32(_libm.sinf(a)), np.float32(_libm.cosf(a))
    return np.float64(_libm.sin(alpha)), np.float64(_libm.cos(alpha))


def grid(shape, order, dtype, gc=None):
    if order == 2:
        return cm.grid_2nd(*shape, gc=gc or (1, 1, 1), dtype=dtype)
    gc = gc or (2, 2, 3)                                       # igc = 2: the x stencil of the slope form; kgc = 3: Grid's 4th-order metrics
    return cm.grid_4th(*shape, dtype=dtype, igc=gc[0], jgc=gc[1], kgc=gc[2])


# ---- the numpy restatement of src/thermo_buoy.cxx ----------------------------------------------------------------------
def _i2(T, a, b):
    return T(0.5) * (a + b)                                    # interp2, include/finite_difference.h:37-40


def _i4c(T, a, b, c, d):
    return T(-1./16.) * (a + d) + T(9./16.) * (b + c)          # interp4c = ci0*(a+d) + ci1*(b+c), :93-96


def ref_tend(g, order, c, n, alpha, n2, utrans):
    """Thermo_buoy::exec (:347-395): returns (ut, wt, bt)."""
    T = g.np_dtype.type
    ut, wt, bt = c.ut.copy(), c.wt.copy(), c.st[n].copy()
    b, u, w = c.s[n], c.u, c.w
    J, I = slice(g.jstart, g.jend), slice(g.istart, g.iend)

    def at(a, k0, k1, dk=0, di=0):
        return a[k0+dk:k1+dk, J, g.istart+di:g.iend+di]

    def interp(a, k0, k1, axis, off):                        # the face between cells off-1 and off along axis ("k" or "i")
        sh = (lambda d: at(a, k0, k1, dk=off+d)) if axis == "k" else (lambda d: at(a, k0, k1, di=off+d))
        return _i4c(T, sh(-2), sh(-1), sh(0), sh(1)) if order == 4 else _i2(T, sh(-1), sh(0))
    ks, ke = g.kstart, g.kend
    if alpha == 0. and n2 == 0.:
        wt[ks+1:ke, J, I] += interp(b, ks+1, ke, "k", 0)                                           # calc_buoyancy_tend_2nd/_4th
        return ut, wt, bt
    sa, ca = sincos(alpha, T)
    ut[ks:ke, J, I] += sa * interp(b, ks, ke, "i", 0)                                              # calc_buoyancy_tend_u_*
    wt[ks+1:ke, J, I] += ca * interp(b, ks+1, ke, "k", 0)                                          # calc_buoyancy_tend_w_*
    bt[ks:ke, J, I] -= T(n2) * (sa * (interp(u, ks, ke, "i", 1) + T(utrans)) + ca * interp(w, ks, ke, "k", 1))   # _b_*
    return ut, wt, bt


def ref_N2(g, b, bg_n2):
    """calc_N2 (:49-61): interior only, everything else as it was."""
    T = g.np_dtype.type
    out = np.zeros(g.shape3, dtype=g.np_dtype)
    ks, ke = g.kstart, g.kend
    dzi = g.dzi[ks:ke, None, None]
    J, I = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    out[ks:ke, J, I] = T(0.5) * (b[ks+1:ke+1, J, I] - b[ks-1:ke-1, J, I]) * dzi + T(bg_n2)
    return out


def case(g, nscalars=2, periodic=False):
    c = cm.Case(g, nscalars=nscalars, periodic=periodic)
    T = g.np_dtype.type
    for n in range(nscalars):                 # a stratified b with a bit of noise (positive and negative N2 both occur)
        c.s[n] = (T(0.003) * np.arange(g.kcells, dtype=g.np_dtype)[:, None, None] + T(0.01) * c.s[n]).astype(g.np_dtype)
    if periodic:
        for a in c.s:
            cm.oracle().orc_boundary_cyclic(g.host_struct(), cm.ptr(a), cm.EDGE_BOTH)
    return c


def tend(be, d, order, n, alpha, n2, utrans):
    f = d.fields()
    B.ok(be, be.lib.mhh_thermo_buoy_tend(d.G, order, C.byref(f), n, alpha, n2, utrans, be.stream))


# ---- stand-alone kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("form", list(FORMS))
def test_buoyancy_tendency_standalone_bitexact(be, dtype, order, form):
    alpha, n2, utrans = FORMS[form]
    for shape in SHAPES:
        g = grid(shape, order, dtype)
        c = case(g)
        for n in (0, 1):
            want = ref_tend(g, order, c, n, alpha, n2, utrans)
            d = B.DevCase(be, c)
            tend(be, d, order, n, alpha, n2, utrans)
            got = (be.host(d.ut), be.host(d.wt), be.host(d.st[n]))
            for a, b, nm in zip(got, want, ("ut", "wt", "bt")):
                assert same(a, b), (form, order, shape, n, nm, cm.ulp_diff(a, b))
            assert same(be.host(d.st[1-n]), c.st[1-n])        # the other scalar's tendency is left alone
            assert not same(want[1], c.wt)
            if form == "flat":
                assert same(got[0], c.ut) and same(got[2], c.st[n])
            else:                                              # sin(0) = 0: ut keeps its bits in the stratified form
                assert same(want[0], c.ut) == (alpha == 0.) and not same(want[2], c.st[n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bg_n2", [0., 0.7])
def test_N2_standalone_bitexact(be, dtype, bg_n2):
    for shape in SHAPES:
        g = grid(shape, 2, dtype)
        c = case(g)
        d = B.DevCase(be, c)
        out = be.zeros(g.shape3, dtype)
        B.ok(be, be.lib.mhh_thermo_buoy_N2(d.G, be.ptr(out), be.ptr(d.s[1]), bg_n2, be.stream))
        want = ref_N2(g, c.s[1], bg_n2)
        assert same(be.host(out), want), (shape, cm.ulp_diff(be.host(out), want))


def test_refusals(be):
    g = grid((17, 9, 8), 2, np.float64)
    d = B.DevCase(be, case(g))
    f = d.fields()

    def refused(rc, words):
        msg = be.lib.mhh_last_error().decode()
        assert rc == 1, rc                                      # MHH_EINVAL
        assert words in msg, msg
    refused(be.lib.mhh_thermo_buoy_tend(d.G, 2, C.byref(f), 2, 0., 0., 0., be.stream), "b_index")
    refused(be.lib.mhh_thermo_buoy_tend(d.G, 2, C.byref(f), -1, 0., 0., 0., be.stream), "b_index")
    refused(be.lib.mhh_thermo_buoy_tend(d.G, 3, C.byref(f), 0, 0., 0., 0., be.stream), "order")
    refused(be.lib.mhh_thermo_buoy_tend(d.G, 4, C.byref(f), 0, 0., 0., 0., be.stream), "kgc")      # kgc = 1
    g4 = grid((17, 9, 8), 4, np.float64, gc=(1, 2, 3))
    d4 = B.DevCase(be, case(g4)); f4 = d4.fields()
    B.ok(be, be.lib.mhh_thermo_buoy_tend(d4.G, 4, C.byref(f4), 0, 0., 0., 0., be.stream))          # flat: no x stencil
    refused(be.lib.mhh_thermo_buoy_tend(d4.G, 4, C.byref(f4), 0, 0.5235, 1., 0., be.stream), "igc")
    # buoyancy_kind is 0 or 1; the row-wise pass folds the flat form only
    g2 = cm.grid_2nd(16, 12, 10, gc=(3, 3, 1))
    d2 = B.DevCase(be, case(g2)); f2 = d2.fields()
    p = cm.diff_params(1, mlen0=be.ptr(B.mlen0(be, g2, 0.23)).value)
    p.buoyancy = 2; p.buoyancy_kind = 2; p.th_for_N2 = 0
    refused(be.lib.mhh_rhs_exec(d2.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f2), C.byref(p), be.stream), "buoyancy_kind")
    p.buoyancy_kind = 1; p.alpha = 0.5235
    refused(be.lib.mhh_rhs_exec_rows(d2.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f2), C.byref(p), g2.jstart, g2.jend, be.stream), "flat form")
    p.buoyancy_kind = 3
    refused(be.lib.mhh_diff_exec_viscosity(d2.G, cm.DIFF_SMAG2, C.byref(f2), C.byref(p), be.stream), "buoyancy_kind")


# ---- N2 of b inside exec_viscosity ---------------------------------------------------------------------------------------
def _visc_params(be, g, sm, keep):
    p = cm.diff_params(sm, neutral=0)
    ml = B.mlen0(be, g, 0.23); keep.append(ml); p.mlen0 = be.ptr(ml).value
    return p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sm", [1, 0])
@pytest.mark.parametrize("route", ["march", "cell", "rows"])
def test_exec_viscosity_inline_N2_of_b_equals_N2_through_a_pointer(be, dtype, sm, route):
    """buoyancy_kind = 1: N2 = calc_N2(b) evaluated inside exec_viscosity gives the bits of get_thermo_field("N2") into a 3-D
    field read through mhh_diff_params::N2 -- in the marching form, the cell form and the row forms with the locally evaluated
    ghost rows (evisc_ghost_rows) of the overlapped slab sub-step."""
    shapes = [(70, 10, 12), (17, 9, 8), (20, 1, 12)] if route != "rows" else [(70, 14, 12), (17, 13, 8)]
    for shape in shapes:
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype)
        c = case(g, nscalars=2, periodic=True)
        out = {}
        for how in ("inline", "pointer"):
            keep = []
            d = B.DevCase(be, c); f = d.fields()
            p = _visc_params(be, g, sm, keep)
            p.buoyancy_kind = 1; p.bg_n2 = 0.7; p.th_for_N2 = 1
            if how == "pointer":
                n2 = be.zeros(g.shape3, dtype); keep.append(n2)
                B.ok(be, be.lib.mhh_thermo_buoy_N2(d.G, be.ptr(n2), be.ptr(d.s[1]), p.bg_n2, be.stream))
                B.ok(be, be.lib.mhh_boundary_cyclic(d.G, be.ptr(n2), cm.EDGE_BOTH, be.stream))   # the ghost rows of the row forms
                p.N2 = be.ptr(n2).value; p.th_for_N2 = -1
            with cm.switches(MHH_VISC_IMPL="cell" if route == "cell" else "march"):
                if route == "rows":
                    p.evisc_ghost_rows = 1
                    B.ok(be, be.lib.mhh_diff_exec_viscosity_rows(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), g.jstart + 1, g.jend - 1, be.stream))
                    B.ok(be, be.lib.mhh_diff_exec_viscosity_rows2(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), g.jstart - 1, g.jstart + 1,
                                                                  g.jend - 1, g.jend + 1, be.stream))
                else:
                    B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
            out[how] = be.host(d.evisc)
        assert same(out["inline"], out["pointer"]), (route, shape, cm.ulp_diff(out["inline"], out["pointer"]))
        assert not same(out["inline"], c.evisc)


# ---- the buoyancy folded into the fused RHS passes -------------------------------------------------------------------------
PAIRS = [  # advec, diff, order, environment
    pytest.param(cm.ADVEC_2I5, cm.DIFF_SMAG2, 2, {}, id="2i5-smag2-march"),
    pytest.param(cm.ADVEC_2I5, cm.DIFF_SMAG2, 2, {"MHH_RHS25_IMPL": "cell"}, id="2i5-smag2-cell"),
    pytest.param(cm.ADVEC_4, cm.DIFF_4, 4, {}, id="4-4-march"),
    pytest.param(cm.ADVEC_4, cm.DIFF_4, 4, {"MHH_RHS44_IMPL": "cell"}, id="4-4-cell"),
    pytest.param(cm.ADVEC_2, cm.DIFF_2, 2, {}, id="2-2"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("adv,dif,order,env", PAIRS)
@pytest.mark.parametrize("form", ["flat", "sloped"])
def test_folded_buoyancy_equals_standalone_then_unfused(be, dtype, adv, dif, order, env, form):
    """mhh_rhs_exec with Thermo_buoy's buoyancy (buoyancy_kind = 1) against mhh_thermo_buoy_tend followed by mhh_advec_exec and
    mhh_diff_exec (Thermo::exec precedes Advec::exec, src/model.cxx:366,388): the same bits, with b as scalar 0 (folded into the
    marching 2i5 kernel) and as scalar 1 (its own launch first)."""
    alpha, n2, utrans = FORMS[form]
    sm = 1 if dif == cm.DIFF_SMAG2 else 0
    shapes = [(16, 12, 10), (17, 9, 8)] if order == 2 else [(16, 12, 12), (17, 9, 10), (20, 1, 12)]   # jtot = 1: rhs44 keeps the separate launch
    if order == 2 and dtype == np.float32:
        shapes.append((128, 9, 8))            # imax % 128 == 0: the packed-fp32 (two cells per lane) form of the rhs25 marching kernel
    for shape in shapes:
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype) if order == 2 else cm.grid_4th(*shape, dtype=dtype)
        c = case(g, nscalars=2)
        for nb in (0, 1):
            out = {}
            for how in ("folded", "alone"):
                keep = []
                d = B.DevCase(be, c); f = d.fields()
                p = _visc_params(be, g, sm, keep) if sm else capi.MhhDiffParams()
                if not sm:
                    p.cs = 0.23; p.tPr = 1./3.
                with cm.switches(**env):
                    if how == "folded":
                        p.buoyancy = order; p.buoyancy_kind = 1; p.th_for_N2 = nb; p.alpha, p.bg_n2, p.utrans = alpha, n2, utrans
                        B.ok(be, be.lib.mhh_rhs_exec(d.G, adv, dif, C.byref(f), C.byref(p), be.stream))
                    else:
                        tend(be, d, order, nb, alpha, n2, utrans)
                        B.ok(be, be.lib.mhh_advec_exec(d.G, adv, C.byref(f), be.stream))
                        B.ok(be, be.lib.mhh_diff_exec(d.G, dif, C.byref(f), C.byref(p), be.stream))
                out[how] = [be.host(d.ut), be.host(d.vt), be.host(d.wt)] + [be.host(x) for x in d.st]
            for a, b, nm in zip(out["folded"], out["alone"], ("ut", "vt", "wt", "s0t", "s1t")):
                assert same(a, b), (form, shape, nb, nm, cm.ulp_diff(a, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_flat_buoyancy_in_the_row_forms(be, dtype):
    """mhh_rhs_exec_rows / _rows2 fold the flat Thermo_buoy form of scalar 0 like the whole-slab call."""
    g = cm.grid_2nd(16, 14, 10, gc=(3, 3, 1), dtype=dtype)
    c = case(g, nscalars=1)
    out = {}
    for how in ("whole", "rows"):
        keep = []
        d = B.DevCase(be, c); f = d.fields()
        p = _visc_params(be, g, 1, keep)
        p.buoyancy = 2; p.buoyancy_kind = 1; p.th_for_N2 = 0
        if how == "whole":
            B.ok(be, be.lib.mhh_rhs_exec(d.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
        else:
            ja, jb = g.jstart + 4, g.jend - 4
            B.ok(be, be.lib.mhh_rhs_exec_rows(d.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f), C.byref(p), ja, jb, be.stream))
            B.ok(be, be.lib.mhh_rhs_exec_rows2(d.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f), C.byref(p), g.jstart, ja, jb, g.jend, be.stream))
        out[how] = [be.host(d.ut), be.host(d.vt), be.host(d.wt), be.host(d.st[0])]
    for a, b in zip(out["whole"], out["rows"]):
        assert same(a, b), cm.ulp_diff(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_initialised_params_keep_the_dry_meaning(be, dtype):
    """buoyancy_kind = 0 (zero-initialised params): the dry N2 from th with thref and grav, and the dry buoyancy folded as before."""
    g = cm.grid_2nd(16, 12, 10, gc=(3, 3, 1), dtype=dtype)
    c = cm.Case(g, nscalars=1, periodic=True)
    T = g.np_dtype.type
    thref = np.full(g.kcells, 300., dtype=dtype); threfh = (300. + 0.37*np.arange(g.kcells)).astype(dtype)
    out = {}
    for how in ("inline", "alone"):
        keep = []
        d = B.DevCase(be, c); f = d.fields()
        p = _visc_params(be, g, 1, keep)
        dthref, dthrefh = be.arr(thref), be.arr(threfh); keep += [dthref, dthrefh]
        p.grav = 9.81
        if how == "inline":
            p.th_for_N2 = 0; p.thref = be.ptr(dthref).value
            p.buoyancy = 2; p.threfh = be.ptr(dthrefh).value
            B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
            B.ok(be, be.lib.mhh_rhs_exec(d.G, cm.ADVEC_2I5, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
        else:
            n2 = be.zeros(g.shape3, dtype); keep.append(n2)
            B.ok(be, be.lib.mhh_calc_N2(d.G, be.ptr(n2), be.ptr(d.s[0]), be.ptr(dthref), T(9.81), be.stream))
            p.N2 = be.ptr(n2).value; p.th_for_N2 = -1
            B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
            B.ok(be, be.lib.mhh_thermo_dry_buoyancy_tend(d.G, 2, be.ptr(d.wt), be.ptr(d.s[0]), be.ptr(dthrefh), 9.81, be.stream))
            B.ok(be, be.lib.mhh_advec_exec(d.G, cm.ADVEC_2I5, C.byref(f), be.stream))
            B.ok(be, be.lib.mhh_diff_exec(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
        out[how] = [be.host(d.evisc), be.host(d.ut), be.host(d.vt), be.host(d.wt), be.host(d.st[0])]
    for a, b, nm in zip(out["inline"], out["alone"], ("evisc", "ut", "vt", "wt", "tht")):
        assert same(a, b), (nm, cm.ulp_diff(a, b))


# ---- full-size cases on the GPU ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case_name,shape", [("drycbl", (512, 256, 256)), ("drycbl", (1024, 1, 384)), ("sbl", (256, 256, 256))])
def test_fullsize_buoy_cases_folded_equals_unfolded(case_name, shape):
    """HotPath of the Thermo_buoy cases: the step with the folded buoyancy against Thermo_buoy::exec on its own followed by the
    unfused Advec::exec + Diff::exec, bit for bit; then the pressure solve leaves the divergence at the level of the other cases."""
    import torch
    from microhh_amd.model import HotPath
    out = {}
    for how in ("folded", "unfolded"):
        hp = HotPath(case_name, *shape)
        assert hp.buoyant
        hp.cyclic_prognostic(); hp.exec_viscosity()
        (hp.rhs if how == "folded" else hp.rhs_unfused)()
        torch.cuda.synchronize()
        out[how] = [t.detach().cpu().numpy() for t in (hp.ut, hp.vt, hp.wt, hp.st[0])]
        if how == "folded":
            hp.pres()
            d1, d0 = hp.projected_divergence()
            assert d0 > 1e-3 and d1 / d0 < 1e-9, (case_name, shape, d1, d0)
        hp.close()
    for a, b, nm in zip(out["folded"], out["unfolded"], ("ut", "vt", "wt", "bt")):
        assert same(a, b), (case_name, shape, nm, cm.ulp_diff(a, b))
