"""The launch geometry of large and ragged grids: which block works which cells, against the CPU oracle bit for bit.

Three host-side tilers deal (strip, k-chunk) units round-robin to the 8 XCDs: make_tiling / decode_tile (csrc/k_common.h, every
one-thread-per-cell kernel), make_march_tiling / decode_march / march_tile_rows (csrc/k_march_common.h, the k-marching kernels) and
level_tiling / level_tile (csrc/level_reduce.h, the level reductions). A strip holds ``sr`` tile rows: 4 on every benchmark grid, fewer
where there are few rows. The other parity modules stay at jtot <= 37, that is sr = 1; this one runs thin grids (few columns, many
rows) whose tilings are those of the benchmark grids and of large grids that are no power of two: sr = 2, 3, 4, a last strip cut by
the end of the rows, a last round of units with idle XCD slots, several k-chunks, and a two-range launch one of whose strips holds
tile rows of both ranges.

tests/cpp/tiling_probe.cpp includes the three headers themselves: mode ``cover`` walks the real decoders over a sweep of tilings,
mode ``describe`` prints the tiling the library uses for a launch (so the class of a shape below comes from the headers, not from a
copy in Python), mode ``divknown`` compares div_known (csrc/cell_ops.h) with the IEEE quotient for the turbulent Prandtl numbers
the cases draw from TPRS. Every comparison with the oracle is np.array_equal, except the one exec_viscosity-against-oracle bound of
8 ulp taken over from tests/test_parity.py::test_exec_viscosity. The level tiler's shapes run in tests/test_reduction_order.py
(means_common.LEVEL_SHAPES).

Runs on the ``emul`` backend and on the ``hip`` backend (marked gpu); one test per kernel family and dtype.
"""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import common as cm
import means_common
import micro_ref as R
import moist_ref as M
from backends import be  # noqa: F401
from common import DTYPES, ptr, dbl
from test_layout_matrix import _report

ADV, DIF = cm.ADVEC_2I5, cm.DIFF_SMAG2
TPRS = (1./3., 0.4, 0.7, 0.85, 1.0)
GRAV = 9.81
RHS25_KC, VISC_KC, MOIST_KC, NJ = 128, 64, 32, 4            # the k-chunks and tile rows of the kernels (k_march.hip, k_visc.hip, thermo_moist.h)

# (itot, jtot, ktot), levels per k-chunk (MHH_MARCH_KC_RT / MHH_VISC_KC_RT) or None, scalars, the flux-limited ones, dtypes.
# What each is there for (march tiler; the cell tiler of the same shape in brackets) -- test_matrix_reaches_every_geometry_class
# prints the table from the probe:
GRIDS = [
    ((66, 100, 20), 8, 1, (), DTYPES),        # sr 4, last strip cut, 21 units, three k-chunks [sr 3, cut]
    ((130, 132, 9), None, 3, (1,), DTYPES),   # sr 4, 9 strips of which the last holds one tile row, three tiles per row [sr 4, cut]
    ((8, 128, 24), 8, 0, (), DTYPES),         # sr 4, 8 whole strips, 24 units, one tile per row [sr 4, whole]
    ((66, 128, 20), 8, 1, (), DTYPES),        # the class of every benchmark grid: sr 4, whole strips, units a multiple of 8, nbx > 1, nkc > 1
    ((66, 64, 9), None, 3, (2,), DTYPES),     # sr 2, 8 whole strips [the 512 x 64 x 512 slab rank's: sr 2, whole]
    ((8, 68, 9), None, 0, (), DTYPES),        # sr 2, cut
    ((66, 96, 9), None, 1, (), DTYPES),       # sr 3, 8 whole strips
    ((8, 36, 9), None, 3, (), DTYPES),        # sr 1, 9 strips: one idle round
    ((8, 24, 9), None, 1, (), DTYPES),        # sr 1, 6 strips [two k-segments]
    ((128, 100, 9), None, 1, (), [np.float32]),   # fp32, two cells per lane (tiles of 128 cells): sr 3, cut, one tile per row
    ((256, 68, 9), None, 1, (), [np.float32]),    # the same with two tiles per row: sr 2, cut
]
GRIDS_4 = [((66, 100, 12), 1), ((8, 128, 12), 0), ((130, 68, 12), 1)]
VISC_GRIDS = [((66, 100, 20), 8), ((130, 132, 9), None), ((8, 128, 24), 8), ((66, 96, 9), None), ((8, 68, 9), None)]
MOIST_SHAPES = [(66, 100, 40), (130, 132, 9)]
ROWS2_SHAPE = (66, 128, 9)
BENCH = [(512, 512, 512), (256, 256, 256), (512, 256, 256), (1024, 1024, 256), (1024, 128, 256), (512, 64, 512)]


# ---- the probe ------------------------------------------------------------------------------------------------------------------
_probe = []


def probe():
    """tests/cpp/tiling_probe.cpp built once per session with the host compiler, as tests/emul/Makefile builds the kernels."""
    if not _probe:
        tmp = tempfile.TemporaryDirectory()
        exe = os.path.join(tmp.name, "tiling_probe")
        t = os.path.join(cm.ROOT, "tests")
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-march=native", "-pthread", "-ffp-contract=off", "-I", os.path.join(t, "emul"),
                        "-I", os.path.join(cm.ROOT, "microhh_amd", "csrc"), "-Wno-attributes", "-Wno-unused-value", "-o", exe,
                        os.path.join(t, "cpp", "tiling_probe.cpp"), os.path.join(t, "emul", "emul_globals.cpp")], check=True)
        _probe.extend([tmp, exe])
    return _probe[1]


def run_probe(mode, *args, stdin=None, kc_rt=None, tune="MHH_MARCH_KC_RT"):
    env = {k: v for k, v in os.environ.items() if k not in ("MHH_MARCH_KC_RT", "MHH_VISC_KC_RT")}
    if kc_rt:
        env[tune] = str(kc_rt)
    r = subprocess.run([probe(), mode, *args], input=stdin, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "tiling_probe ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def describe(shape, kc, kc_rt=None, tw=64, rows=(), tune="MHH_MARCH_KC_RT", levels=None):
    """{"cell": .., "march": .., "level": ..} of a launch over `shape`, from the library's headers."""
    line = "%d %d %d %d %d %d" % (shape[0], shape[1], levels or shape[2], NJ, kc, tw) + "".join(" %d" % j for j in rows) + "\n"
    out = run_probe("describe", tune, stdin=line, kc_rt=kc_rt, tune=tune)
    return json.loads(out.splitlines()[0])


def march_class(m):
    return ("sr %d" % m["sr"], "whole strips" if m["nby"] % m["sr"] == 0 else "cut strip", "units % 8 == 0" if (m["ns"]*m["nkc"]) % 8 == 0 else "idle slots",
            "nbx 1" if m["nbx"] == 1 else "nbx > 1", "nkc 1" if m["nkc"] == 1 else "nkc > 1")


def cell_class(t, with_nbx=True):
    units = t["ns"]*t["nseg"]
    return ("sr %d" % t["sr"], "whole strips" if t["nby"] % t["sr"] == 0 else "cut strip", "units % 8 == 0" if units % 8 == 0 else "idle slots",
            ("nbx 1" if t["nbx"] == 1 else "nbx > 1") if with_nbx else "nbx 1", "one k-segment" if t["nseg"] == 1 else "k-segments")


def test_decoders_cover_every_tile_once():
    """decode_tile, decode_march + march_tile_rows and level_tile over nbx 1..3, nby 1..140, nk or nkc 1..20, two-range launches
    included: every (bx, by, kz or kc) exactly once, nothing else, and the rows handed out are the rows asked for."""
    out = run_probe("cover")
    assert "decode every tile once" in out, out
    print(out)


def _rows2(g):
    return (g.jstart, g.jstart + 50, g.jend - 47, g.jend)


def test_matrix_reaches_every_geometry_class():
    """The shapes of this module (and, for the level tiler, of tests/test_reduction_order.py) reach every launch-geometry class
    of each tiler, and the class of every benchmark grid is among them. The table printed is the one of the pull request."""
    march, cell, level, straddle = {}, {}, {}, []
    for shape, kc_rt, nsc, lim, dtypes in GRIDS:
        tw = 128 if (np.float32 in dtypes and len(dtypes) == 1) else 64
        d = describe(shape, RHS25_KC, kc_rt, tw)
        march.setdefault(march_class(d["march"]), []).append((shape, kc_rt, "rhs25"))
        cell.setdefault(cell_class(d["cell"]), []).append(shape)
    for shape, kc_rt in VISC_GRIDS:
        d = describe(shape, VISC_KC, kc_rt, tune="MHH_VISC_KC_RT")
        march.setdefault(march_class(d["march"]), []).append((shape, kc_rt, "visc"))
    for shape in MOIST_SHAPES:
        d = describe(shape, MOIST_KC)
        march.setdefault(march_class(d["march"]), []).append((shape, None, "moist, micro"))
    g = cm.grid_2nd(*ROWS2_SHAPE)
    for kc, tune, who in ((RHS25_KC, "MHH_MARCH_KC_RT", "rhs25 rows2"), (VISC_KC, "MHH_VISC_KC_RT", "visc rows2")):
        d = describe(ROWS2_SHAPE, kc, rows=_rows2(g), tune=tune)["march"]
        assert (d["nby1"], d["nby"], d["sr"]) == (13, 25, 3), d
        if d["straddle"]:
            straddle.append((ROWS2_SHAPE, who))
        march.setdefault(march_class(d), []).append((ROWS2_SHAPE, None, who))
    for shape in means_common.LEVEL_SHAPES:
        d = describe(shape, RHS25_KC, levels=shape[2] + 2)
        level.setdefault(cell_class(d["level"], False), []).append(shape)
    for name, table in (("march tiler", march), ("cell tiler", cell), ("level tiler", level)):
        for k in sorted(table):
            print("%-12s %-70s %s" % (name, ", ".join(k), table[k]))
    print("rows2 launch with a strip over both ranges:", straddle)

    def axis(table, n):
        return {k[n] for k in table}
    for name, table in (("march", march), ("cell", cell), ("level", level)):
        assert axis(table, 0) == {"sr 1", "sr 2", "sr 3", "sr 4"}, (name, axis(table, 0))
        assert axis(table, 1) == {"whole strips", "cut strip"}, (name, axis(table, 1))
        assert axis(table, 2) == {"units % 8 == 0", "idle slots"}, (name, axis(table, 2))
    assert axis(march, 3) == {"nbx 1", "nbx > 1"} and axis(cell, 3) == {"nbx 1", "nbx > 1"}      # (a level launch has one block column)
    assert axis(march, 4) == {"nkc 1", "nkc > 1"}
    assert axis(cell, 4) == {"one k-segment", "k-segments"} and axis(level, 4) == {"one k-segment", "k-segments"}
    assert len(straddle) == 2, straddle
    for shape in BENCH:
        d = describe(shape, RHS25_KC, levels=shape[2])
        assert march_class(d["march"]) in march, ("march", shape, d["march"])
        assert cell_class(d["cell"]) in cell, ("cell", shape, d["cell"])
        assert cell_class(describe(shape, RHS25_KC, levels=shape[2] + 2)["level"], False) in level, ("level", shape)
        print("benchmark grid %-18s march: %s; cell: %s" % (shape, ", ".join(march_class(d["march"])), ", ".join(cell_class(d["cell"]))))


def test_div_known_is_the_ieee_quotient_for_the_prandtl_numbers_of_this_module():
    """div_known(x, d, RN(1/d)) == x / d for d = tPr and 2 tPr of TPRS: every fp32 significand of x, both signs, and every 101st
    in binades from 2^100 down to the bound stated in cell_ops.h (2^-100, every binade from 2^-70 on); 10^8 random fp64 pairs above
    that header's fp64 bound. Below the fp32 bound the probe reports where the first mismatch lies."""
    out = run_probe("divknown")
    print(out)
    assert "fp64: 100000000 random pairs exact" in out
    assert sum("exact for |x| >= 2^-100" in ln for ln in out.splitlines()) == 2*len(TPRS), out
    firsts = [int(ln.rsplit("2^", 1)[1]) for ln in out.splitlines() if "first mismatch in the binade" in ln]
    assert all(f < -100 for f in firsts), firsts


# ---- the fused (advec_2i5, diff_smag2) pass ---------------------------------------------------------------------------------------
def _svisc(n):
    return [1e-5 * (1 + 0.25*m) for m in range(n)]


def _compare(fails, key, got, want):
    names = ["ut", "vt", "wt"] + ["st%d" % n for n in range(len(want[3]))]
    for nm, a, b in zip(names, cm.flat(got), cm.flat(want)):
        if not np.array_equal(a, b):
            fails.append("%s %s: %s" % (key, nm, _report(a, b)))


def _dev(be, c, limited=()):
    d = B.DevCase(be, c); f = d.fields()
    for n, sv in enumerate(_svisc(len(c.s))):
        f.svisc[n] = sv
    for n in limited:
        f.s_fluxlimit[n] = 1
    return d, f


_oracle = {}


def _want(c, key, adv, dif, sm, tPr, limited, advec_only=False):
    """The oracle's tendencies of a case, computed once and shared by the forms, the backends and the tests; never written to."""
    key = key + (advec_only,)
    if key not in _oracle:
        _oracle[key] = cm.oracle_rhs(c, adv, None if advec_only else dif, sm, tPr=tPr, svisc=_svisc(len(c.s)), limited=limited)
    return _oracle[key]


def _clean(fails):
    assert not fails, "%d mismatches:\n%s" % (len(fails), "\n".join(fails))


CELL25 = dict(MHH_RHS25_IMPL="cell", MHH_ADVEC25_IMPL="cell", MHH_DIFF22_IMPL="cell", MHH_SCALAR_IMPL="cell")


@pytest.mark.parametrize("dtype", DTYPES)
def test_advec_2i5_diff_smag2_marching_and_cell_forms_on_every_geometry_class(be, dtype):
    """mhh_rhs_exec in the marching form and in the cell form, and mhh_advec_exec followed by mhh_diff_exec, on every shape of
    GRIDS with 0, 1 and 3 scalars (one flux-limited), tPr drawn per shape: the oracle's bits."""
    fails = []
    for n, (shape, kc_rt, nsc, limited, dtypes) in enumerate(GRIDS):
        if dtype not in dtypes:
            continue
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype)
        sm, tPr = n % 2, TPRS[n % len(TPRS)]
        c = cm.Case(g, nscalars=nsc, rho=("random", "one")[n % 2])
        ck = ("25", np.dtype(dtype).name, shape)
        want = _want(c, ck, ADV, DIF, sm, tPr, limited)
        key = "%s %s kc %s sm %d tPr %.3g nsc %d lim %s" % (np.dtype(dtype).name, shape, kc_rt, sm, tPr, nsc, limited)
        p = cm.diff_params(sm, tPr=tPr)
        for form, env in (("march", {}), ("cell", CELL25)):
            with cm.switches(MHH_MARCH_KC_RT=kc_rt, **env):
                d, f = _dev(be, c, limited)
                n0 = be.lib.mhh_stat_scalar_march_launches()
                B.ok(be, be.lib.mhh_rhs_exec(d.G, ADV, DIF, C.byref(f), C.byref(p), be.stream))
                if nsc > 1:                                        # scalars 1, 2: the scalar pass in the marching form only
                    assert (be.lib.mhh_stat_scalar_march_launches() > n0) == (form == "march"), (key, form)
                if form == "march" and len(dtypes) == 1:
                    v = [C.c_int(0) for _ in range(4)]
                    B.ok(be, be.lib.mhh_stat_march_form(0, *[C.byref(x) for x in v]))
                    assert v[3].value == 2, (key, "two cells per lane")
                _compare(fails, key + " rhs_exec " + form, cm.tendencies(be, d), want)
        with cm.switches(MHH_MARCH_KC_RT=kc_rt):
            d, f = _dev(be, c, limited)
            B.ok(be, be.lib.mhh_advec_exec(d.G, ADV, C.byref(f), be.stream))
            _compare(fails, key + " advec_exec", cm.tendencies(be, d), _want(c, ck, ADV, DIF, sm, tPr, limited, advec_only=True))
            B.ok(be, be.lib.mhh_diff_exec(d.G, DIF, C.byref(f), C.byref(p), be.stream))
            _compare(fails, key + " advec_exec + diff_exec", cm.tendencies(be, d), want)
    _clean(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_prandtl_number_div_known_cannot_take_is_refused(be, dtype):
    """tPr whose doubled significand is all ones (the largest value below 1): mhh_rhs_exec with a scalar returns an error that
    names tPr and writes no tendency."""
    g = cm.grid_2nd(16, 12, 10, dtype=dtype)
    c = cm.Case(g, nscalars=1)
    d, f = _dev(be, c)
    p = cm.diff_params(1, tPr=float(np.nextafter(dtype(1), dtype(0))))
    assert be.lib.mhh_rhs_exec(d.G, ADV, DIF, C.byref(f), C.byref(p), be.stream) != 0
    assert b"tPr" in be.lib.mhh_last_error(), be.lib.mhh_last_error()
    be.sync()
    for a, b in zip(cm.flat(cm.tendencies(be, d)), (c.ut, c.vt, c.wt, c.st[0])):
        assert cm.same_bits(a, b)


# ---- 4th order, 2nd order, and the cell kernels that are no RHS --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_advec_4_diff_4_marching_and_cell_forms(be, dtype):
    """mhh_rhs_exec for (advec_4, diff_4) in the marching and the cell form on sr = 3 (cut), sr = 4 and sr = 2 (cut), and once with
    the 4th-order scalar pass (MHH_SCALAR_IMPL=march) over three k-chunks."""
    fails = []
    runs = [(shape, nsc, None, env, form) for shape, nsc in GRIDS_4 for form, env in (("march", {}), ("cell", {"MHH_RHS44_IMPL": "cell"}))]
    runs.append(((66, 100, 20), 2, 8, {"MHH_SCALAR_IMPL": "march"}, "scalar pass"))
    for shape, nsc, kc_rt, env, form in runs:
        g = cm.grid_4th(*shape, dtype=dtype)
        c = cm.Case(g, nscalars=nsc)
        want = _want(c, ("44", np.dtype(dtype).name, shape, nsc), cm.ADVEC_4, cm.DIFF_4, 0, 1./3., ())
        d, f = _dev(be, c)
        n0, m0 = be.lib.mhh_stat_scalar4_march_launches(), be.lib.mhh_stat_rhs44_march_launches()
        with cm.switches(MHH_MARCH_KC_RT=kc_rt, **env):
            B.ok(be, be.lib.mhh_rhs_exec(d.G, cm.ADVEC_4, cm.DIFF_4, C.byref(f), C.byref(cm.diff_params(0)), be.stream))
        assert be.lib.mhh_stat_rhs44_march_launches() - m0 == (0 if form == "cell" else 1), (shape, form)
        if form == "scalar pass":
            assert be.lib.mhh_stat_scalar4_march_launches() > n0
        _compare(fails, "%s %s 4th order %s" % (np.dtype(dtype).name, shape, form), cm.tendencies(be, d), want)
    _clean(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_kernels_advec_2_diff_2_cyclic_rk_and_pressure_stages(be, dtype):
    """The one-thread-per-cell launcher on sr = 3 with a cut strip and on sr = 4 with 9 strips: advec_2 + diff_2, the cyclic
    fills, the Runge-Kutta sub-step, and mhh_pres_input / mhh_pres_output in the staged form, each with the oracle's bits."""
    O = cm.oracle()
    fails = []
    for shape in ((66, 100, 9), (130, 132, 9)):
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype)
        Gh = g.host_struct()
        c = cm.Case(g, nscalars=1)
        tag = "%s %s" % (np.dtype(dtype).name, shape)
        if shape[0] == 66:
            d, f = _dev(be, c)
            B.ok(be, be.lib.mhh_rhs_exec(d.G, cm.ADVEC_2, cm.DIFF_2, C.byref(f), C.byref(cm.diff_params(0)), be.stream))
            _compare(fails, tag + " advec_2 + diff_2", cm.tendencies(be, d), _want(c, ("22", np.dtype(dtype).name, shape), cm.ADVEC_2, cm.DIFF_2, 0, 1./3., ()))
        for edge in (cm.EDGE_EW, cm.EDGE_NS, cm.EDGE_BOTH):
            want = c.u.copy(); O.orc_boundary_cyclic(Gh, ptr(want), edge)
            da = be.arr(c.u)
            B.ok(be, be.lib.mhh_boundary_cyclic(be.grid(g), be.ptr(da), edge, be.stream))
            if not np.array_equal(be.host(da), want):
                fails.append("%s boundary_cyclic edge %d: %s" % (tag, edge, _report(be.host(da), want)))
        for order, sub in ((3, 1), (4, 4)):
            a, at = c.u.copy(), c.ut.copy()
            O.orc_rk_substep(Gh, order, sub, dbl(0.31), ptr(a), ptr(at))
            da, dat = be.arr(c.u), be.arr(c.ut)
            B.ok(be, be.lib.mhh_rk_substep(be.grid(g), order, sub, 0.31, be.ptr(da), be.ptr(dat), be.stream))
            for nm, x, y in (("a", be.host(da), a), ("at", be.host(dat), at)):
                if not np.array_equal(x, y):
                    fails.append("%s rk%d substep %d %s: %s" % (tag, order, sub, nm, _report(x, y)))
    # the pressure stages around the solve (tests/test_parity.py::test_pres), staged form
    g = cm.grid_2nd(66, 100, 9, gc=(3, 3, 1), dtype=dtype)
    Gh = g.host_struct(); dt = 0.7
    c = cm.Case(g, periodic=True)
    d = B.DevCase(be, c); f = d.fields()
    with cm.switches(MHH_PRES_LDS="0"), B.pres_plan(be, g, c, 2) as plan:
        pk_want = np.zeros((g.ktot, g.jtot, g.itot), dtype=dtype)
        ut, vt, wt = c.ut.copy(), c.vt.copy(), c.wt.copy()
        O.orc_pres_input(Gh, 2, ptr(pk_want), ptr(c.u), ptr(c.v), ptr(c.w), ptr(ut), ptr(vt), ptr(wt), ptr(c.rhoref), ptr(c.rhorefh), dbl(dt))
        pk = be.zeros((g.ktot, g.jtot, g.itot), dtype)
        B.ok(be, be.lib.mhh_pres_input(plan, d.G, C.byref(f), dt, be.ptr(pk), be.stream))
        for nm, x, y in (("packed p", be.host(pk), pk_want), ("ut", be.host(d.ut), ut), ("vt", be.host(d.vt), vt), ("wt", be.host(d.wt), wt)):
            if not np.array_equal(x, y):
                fails.append("pres_input %s %s: %s" % (np.dtype(dtype).name, nm, _report(x, y)))
        p_in = cm.Case(g, seed=7, periodic=True).u                 # any periodic field serves as p: the stage is checked on its own
        dp = be.arr(p_in); f2 = d.fields(); f2.p = be.ptr(dp).value
        O.orc_pres_output(Gh, 2, ptr(ut), ptr(vt), ptr(wt), ptr(p_in))
        B.ok(be, be.lib.mhh_pres_output(plan, d.G, C.byref(f2), be.stream))
        for nm, x, y in (("ut", be.host(d.ut), ut), ("vt", be.host(d.vt), vt), ("wt", be.host(d.wt), wt)):
            if not np.array_equal(x, y):
                fails.append("pres_output %s %s: %s" % (np.dtype(dtype).name, nm, _report(x, y)))
    _clean(fails)


# ---- exec_viscosity -----------------------------------------------------------------------------------------------------------------
def _visc_call(be, c, sm, tPr, thref, impl, kc_rt=None, rows=None):
    g = c.grid
    d = B.DevCase(be, c); f = d.fields()
    p = cm.diff_params(sm, tPr=tPr)
    p.N2 = None; p.th_for_N2 = 0; dth = be.arr(thref); p.thref = be.ptr(dth).value; p.grav = GRAV
    ml = B.mlen0(be, g, 0.23); p.mlen0 = be.ptr(ml).value
    with cm.switches(MHH_VISC_IMPL=impl, MHH_VISC_KC_RT=kc_rt):
        n0 = be.lib.mhh_stat_visc_march_launches()
        if rows:
            B.ok(be, be.lib.mhh_diff_exec_viscosity_rows2(d.G, DIF, C.byref(f), C.byref(p), *rows, be.stream))
        else:
            B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, DIF, C.byref(f), C.byref(p), be.stream))
        assert be.lib.mhh_stat_visc_march_launches() - n0 == (1 if impl == "march" else 0), (impl, g.shape3)
    return be.host(d.evisc)


def _visc_oracle(c, sm, tPr, thref):
    O = cm.oracle(); g = c.grid; Gh = g.host_struct(); dtype = g.np_dtype
    want = np.zeros(g.shape3, dtype=dtype); n2 = np.zeros(g.shape3, dtype=dtype)
    O.orc_smag2_strain2(Gh, sm, ptr(want), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.dudz), ptr(c.dvdz))
    O.orc_calc_N2(Gh, ptr(n2), ptr(c.s[0]), ptr(thref), dbl(GRAV))
    O.orc_smag2_evisc(Gh, sm, ptr(want), ptr(n2), ptr(c.dbdz), ptr(c.z0m), dbl(0.23), dbl(tPr))
    return want


@pytest.mark.parametrize("dtype", DTYPES)
def test_exec_viscosity_marching_form_equals_cell_form_and_the_oracle(be, dtype):
    """mhh_diff_exec_viscosity on VISC_GRIDS: the marching form has the cell form's bits, and the cell form of the first shape lies
    within the 8 ulp of tests/test_parity.py::test_exec_viscosity of the oracle's three steps."""
    fails = []
    for n, (shape, kc_rt) in enumerate(VISC_GRIDS):
        g = cm.grid_2nd(*shape, gc=(3, 3, 1), dtype=dtype)
        c = cm.Case(g, periodic=True)
        sm, tPr = (n + 1) % 2, TPRS[(n + 2) % len(TPRS)]
        thref = (300. + 7.*np.sin(0.37*np.arange(g.kcells))).astype(dtype)
        cell = _visc_call(be, c, sm, tPr, thref, "cell")
        march = _visc_call(be, c, sm, tPr, thref, "march", kc_rt)
        if not np.array_equal(march, cell):
            fails.append("%s %s kc %s sm %d tPr %.3g exec_viscosity march vs cell: %s" % (np.dtype(dtype).name, shape, kc_rt, sm, tPr, _report(march, cell)))
        if n == 0:
            want = _visc_oracle(c, sm, tPr, thref)
            ulp = cm.ulp_diff(cell[g.kstart:g.kend], want[g.kstart:g.kend])
            print("exec_viscosity %s %s cell form against the oracle: %.3g ulp" % (np.dtype(dtype).name, shape, ulp))
            assert ulp <= 8, ulp
    _clean(fails)


# ---- two row ranges in one launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_row_ranges_with_a_strip_over_both(be, dtype):
    """mhh_rhs_exec_rows2 and mhh_diff_exec_viscosity_rows2 over [jstart, jstart + 50) and [jend - 47, jend) of jtot = 128: 13 + 12
    tile rows in strips of 3, so the fifth strip holds tile rows of both ranges (asserted through the probe by
    test_matrix_reaches_every_geometry_class). The rows of both ranges have the oracle's bits, every other row keeps its input bits."""
    fails = []
    g = cm.grid_2nd(*ROWS2_SHAPE, gc=(3, 3, 1), dtype=dtype)
    j0, j1, j2, j3 = _rows2(g)
    inside = np.zeros(g.jcells, dtype=bool); inside[j0:j1] = True; inside[j2:j3] = True
    sm, tPr = 1, 0.7
    c = cm.Case(g, nscalars=1)
    want = _want(c, ("rows2", np.dtype(dtype).name), ADV, DIF, sm, tPr, ())
    d, f = _dev(be, c)
    p = cm.diff_params(sm, tPr=tPr)
    B.ok(be, be.lib.mhh_rhs_exec_rows2(d.G, ADV, DIF, C.byref(f), C.byref(p), j0, j1, j2, j3, be.stream))
    for nm, got, w, src in zip(("ut", "vt", "wt", "st0"), cm.flat(cm.tendencies(be, d)), cm.flat(want), (c.ut, c.vt, c.wt, c.st[0])):
        if not np.array_equal(got[:, inside], w[:, inside]):
            fails.append("%s rhs_exec_rows2 %s, rows of the ranges: %s" % (np.dtype(dtype).name, nm, _report(got[:, inside], w[:, inside])))
        if not cm.same_bits(got[:, ~inside], src[:, ~inside]):
            fails.append("%s rhs_exec_rows2 %s: rows outside the ranges were written" % (np.dtype(dtype).name, nm))
        assert not np.array_equal(w[:, inside], src[:, inside])
    # exec_viscosity: the whole-slab cell form is the reference of the rows' bits; it is tied to the oracle at 8 ulp here as well
    c = cm.Case(g, periodic=True)
    thref = (300. + 7.*np.sin(0.37*np.arange(g.kcells))).astype(dtype)
    whole = _visc_call(be, c, sm, tPr, thref, "cell")
    rows = _visc_call(be, c, sm, tPr, thref, "march", rows=(j0, j1, j2, j3))
    ks, ke, cols = g.kstart, g.kend, slice(g.istart, g.iend)
    if not np.array_equal(rows[ks:ke, inside, cols], whole[ks:ke, inside, cols]):
        fails.append("%s exec_viscosity_rows2, rows of the ranges: %s" % (np.dtype(dtype).name, _report(rows[ks:ke, inside, cols], whole[ks:ke, inside, cols])))
    outside = ~inside; outside[:g.jstart] = False; outside[g.jend:] = False
    if not cm.same_bits(rows[ks:ke, outside, cols], c.evisc[ks:ke, outside, cols]):
        fails.append("%s exec_viscosity_rows2: rows outside the ranges were written" % np.dtype(dtype).name)
    want = _visc_oracle(c, sm, tPr, thref)
    ulp = cm.ulp_diff(rows[ks:ke, inside, cols], want[ks:ke, inside, cols])
    print("exec_viscosity_rows2 %s against the oracle: %.3g ulp" % (np.dtype(dtype).name, ulp))
    assert ulp <= 8, ulp
    _clean(fails)


# ---- the moist and micro marching kernels (k-chunks of 32 levels, tilings of their own) ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_moist_buoyancy_tendency_marching_form_equals_cell_form(be, dtype):
    """mhh_thermo_moist_buoyancy_tend on (66, 100, 40) (sr 4, 7 strips, two k-chunks) and (130, 132, 9) (9 strips): the marching form
    has the bits of the cell form, which tests/test_moist_tend.py ties to the reference at small shapes."""
    for shape in MOIST_SHAPES:
        c, g = M.field_case(shape), M.grid_of(shape, (3, 3, 1), dtype)
        host = {n: c.embed(np.asarray(a, dtype=dtype), g) for n, a in (("thl", c.thl), ("qt", c.qt), ("wt", c.wt))}
        tab = {"prefh": np.ascontiguousarray(c.prefh, dtype=dtype), "thvrefh": np.ascontiguousarray(c.thvrefh, dtype=dtype)}
        tab["exnrefh"] = np.ascontiguousarray(M.exn_like(c.prefh.astype(np.float64)), dtype=dtype)        # an Exner-like table: an input
        assert (c.thl[g.kstart+1:g.kend].astype(dtype) * tab["exnrefh"][g.kstart+1:g.kend, None, None] >= dtype(M.T0 + 1.)).all(), "warm inputs"
        out = {}
        for impl in (0, 1):                                        # MARCH, CELL (tests/test_moist_tend.py)
            dv = {n: be.arr(a) for n, a in host.items()}
            t = {n: be.arr(a) for n, a in tab.items()}
            keep, cptr, count = M.counter(be)
            B.ok(be, be.lib.mhh_thermo_moist_buoyancy_tend_impl(be.grid(g), impl, be.ptr(dv["wt"]), be.ptr(dv["thl"]), be.ptr(dv["qt"]), be.ptr(t["prefh"]),
                                                                be.ptr(t["exnrefh"]), be.ptr(t["thvrefh"]), cptr, be.stream))
            be.sync()
            out[impl] = be.host(dv["wt"]).reshape(g.shape3)
            assert count() == 0
        assert cm.same_bits(out[0], out[1]), (shape, _report(out[0], out[1]))
        assert not np.array_equal(out[1][g.interior], host["wt"][g.interior])


@pytest.mark.parametrize("dtype", DTYPES)
def test_warm_microphysics_marching_form_equals_cell_form(be, dtype):
    """mhh_micro_2mom_warm_exec, every process at once, on the same two shapes: the marching form has the bits of the cell form,
    which tests/test_micro_exec.py ties to the reference at small shapes."""
    for shape in MOIST_SHAPES:
        c = R.rain_case(shape)
        out = {}
        for impl in (R.MARCH, R.CELL):
            x = R.Dev(be, shape, (3, 3, 1), dtype)
            out[impl] = x.exec(R.ALL, c.dt["hi"], impl)
            assert x.count() == 0
        for n in ("qr", "nr") + R.OUT + ("rr_bot",):
            assert cm.same_bits(out[R.MARCH][n], out[R.CELL][n]), (shape, n, _report(out[R.MARCH][n], out[R.CELL][n]))
            if n in R.OUT:
                assert not cm.same_bits(out[R.CELL][n], x.h[n]), (shape, n)
