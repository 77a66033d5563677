"""Shared plumbing of the statistics tests (tests/test_stats_*.py): the seeded cases and their reference results.

The reference is the reference's OWN source (src/stats.cxx) behind tests/cpp/ref_stats_shim.cpp, compiled into a temporary directory
where the reference tree exists. Where it is absent the same cases read tests/golden/stats_ref.npz, recorded with
MHH_RECORD_STATS_GOLDEN=1 python -m pytest tests/test_stats_masks.py: reference OUTPUTS only (mask words, counts, areas, profiles,
time series). The inputs are not stored: every draw is numpy's seeded legacy generator, everything derived from a draw uses + - * /
only and is narrowed to values a float holds exactly, so they are the same numbers on every host and in both dtypes; the file holds
their digest per case. Two things are restated in NumPy: the cyclic fill of the mask words between the thresholds and calc_nmask
(periodic copies; the library's fills are pinned to the reference's by tests/test_pres_ref.py), and calc_grad_2nd, a member of
Stats<TF> that cannot be reached without an object (one loop, float64, in row order).
"""
import ctypes as C

import numpy as np

import common as cm
import moist_ref as M
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag
from microhh_amd.grid import Grid
from microhh_amd import stats as S

ZSIZE = 3000.

# (itot, jtot, ktot): 70 crosses a 64-lane row; jtot = 1 is the degenerate row; 37 rows make two row chunks with a ragged second one
SHAPES = [M.SHAPES[0], M.SHAPES[1], M.SHAPES[2], (24, 37, 8)]
STRETCHED = {SHAPES[0]: False, SHAPES[1]: True, SHAPES[2]: False, SHAPES[3]: True}
LAYOUTS = [(s, gc) for s in SHAPES[:3] for gc in M.GCS] + [(SHAPES[3], M.GCS[0])]
MASKS = ("default", "sparse", "topless")
# (variable, loc, offset, threshold, operations): a full-level and a half-level variable with every profile, a cloud-water-like one
VARS = [("a", 0, 0.5, 0., ("mean", "2", "3", "4", "grad")), ("wh", 1, 0., 0., ("mean", "2", "3", "4", "grad")),
        ("q", 0, 0., 1.e-5, ("mean", "frac", "path", "cover"))]
BOT_OFFSET = 0.25
OPCODE = {"mean": S.MEAN, "2": S.MOMENT2, "3": S.MOMENT3, "4": S.MOMENT4, "frac": S.FRAC, "grad": S.GRAD}


def flags(n):
    return np.uint32(1 << (2*n)), np.uint32(1 << (2*n + 1))


def grid_of(shape, gc, dtype, zsize=ZSIZE, stretched=None):
    z = None
    if STRETCHED.get(shape, False) if stretched is None else stretched:
        s = (np.arange(shape[2]) + 0.5)/shape[2]
        z = f32exact(zsize*(s + 0.6*s*s)/1.6)
    return Grid(shape[0], shape[1], shape[2], 6400., 6400., zsize, order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype, z=z)


class StatCase:
    """The variables and the thresholded fields of one shape on ktot + 2 levels (the vertical ghost levels hold seeded values: the
    profiles read level kend) of jtot x itot columns, the same for every ghost layout and both dtypes.
    sparse: about a third of the cells, no level empty. topless: about half, the top interior level empty on full and half levels."""

    def __init__(self, shape, kind="seeded"):
        self.shape, self.kind = shape, kind
        self.key = "%dx%dx%d%s" % (shape + ("" if kind == "seeded" else "-" + kind,))
        itot, jtot, ktot = shape
        rs = np.random.RandomState(7300 + itot + 7*ktot + 131*jtot)
        n3, n2 = (ktot + 2, jtot, itot), (jtot, itot)
        lev = np.arange(ktot + 2)[:, None, None]
        f = {}
        f["a"] = f32exact(3. + 0.25*lev + (rs.random_sample(n3) - 0.5))
        f["wh"] = f32exact(2.*(rs.random_sample(n3) - 0.5))
        cloud = rs.random_sample(n3) < 0.3
        f["q"] = f32exact(np.where(cloud, 1.e-3*rs.random_sample(n3), np.where(rs.random_sample(n3) < 0.5, 0., 8.e-6)))
        f["bot"] = f32exact(290. + rs.random_sample(n2))
        f["rho"] = f32exact(1.16 - 0.02*np.arange(ktot + 2))
        for h in ("", "h"):
            m = rs.random_sample(n3) - 2./3.
            m[:, 0, :1] = 0.125                                   # no level empty, the one of 20 cells too
            f["sparse" + h] = f32exact(m)
            m = rs.random_sample(n3) - 0.5
            m[ktot] = -np.abs(m[ktot]) - 0.125                    # kend-1 empty
            f["topless" + h] = f32exact(m)
        f["sparse_bot"] = f32exact(rs.random_sample(n2) - 0.5)
        f["topless_bot"] = f32exact(rs.random_sample(n2) - 0.5)
        if kind == "quirk":
            # a mask without a column (the NaN of path) and one whose first non-empty column is neither the first nor in the first row
            ij = np.arange(jtot*itot).reshape(n2)
            late = ij >= 2*itot + 3
            f["sparse"] = f["sparseh"] = np.full(n3, -1.)
            f["topless"] = f32exact(np.where(late[None], f["topless"], -1.))
            f["toplessh"] = f32exact(np.where(late[None], f["toplessh"], -1.))
        # for the fluxes, drawn last so that the fields above keep their values: an eddy viscosity and the two boundary fluxes
        f["ev"] = f32exact(0.05 + rs.random_sample(n3))
        f["fbot"] = f32exact(rs.random_sample(n2) - 0.5)
        f["ftop"] = f32exact(rs.random_sample(n2) - 0.5)
        self.f = f

    def digest(self):
        return refshim.digest(*[np.asarray(self.f[k], dtype=np.float64) for k in sorted(self.f)])

    def host(self, g):
        """Host arrays of grid g's dtype and layout; horizontal ghost cells hold 777, which no kernel may read into a result."""
        t, out = g.np_dtype, {}
        for k, a in self.f.items():
            if a.ndim == 3:
                o = np.full(g.shape3, 777., dtype=t)
                o[:, g.jstart:g.jend, g.istart:g.iend] = a
            elif a.ndim == 2:
                o = np.full(g.shape2, 777., dtype=t)
                o[g.jstart:g.jend, g.istart:g.iend] = a
            else:
                o = np.ascontiguousarray(a, dtype=t)
            out[k] = o
        return out


class ExactCase(StatCase):
    """Variables of multiples of 1/4 in [-1, 1) on 16 x 8 columns and 8 levels of depth 16: n = 128, so under the default mask a mean
    is a multiple of 2^-9, a deviation an integer below 2^10 times 2^-9, its fourth power below 2^40 units and a level's sum of them
    below 2^47 < 2^53; dzhi = 1/16, rho*dz = 8. Every partial sum is exact in any order, so every profile has the reference's bits."""

    def __init__(self):
        shape = (16, 8, 8)
        self.shape, self.kind, self.key = shape, "exact", "16x8x8-exact"
        itot, jtot, ktot = shape
        rs = np.random.RandomState(424242)
        n3, n2 = (ktot + 2, jtot, itot), (jtot, itot)
        q4 = lambda n, lo, hi: (rs.randint(lo*4, hi*4, size=n)/4.).astype(np.float64)      # noqa: E731
        f = {"a": q4(n3, -1, 1), "wh": q4(n3, -1, 1), "q": np.where(rs.random_sample(n3) < 0.3, 0.25, 0.), "bot": q4(n2, -2, 2),
             "rho": np.full(ktot + 2, 0.5)}
        for h in ("", "h"):
            f["sparse" + h] = q4(n3, -2, 2); f["topless" + h] = q4(n3, -2, 2)
        f["sparse_bot"] = q4(n2, -2, 2); f["topless_bot"] = q4(n2, -2, 2)
        self.f = f


_cases = {}
EXACT = ((16, 8, 8), (1, 1, 1))
QUIRK = (SHAPES[1], (1, 1, 1))


def case_of(shape, kind="seeded"):
    if (shape, kind) not in _cases:
        _cases[(shape, kind)] = ExactCase() if kind == "exact" else StatCase(shape, kind)
    return _cases[(shape, kind)]


def case_grid(shape, gc, dtype, kind):
    if kind == "exact":
        return grid_of(shape, gc, dtype, zsize=128., stretched=False)
    return grid_of(shape, gc, dtype)


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci, cd, cu = C.c_void_p, C.c_int, C.c_double, C.c_uint
    DP = C.POINTER(Dims)
    lib.ref_stats_thres.argtypes = [ci, DP, ci, vp, vp, cu, cu, vp, vp, vp, cd]; lib.ref_stats_thres.restype = None
    lib.ref_stats_counts.argtypes = [ci, DP, ci, vp, vp, cu, cu, vp, vp, vp, vp, vp]; lib.ref_stats_counts.restype = None
    lib.ref_stats_prof.argtypes = [ci, DP, ci, vp, vp, vp, cd, cd, vp, cu, vp]; lib.ref_stats_prof.restype = None
    lib.ref_stats_columns.argtypes = [ci, DP, vp, vp, vp, vp, cd, cd, vp, cu, vp]; lib.ref_stats_columns.restype = None
    lib.ref_stats_mean_2d.argtypes = [ci, DP, ci, ci, vp, cd]; lib.ref_stats_mean_2d.restype = cd
    lib.ref_stats_ql_h.argtypes = [ci, DP, vp, vp, vp, vp]; lib.ref_stats_ql_h.restype = None
    lib.ref_stats_flux_advec_2.argtypes = [ci, DP, ci, vp, vp, vp]; lib.ref_stats_flux_advec_2.restype = None
    lib.ref_stats_flux_advec_2i5.argtypes = [ci, DP, ci, vp, vp, vp]; lib.ref_stats_flux_advec_2i5.restype = None
    lib.ref_stats_flux_diff_2.argtypes = [ci, DP, vp, vp, cd, vp]; lib.ref_stats_flux_diff_2.restype = None
    lib.ref_stats_flux_diff_smag2.argtypes = [ci, DP, ci, ci, vp, vp, vp, vp, vp, vp, cd, vp, cd, cd]; lib.ref_stats_flux_diff_smag2.restype = None


shim = refshim.Shim("stats", ["ref_stats_shim.cpp", "ref_stats_qlh_shim.cpp"] +
                    ["ref_stats_flux_%s_shim.cpp" % n for n in ("advec_2", "advec_2i5", "diff_2", "diff_smag2")], _bind,
                    defines=refshim.NC_FILL, stubs=True)


def ref_ql_h(g, thl, qt, prefh):
    """calc_liquid_water_h (src/thermo_moist.cxx:368-411) on host arrays of grid g: ql_h over a zero field."""
    out = np.zeros(g.shape3, dtype=g.np_dtype)
    d = dims_of(g)
    shim().ref_stats_ql_h(code(g.np_dtype), C.byref(d), cm.ptr(out), cm.ptr(np.ascontiguousarray(thl)), cm.ptr(np.ascontiguousarray(qt)),
                          cm.ptr(np.ascontiguousarray(prefh)))
    return out


def cyclic(a, g):
    """The periodic fill of the horizontal ghost cells of a 2-D or 3-D array of grid g (Boundary_cyclic::exec / exec_2d)."""
    inner = a[..., g.jstart:g.jend, g.istart:g.iend]
    pad = [(0, 0)]*(a.ndim - 2) + [(g.jgc, g.jgc), (g.igc, g.igc)]
    out = np.ascontiguousarray(np.pad(inner, pad, mode="wrap"))
    if g.jtot == 1 and a.ndim == 3:
        # the single row is replicated over the y ghosts on the interior levels only (src/boundary_cyclic.cxx); on the vertical
        # ghost levels the ghost rows keep what they held, filled east-west from themselves
        ew = np.pad(a[..., g.istart:g.iend], [(0, 0), (0, 0), (g.igc, g.igc)], mode="wrap")
        for k in list(range(g.kstart)) + list(range(g.kend, g.kcells)):
            out[k, :g.jstart], out[k, g.jend:] = ew[k, :g.jstart], ew[k, g.jend:]
    return out


def thresholds(kind):
    """(mask, fld, fldh, fld_bot, threshold, mode) in the order applied. The quirk case's `sparse` is mode Min with threshold -2 over a
    field of -1: every value is above the threshold, so every cell leaves: a mask without a column."""
    if kind == "quirk":
        return [("sparse", "sparse", "sparseh", "sparse_bot", -2., S.MIN), ("topless", "topless", "toplessh", "topless_bot", 0., S.PLUS)]
    return [("sparse", "sparse", "sparseh", "sparse_bot", 0., S.PLUS), ("topless", "topless", "toplessh", "topless_bot", 0., S.PLUS)]


def term_scale(h, g, var, op, off, mean, mfield, flag, nmask):
    """S_k of the bound: the masked mean of |term| per level in float64, the term being what the reference's loop adds (the argument
    of a power in the dtype, as there). It only sets the scale of the bound."""
    t = g.np_dtype
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    out = np.zeros(g.kcells)
    for k in range(g.kstart, g.kend + 1):
        v = h[var][k, js, ie]
        if op == "mean":
            term = v.astype(np.float64)
        elif op == "grad":
            term = (v - h[var][k-1, js, ie]).astype(t).astype(np.float64)*float(g.dzhi[k])
        else:
            with np.errstate(over="ignore"):
                term = ((v - mean[k]).astype(t) + t.type(off)).astype(t).astype(np.float64)**int(op)
        m = (mfield[k, js, ie] & flag) != 0
        out[k] = np.abs(term[m]).sum()/max(int(nmask[k]), 1)
    return out


def bound(g, want, scale):
    """|got - want| <= 4 n 2^-53 S_k + one ulp of the dtype at want: two double sums of the same n terms in different orders each lie
    within (n-1) 2^-53 sum|t| of the exact sum; the factor leaves room for a power that differs by an ulp or two per term."""
    n = g.itot*g.jtot
    return 4.*n*2.**-53*scale + np.spacing(np.abs(want).astype(g.np_dtype)).astype(np.float64)


def grad_2nd(fld, dzhi, mfield, flag, nmask, g):
    """calc_grad_2nd (src/stats.cxx:2171-2195) restated: double(in_mask) * (data[k] - data[k-1]) * dzhi[k], the difference in the
    dtype, summed in float64 in row order; prof[k] = tmp / nmask[k], narrowed. Levels kstart .. kend."""
    t = g.np_dtype
    prof = np.zeros(g.kcells, dtype=t)
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    for k in range(g.kstart, g.kend + 1):
        if nmask[k]:
            m = ((mfield[k, js, ie] & flag) != 0).astype(np.float64)
            term = m * (fld[k, js, ie] - fld[k-1, js, ie]).astype(t).astype(np.float64) * np.float64(dzhi[k])
            prof[k] = t.type(np.cumsum(term.reshape(-1))[-1] / nmask[k])
    prof[np.asarray(nmask) == 0] = S.fill_value(t)
    return prof


def ref_case(shape, gc, dtype, kind="seeded"):
    """Everything the reference gives on one case: {key: array}."""
    lib = shim()
    c, g = case_of(shape, kind), case_grid(shape, gc, dtype, kind)
    h, d, cd = c.host(g), dims_of(g), code(dtype)
    t = g.np_dtype
    nm = len(MASKS)
    out = {}
    flagmax = np.uint32(sum(int(f) for n in range(nm) for f in flags(n)))
    mf, mb = np.full(g.shape3, flagmax, dtype=np.uint32), np.full(g.shape2, flagmax, dtype=np.uint32)
    for n, (mask, fld, fldh, bot, thr, mode) in enumerate(thresholds(kind)):
        fl, flh = flags(MASKS.index(mask))
        lib.ref_stats_thres(cd, C.byref(d), mode, cm.ptr(mf), cm.ptr(mb), int(fl), int(flh), cm.ptr(h[fld]), cm.ptr(h[fldh]), cm.ptr(h[bot]), thr)
        out["mfield%d" % (n + 1)], out["mfield_bot%d" % (n + 1)] = mf.astype(np.uint8), mb.astype(np.uint8)
    mf, mb = cyclic(mf, g), cyclic(mb, g)
    out["mfield"], out["mfield_bot"] = mf.astype(np.uint8), mb.astype(np.uint8)
    nmask = np.zeros((nm, 2, g.kcells), dtype=np.int32)
    nbot = np.zeros(nm, dtype=np.int32)
    area, areah = np.zeros((nm, g.kcells), dtype=t), np.zeros((nm, g.kcells), dtype=t)
    for n in range(nm):
        fl, flh = flags(n)
        lib.ref_stats_counts(cd, C.byref(d), g.itot*g.jtot, cm.ptr(mf), cm.ptr(mb), int(fl), int(flh), cm.ptr(nmask[n, 0]), cm.ptr(nmask[n, 1]),
                             cm.ptr(nbot[n:n+1]), cm.ptr(area[n]), cm.ptr(areah[n]))
    out.update(nmask=nmask, nmask_bot=nbot, area=area, areah=areah)
    for var, loc, off, thr, ops in VARS:
        for op in ops:
            if op in S.COLUMN:
                continue
            p = np.zeros((nm, g.kcells), dtype=t)
            for n in range(nm):
                half = (1 - loc) if op == "grad" else loc
                flag, nmk = flags(n)[half], nmask[n, half]
                if op == "grad":
                    p[n] = grad_2nd(h[var], g.dzhi, mf, flag, nmk, g)
                else:
                    mean = out[var][n] if op in ("2", "3", "4") else None
                    lib.ref_stats_prof(cd, C.byref(d), OPCODE[op], cm.ptr(p[n]), cm.ptr(h[var]), None if mean is None else cm.ptr(mean), off, thr,
                                       cm.ptr(mf), int(flag), cm.ptr(nmk))
            out[S.prof_name(var, op)] = p
        if any(op in S.COLUMN for op in ops):
            col = np.zeros((nm, 4), dtype=t)
            for n in range(nm):
                lib.ref_stats_columns(cd, C.byref(d), cm.ptr(col[n]), cm.ptr(h[var]), cm.ptr(g.dz), cm.ptr(h["rho"]), off, thr, cm.ptr(mf),
                                      int(flags(n)[loc]), cm.ptr(nmask[n, loc]))
            out[var + "_columns"] = col
    out["bot"] = np.array([lib.ref_stats_mean_2d(cd, C.byref(d), g.itot, g.jtot, cm.ptr(h["bot"]), BOT_OFFSET)])
    if kind == "seeded":
        out.update(ref_fluxes(shape, gc, dtype, out))
    return out



# ---- the fluxes --------------------------------------------------------------------------------------------------------------
ADVEC_2, ADVEC_2I5, DIFF_2, DIFF_SMAG2 = 2, 25, 2, 22
VISC, TPR = 1.e-2, 1./3.
FLUX_VAR, FLUX_OFF = "a", 0.5                      # VARS[0]: a full-level variable with an offset, taken as a scalar, as u and as v
# (advection scheme, kind, limited) and (diffusion scheme, kind, surface model) of every flux held against the reference
W_CASES = [(ADVEC_2, 0, 0), (ADVEC_2, 1, 0), (ADVEC_2, 2, 0), (ADVEC_2I5, 0, 0), (ADVEC_2I5, 1, 0), (ADVEC_2I5, 2, 0), (ADVEC_2I5, 0, 1)]
D_CASES = [(DIFF_2, 0, 0)] + [(DIFF_SMAG2, kind, sm) for sm in (0, 1) for kind in (0, 1, 2)]
SUM_CASE = (W_CASES[4], D_CASES[5])                # _flux of a u-like variable: advec_2i5 and smag2 with a surface model


def w_key(c):
    return "w-%d-%d-%d" % c


def d_key(c):
    return "diff-%d-%d-%d" % c


def flux_host(c, g):
    """The host arrays of the flux tests: the variable, w, evisc with their horizontal ghost cells filled periodically (u and v
    read a neighbour), the boundary fluxes."""
    h = c.host(g)
    return {"a": cyclic(h["a"], g), "wh": cyclic(h["wh"], g), "ev": cyclic(h["ev"], g), "fbot": h["fbot"], "ftop": h["ftop"]}


def ref_flux_fields(g, h, mean, wmean):
    """The reference's flux FIELDS of one mask: {key: [kcells][jcells][icells]}. fld' and w' are subtract_mean's (stats.cxx:514-535,
    a subtraction in the dtype, restated here) over zero-filled tmp fields: fld' on kstart .. kend-1, w' on kstart .. kend."""
    lib, t, d, cd_ = shim(), g.np_dtype, dims_of(g), code(g.np_dtype)
    ks, ke = g.kstart, g.kend
    ap, wp = np.zeros(g.shape3, dtype=t), np.zeros(g.shape3, dtype=t)
    with np.errstate(over="ignore", invalid="ignore"):
        ap[ks:ke] = h["a"][ks:ke] - mean[ks:ke, None, None]
        wp[ks:ke+1] = h["wh"][ks:ke+1] - wmean[ks:ke+1, None, None]
    out = {}
    for c in W_CASES:
        st = np.zeros(g.shape3, dtype=t)
        fn = lib.ref_stats_flux_advec_2 if c[0] == ADVEC_2 else lib.ref_stats_flux_advec_2i5
        fn(cd_, C.byref(d), 3 if c[2] else c[1], cm.ptr(st), cm.ptr(ap), cm.ptr(wp))
        out[w_key(c)] = st
    for c in D_CASES:
        st = np.zeros(g.shape3, dtype=t)
        if c[0] == DIFF_2:
            lib.ref_stats_flux_diff_2(cd_, C.byref(d), cm.ptr(st), cm.ptr(h["a"]), VISC, cm.ptr(g.dzhi))
        else:
            di = float(t.type(1./float(t.type(g.dx if c[1] == 1 else g.dy))))            # gd.dxi = 1./gd.dx (src/grid.cxx:244)
            lib.ref_stats_flux_diff_smag2(cd_, C.byref(d), c[1], c[2], cm.ptr(st), cm.ptr(h["a"]), cm.ptr(h["wh"]), cm.ptr(h["ev"]), cm.ptr(h["fbot"]),
                                          cm.ptr(h["ftop"]), di, cm.ptr(g.dzhi), TPR, VISC)
        out[d_key(c)] = st
    return out


def ref_fluxes(shape, gc, dtype, base):
    """The flux profiles [nmasks][kcells] of the reference, calc_mean of the flux field under flagh (:1717-1727, :1746-1756) and
    add_fluxes (:400-407); base holds the case's mfield, nmask and the means of the variable and of w. Also the scale S_k of the
    bound, the masked mean of |flux| per level."""
    lib = shim()
    c, g = case_of(shape), grid_of(shape, gc, dtype)
    h, d, cd_, t = flux_host(c, g), dims_of(g), code(dtype), g.np_dtype
    nm = len(MASKS)
    mf = np.ascontiguousarray(base["mfield"].astype(np.uint32))
    out = {}
    for n in range(nm):
        flagh, nmh = flags(n)[1], np.ascontiguousarray(base["nmask"][n, 1])
        fields = ref_flux_fields(g, h, base[FLUX_VAR][n], base["wh"][n])
        for key, st in fields.items():
            p = np.zeros(g.kcells, dtype=t)
            lib.ref_stats_prof(cd_, C.byref(d), 0, cm.ptr(p), cm.ptr(st), None, 0., 0., cm.ptr(mf), int(flagh), cm.ptr(nmh))
            out.setdefault(FLUX_VAR + "_" + key, np.zeros((nm, g.kcells), dtype=t))[n] = p
            m = (mf[:, g.jstart:g.jend, g.istart:g.iend] & flagh) != 0
            with np.errstate(over="ignore", invalid="ignore"):
                sc = (np.abs(st[:, g.jstart:g.jend, g.istart:g.iend].astype(np.float64))*m).sum(axis=(1, 2))/np.maximum(nmh, 1)
            out.setdefault("scale_" + key, np.zeros((nm, g.kcells)))[n] = sc
    wk, dk = FLUX_VAR + "_" + w_key(SUM_CASE[0]), FLUX_VAR + "_" + d_key(SUM_CASE[1])
    tot = np.zeros((nm, g.kcells), dtype=t)
    with np.errstate(over="ignore", invalid="ignore"):
        tot[:, g.kstart:g.kend+1] = out[wk][:, g.kstart:g.kend+1] + out[dk][:, g.kstart:g.kend+1]
    tot[base["nmask"][:, 1] == 0] = S.fill_value(t)
    out[FLUX_VAR + "_flux"] = tot
    return out


def flux_excluded(g, nmask):
    """The (mask, level) pairs of _w and _flux left out of the numeric comparison: the reference subtracts the fill value as the
    mean of a level whose (full-level) mask is empty, so a flux level whose stencil k-3 .. k+2 touches such a level means nothing."""
    ex = np.zeros((len(MASKS), g.kcells), dtype=bool)
    for n in range(len(MASKS)):
        for k in range(g.kstart, g.kend + 1):
            ex[n, k] = any(g.kstart <= kl < g.kend and nmask[n, 0, kl] == 0 for kl in range(k - 3, k + 3))
    return ex


def all_cases():
    return [(s, gc, "seeded") for s, gc in LAYOUTS] + [EXACT + ("exact",), QUIRK + ("quirk",)]


def case_key(shape, gc, dtype, kind):
    return "%s/%d%d%d/%s/" % (case_of(shape, kind).key, gc[0], gc[1], gc[2], tag(dtype))


def _compute_all():
    rec = {}
    for shape, gc, kind in all_cases():
        for dt in cm.DTYPES:
            r = ref_case(shape, gc, dt, kind)
            for k, v in r.items():
                if k.startswith("mfield") and dt != cm.DTYPES[0]:
                    continue                   # the thresholds see values a float holds exactly: the same words in both dtypes
                rec[case_key(shape, gc, dt, kind) + k] = v
        rec["digest/%s" % case_of(shape, kind).key] = np.array(case_of(shape, kind).digest())
    return rec


GOLD = refshim.Golden("stats", _compute_all, "tests/test_stats_masks.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(shape, gc, dtype, kind, name, be=None):
    """A reference result by name (Golden.ref); the mask words are stored once, under the first dtype."""
    return GOLD.ref(case_key(shape, gc, cm.DTYPES[0] if name.startswith("mfield") else dtype, kind) + name, be)


# ---- the device -------------------------------------------------------------------------------------------------------------
class Dev:
    """The arrays of one case on a backend, as torch tensors (CPU tensors for the emulation), and a Sampler over them."""

    def __init__(self, be, shape, gc, dtype, kind="seeded"):
        import torch
        self.be, self.torch = be, torch
        self.c, self.g = case_of(shape, kind), case_grid(shape, gc, dtype, kind)
        self.kind = kind
        self.h = self.c.host(self.g)
        self.device = torch.device("cpu") if be.name == "emul" else be.dev
        self.G = be.grid(self.g)
        self.d = {k: torch.from_numpy(v.copy()).to(self.device) for k, v in self.h.items()}
        self.s = S.Sampler(be.lib, self.g, self.G, torch, self.device, MASKS, stream=lambda: be.stream)

    def masks(self, stages=None):
        """initialize, the thresholds, finalize; stages (a list) receives the words after init and after every threshold."""
        s = self.s
        s.initialize_masks()
        if stages is not None:
            stages.append(s.host_words())
        for mask, fld, fldh, bot, thr, mode in thresholds(self.kind):
            s.set_mask_thres(mask, self.d[fld], self.d[fldh], self.d[bot], thr, mode)
            if stages is not None:
                stages.append(s.host_words())
        s.finalize_masks()
        self.be.sync()

    def tensor(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
