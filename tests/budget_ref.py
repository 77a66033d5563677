"""Shared plumbing of the budget tests (tests/test_budget_*.py): the seeded cases and their reference results.

The reference is the reference's OWN translation unit (src/budget_2.cxx) behind tests/cpp/ref_budget_2_shim.cpp, compiled into a
temporary directory with the command tests/stats_ref.py uses for its shims, where the reference tree exists. Where it is absent the
same cases read tests/golden/budget_ref.npz, recorded with MHH_RECORD_BUDGET_GOLDEN=1 python -m pytest tests/test_budget_terms.py:
profiles, scales and counts only, no 3-D field. The masks, their counts, calc_mean and the fill value come from stats_ref's shim.
Every calc_* call gets zero-filled output fields and, per mask, model profiles that started from zero, so a level that a loop does
not write and a model-profile level without a cell are 0. Grid::interpolate_2nd (wx, wy) is a member of Grid<TF> that cannot be
reached without an object: one expression, restated here in float64 (what its double literals make of it) and narrowed once.
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
import stats_ref as R
from refshim import Dims, code, dims_of, f32exact, tag
from microhh_amd import budget as B
from microhh_amd import stats as S

MASKS = R.MASKS
# (shape, ghost cells, kind): the second ghost layout; 37 rows make two row chunks, the second partial; the exact fixture
LAYOUTS = [((17, 9, 8), (2, 2, 1), "seeded"), ((17, 9, 8), (3, 3, 1), "seeded"), ((24, 37, 8), (2, 2, 1), "seeded")]
EXACT = ((16, 8, 8), (2, 2, 1), "exact")
# every group that is built, in the order of the bits, with its profiles in the library's order
GROUPS = {0: ("ke", "tke"), 1: ("u2_shear", "v2_shear", "tke_shear", "uw_shear", "vw_shear"),
          2: ("u2_turb", "v2_turb", "w2_turb", "tke_turb", "uw_turb", "vw_turb"), 3: ("u2_cor", "v2_cor", "uw_cor", "vw_cor"),
          4: ("w2_pres", "tke_pres", "uw_pres", "vw_pres"), 5: ("u2_rdstr", "v2_rdstr", "w2_rdstr", "uw_rdstr", "vw_rdstr"),
          6: ("u2_diff", "v2_diff", "w2_diff", "tke_diff", "uw_diff", "vw_diff"),
          7: ("w2_buoy", "tke_buoy", "uw_buoy", "vw_buoy"), 8: ("bw_buoy",), 9: ("b2_shear", "b2_turb", "bw_shear", "bw_turb"),
          10: ("bw_pres", "bw_rdstr")}
ALL = sum(1 << G for G in GROUPS)
CUBES = ("tke_turb", "w2_turb")
FIELDS = ("u", "v", "w", "p", "evisc", "b")
PARAMS = {"seeded": dict(utrans=1.5, vtrans=-0.75, fc=1.e-4), "exact": dict(utrans=0.25, vtrans=-0.5, fc=0.25)}


def grid_of(shape, gc, dtype, kind):
    if kind == "exact":
        # dx = dy = 4, dz = 16: dxi, dyi, dzi, dzhi are powers of two
        from microhh_amd.grid import Grid
        return Grid(shape[0], shape[1], shape[2], 4.*shape[0], 4.*shape[1], 16.*shape[2], order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype)
    return R.grid_of(shape, gc, dtype)


class BudgetCase:
    """u, v, w, p, evisc, b on ktot + 2 levels of jtot x itot columns and the two surface fluxes, beside the StatCase of the shape
    (the thresholded fields of the masks). exact: multiples of 1/4 whose sum over every level is a multiple of itot*jtot/4 (a few
    cells of a level are moved by 1/4), so that the default mask's means are multiples of 1/4 and every term, partial sum and
    profile is exact in both dtypes."""

    def __init__(self, shape, kind):
        self.shape, self.kind = shape, kind
        self.stat = R.case_of(shape, kind)
        self.key = "%dx%dx%d-%s" % (shape + (kind,))
        itot, jtot, ktot = shape
        rs = np.random.RandomState(9100 + itot + 7*ktot + 131*jtot)
        n3, n2 = (ktot + 2, jtot, itot), (jtot, itot)
        lev = np.arange(ktot + 2)[:, None, None]
        f = {}
        if kind == "exact":
            def q4(n, lo, hi):
                a = rs.randint(lo*4, hi*4, size=n).astype(np.int64)
                if len(n) == 3:
                    for k in range(n[0]):
                        r = int(a[k].sum()) % (n[1]*n[2])
                        a[k].reshape(-1)[:r] -= 1                  # the level's sum becomes a multiple of the number of columns
                return a/4.
            for n in ("u", "v", "w", "b"):
                f[n] = q4(n3, -1, 1)
            f["p"] = q4(n3, -2, 2)
            f["evisc"] = (rs.randint(1, 8, size=n3)/4.).astype(np.float64)
            f["u_fluxbot"], f["v_fluxbot"] = q4(n2, -1, 1), q4(n2, -1, 1)
        else:
            f["u"] = f32exact(2. + 0.3*lev + (rs.random_sample(n3) - 0.5))
            f["v"] = f32exact(-1. + 0.2*lev + (rs.random_sample(n3) - 0.5))
            f["w"] = f32exact(rs.random_sample(n3) - 0.5)
            f["p"] = f32exact(5.*(rs.random_sample(n3) - 0.5))
            f["evisc"] = f32exact(0.05 + rs.random_sample(n3))
            f["b"] = f32exact(0.1*lev + 0.5*(rs.random_sample(n3) - 0.5))
            f["u_fluxbot"] = f32exact(0.1*(rs.random_sample(n2) - 0.5))
            f["v_fluxbot"] = f32exact(0.1*(rs.random_sample(n2) - 0.5))
        self.f = f

    def digest(self):
        return refshim.digest(*[np.asarray(self.f[k], dtype=np.float64) for k in sorted(self.f)])

    def host(self, g):
        """Host arrays of grid g's dtype and layout with the horizontal ghost cells filled periodically."""
        t, out = g.np_dtype, {}
        for k, a in self.f.items():
            o = np.zeros(g.shape3 if a.ndim == 3 else g.shape2, dtype=t)
            o[..., g.jstart:g.jend, g.istart:g.iend] = a
            out[k] = R.cyclic(o, g)
        return out


_cases = {}


def case_of(shape, kind):
    if (shape, kind) not in _cases:
        _cases[(shape, kind)] = BudgetCase(shape, kind)
    return _cases[(shape, kind)]


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    VPP = C.POINTER(C.c_void_p)
    lib.ref_budget_2_group.argtypes = [C.c_int, C.POINTER(Dims), C.c_int, VPP, VPP, VPP, C.POINTER(C.c_double)]
    lib.ref_budget_2_group.restype = None


shim = refshim.Shim("budget_2", ["ref_budget_2_shim.cpp"], _bind, defines=refshim.NC_FILL, stubs=True)


def _ptrs(arrays):
    return (C.c_void_p*len(arrays))(*[cm.ptr(a).value if a is not None else None for a in arrays])


def interp_w(w, g, axis):
    """Grid::interpolate_2nd (src/grid.cxx:455-486) of w to the location of u (axis 2) or v (axis 1) on the interior columns of all
    levels: the four quarter terms in float64, narrowed once."""
    w64 = w.astype(np.float64)
    sh = np.roll(w64, 1, axis=axis)
    if axis == 2:
        q = 0.25*(0.5*w64 + 0.5*sh)
        o = q + q + q + q
    else:
        a, b = 0.25*(0.5*w64 + 0.5*w64), 0.25*(0.5*sh + 0.5*sh)
        o = a + b + a + b
    out = np.zeros(g.shape3, dtype=g.np_dtype)
    out[:, g.jstart:g.jend, g.istart:g.iend] = o[:, g.jstart:g.jend, g.istart:g.iend].astype(g.np_dtype)
    return out


def ref_masks(c, g):
    """The mask words after the thresholds and the cyclic fill, and nmask[mask][2][kcells], as stats_ref.ref_case makes them."""
    lib, h, d, cd = R.shim(), c.stat.host(g), dims_of(g), code(g.np_dtype)
    nm = len(MASKS)
    flagmax = np.uint32(sum(int(f) for n in range(nm) for f in R.flags(n)))
    mf, mb = np.full(g.shape3, flagmax, dtype=np.uint32), np.full(g.shape2, flagmax, dtype=np.uint32)
    for mask, fld, fldh, bot, thr, mode in R.thresholds(c.kind):
        fl, flh = R.flags(MASKS.index(mask))
        lib.ref_stats_thres(cd, C.byref(d), mode, cm.ptr(mf), cm.ptr(mb), int(fl), int(flh), cm.ptr(h[fld]), cm.ptr(h[fldh]), cm.ptr(h[bot]), thr)
    mf, mb = R.cyclic(mf, g), R.cyclic(mb, g)
    nmask = np.zeros((nm, 2, g.kcells), dtype=np.int32)
    nbot = np.zeros(1, dtype=np.int32)
    t = g.np_dtype
    for n in range(nm):
        fl, flh = R.flags(n)
        lib.ref_stats_counts(cd, C.byref(d), g.itot*g.jtot, cm.ptr(mf), cm.ptr(mb), int(fl), int(flh), cm.ptr(nmask[n, 0]), cm.ptr(nmask[n, 1]),
                             cm.ptr(nbot), cm.ptr(np.zeros(g.kcells, dtype=t)), cm.ptr(np.zeros(g.kcells, dtype=t)))
    return mf, nmask


def mean_all(g, fld, mf, flag, nmk):
    """calc_mean over 0 .. kcells-1 (Stats::calc_mask_mean_profile, src/stats.cxx:1328-1347) into a zeroed profile: a level
    without a cell keeps 0."""
    d = dims_of(g)
    d.kstart, d.kend = 0, g.kcells - 1
    p = np.zeros(g.kcells, dtype=g.np_dtype)
    R.shim().ref_stats_prof(code(g.np_dtype), C.byref(d), 0, cm.ptr(p), cm.ptr(fld), None, 0., 0., cm.ptr(mf), int(flag), cm.ptr(np.ascontiguousarray(nmk)))
    p[np.asarray(nmk) == 0] = 0
    return p


def cube_scale(g, h, wm, k):
    """The sum of the absolute cube addends of tke_turb and w2_turb times their metric at level k, per cell, in float64."""
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    w = h["w"].astype(np.float64)
    wm = wm.astype(np.float64)
    ks, ke = g.kstart, g.kend
    z = np.zeros((g.jmax, g.imax))
    dev = lambda kl: w[kl, js, ie] - wm[kl]      # noqa: E731
    tke = 0.5*(np.abs(dev(k+1))**3 + np.abs(dev(k))**3)*float(g.dzi[k]) if k < ke else z
    if k == ks:
        w2 = 2.*np.abs(0.5*(w[k, js, ie] + w[k+1, js, ie]))**3*float(g.dzhi[k])
    elif k == ke:
        w2 = 2.*np.abs(0.5*(dev(k) + dev(k-1)))**3*float(g.dzhi[k])
    else:
        w2 = (np.abs(0.5*(dev(k) + dev(k+1)))**3 + np.abs(0.5*(dev(k) + w[k-1, js, ie]))**3)*float(g.dzhi[k])
    return {"tke_turb": tke, "w2_turb": w2}


def term_fields(g, h, um, vm, wm, bmean, pmean, par, groups=None):
    """The reference's term FIELDS of one mask over zero-filled tmp fields: yields (name, [kcells][jcells][icells]). h: host arrays
    u, v, w, p, evisc, b, u_fluxbot, v_fluxbot of grid g with their cyclic ghost cells; the profiles of the grid's dtype."""
    lib, t, d, cd = shim(), g.np_dtype, dims_of(g), code(g.np_dtype)
    wx, wy = interp_w(h["w"], g, 2), interp_w(h["w"], g, 1)
    pars = (C.c_double*5)(par["utrans"], par["vtrans"], par["fc"], float(t.type(1.)/t.type(g.dx)), float(t.type(1.)/t.type(g.dy)))
    inp = _ptrs([np.ascontiguousarray(h[n]) for n in ("u", "v", "w", "p", "evisc", "b", "u_fluxbot", "v_fluxbot")] + [wx, wy])
    dzi, dzhi = np.ascontiguousarray(g.dzi, dtype=t), np.ascontiguousarray(g.dzhi, dtype=t)
    prof = _ptrs([np.ascontiguousarray(a, dtype=t) for a in (um, vm, wm, bmean, pmean)] + [dzi, dzhi])
    for G, names in GROUPS.items():
        if groups is not None and not (groups >> G) & 1:
            continue
        flds = [np.zeros(g.shape3, dtype=t) for _ in range(len(names) + (2 if G == 6 else 0))]      # the LES group: wz, evisch
        lib.ref_budget_2_group(cd, C.byref(d), G, _ptrs(flds), inp, prof, pars)
        for name, fld in zip(names, flds):
            yield name, fld


def ref_case(shape, gc, dtype, kind):
    """Everything the reference gives on one case: {key: array}."""
    c, g = case_of(shape, kind), grid_of(shape, gc, dtype, kind)
    h, d, cd, t = c.host(g), dims_of(g), code(dtype), g.np_dtype
    nm, kc = len(MASKS), g.kcells
    js, ie = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    mf, nmask = ref_masks(c, g)
    out = {"nmask": nmask}
    ones = np.ones(g.shape3, dtype=np.uint32)
    nall = np.full(kc, g.itot*g.jtot, dtype=np.int32)
    # field3d_operators.calc_mean_profile (src/field3d_operators.cxx:45-66): the same loop as calc_mean with every cell in the mask
    out["bmean"], out["pmean"] = mean_all(g, h["b"], ones, 1, nall), mean_all(g, h["p"], ones, 1, nall)
    for n in ("umodel", "vmodel", "wmodel"):
        out[n] = np.zeros((nm, kc), dtype=t)
    for names in GROUPS.values():
        for name in names:
            out[name], out["scale_" + name] = np.zeros((nm, kc), dtype=t), np.zeros((nm, kc))
    for name in CUBES:
        out["cube_" + name] = np.zeros((nm, kc))
    for n in range(nm):
        fl, flh = R.flags(n)
        nmk = np.ascontiguousarray(nmask[n, 0])
        um, vm = mean_all(g, h["u"], mf, fl, nmask[n, 0]), mean_all(g, h["v"], mf, fl, nmask[n, 0])
        wm = mean_all(g, h["w"], mf, flh, nmask[n, 1])
        out["umodel"][n], out["vmodel"][n], out["wmodel"][n] = um, vm, wm
        m = (mf[:, js, ie] & fl) != 0
        cnt = np.maximum(nmk, 1)
        for name, fld in term_fields(g, h, um, vm, wm, out["bmean"], out["pmean"], PARAMS[kind]):
            # calc_mask_stats (src/stats.cxx:1350-1390): calc_mean under the full-level flag over kstart .. kend, then the fill value
            p = np.zeros(kc, dtype=t)
            R.shim().ref_stats_prof(cd, C.byref(d), 0, cm.ptr(p), cm.ptr(fld), None, 0., 0., cm.ptr(mf), int(fl), cm.ptr(nmk))
            out[name][n] = p
            with np.errstate(over="ignore", invalid="ignore"):
                out["scale_" + name][n] = (np.abs(fld[:, js, ie].astype(np.float64))*m).sum(axis=(1, 2))/cnt
        for k in range(g.kstart, g.kend + 1):
            for name, a in cube_scale(g, h, wm, k).items():
                out["cube_" + name][n, k] = (a*m[k]).sum()/cnt[k]
    return out


def all_cases():
    return LAYOUTS + [EXACT]


def case_key(shape, gc, dtype, kind):
    return "%s/%d%d%d/%s/" % (case_of(shape, kind).key, gc[0], gc[1], gc[2], tag(dtype))


def _compute_all():
    rec = {}
    for shape, gc, kind in all_cases():
        for dt in cm.DTYPES:
            for k, v in ref_case(shape, gc, dt, kind).items():
                rec[case_key(shape, gc, dt, kind) + k] = v
        rec["digest/%s" % case_of(shape, kind).key] = np.array(case_of(shape, kind).digest())
    return rec


GOLD = refshim.Golden("budget", _compute_all, "tests/test_budget_terms.py")
RECORD, golden, computed, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.record_if_asked


def ref(shape, gc, dtype, kind, name, be=None):
    """A reference result by name (Golden.ref)."""
    return GOLD.ref(case_key(shape, gc, dtype, kind) + name, be)


def bound(g, want, scale, cube=None):
    """stats_ref.bound; for the two cube terms one part more. The reference's pow(x, 3) is libm's pow, documented within 1 ulp of
    the exact cube (a relative 2^-52 in double); x*x*x rounds twice (2 * 2^-53): the two cubes differ by at most 2^-51 of their size,
    and so does every addend of the term, whose sum of absolute addends times the metric has the masked mean `cube`. In float the term
    is narrowed after that, and two doubles that differ at all may narrow to neighbouring floats: one float ulp of each cell's term,
    at most 2^-23 of its size, the masked mean of which is `scale`."""
    b = R.bound(g, want, scale)
    if cube is not None:
        b = b + 2.**-51*cube + (2.**-23*scale if g.np_dtype == np.float32 else 0.)
    return b


# ---- the device -------------------------------------------------------------------------------------------------------------
class Dev(R.Dev):
    """stats_ref.Dev on the budget cases' grids, with the budget fields beside the thresholded ones and a Budget2Sampler."""

    def __init__(self, be, shape, gc, dtype, kind):
        import torch
        self.be, self.torch = be, torch
        self.bc, self.c, self.g, self.kind = case_of(shape, kind), R.case_of(shape, kind), grid_of(shape, gc, dtype, kind), kind
        self.h = self.c.host(self.g)
        self.hb = self.bc.host(self.g)
        self.device = torch.device("cpu") if be.name == "emul" else be.dev
        self.G = be.grid(self.g)
        self.d = {k: torch.from_numpy(v.copy()).to(self.device) for k, v in self.h.items()}
        self.f = {k: torch.from_numpy(v.copy()).to(self.device) for k, v in self.hb.items()}
        self.s = S.Sampler(be.lib, self.g, self.G, torch, self.device, MASKS, stream=lambda: be.stream)
        self.b = B.Budget2Sampler(self.s)

    def fields(self):
        f = self.f
        return dict(u=f["u"], v=f["v"], w=f["w"], p=f["p"], evisc=f["evisc"], b=f["b"], u_fluxbot=f["u_fluxbot"], v_fluxbot=f["v_fluxbot"])
