"""Shared plumbing of the ice microphysics tests (tests/test_nsw6_*.py): the seeded cases and their reference results.

The reference is the reference's OWN source (src/microphys_nsw6.cxx) behind tests/cpp/ref_nsw6_shim.cpp, compiled into a temporary
directory where the reference tree exists. Where it is absent the same cases read tests/golden/nsw6_ref.npz, recorded with
MHH_RECORD_NSW6_GOLDEN=1 python -m pytest tests/test_nsw6_exec.py: reference OUTPUTS only, of runs that start from zero tendencies.
The inputs are not stored: every draw is numpy's seeded legacy generator, everything derived from a draw uses + - * / only and is
narrowed to values a float holds exactly, so they are the same numbers on every host; the file holds their digest per case.

Two ways to feed ql and qi, as the entry point has them: "given" (seeded arrays of their own, so every branch of conversion depends
on exactly representable inputs) and "sat" (both null: sat_adjust inline; the reference is fed by its own sat_adjust).
"""
import ctypes as C

import numpy as np

import common as cm
import micro_ref as MR
import moist_ref as M
import refshim
from refshim import Dims, code, dims_of, f32exact, have_reference, tag

PBOT = 101480.
NC0 = 100.e6
T0 = 273.15

CONV, SEDI_R, SEDI_S, SEDI_G, ALL = 1, 2, 4, 8, 15
POW, SQRT = 0, 1
SPECIES = ("qr", "qs", "qg")
BOT = ("rr_bot", "rs_bot", "rg_bot")
OUT = ("qrt", "qst", "qgt", "thlt", "qtt")
MASKS = {"conv": CONV, "sedi_r": SEDI_R, "sedi_s": SEDI_S, "sedi_g": SEDI_G, "all": ALL}
WRITES = {CONV: OUT, SEDI_R: ("qrt", "rr_bot"), SEDI_S: ("qst", "rs_bot"), SEDI_G: ("qgt", "rg_bot"), ALL: OUT + BOT}
MODES = ("given", "sat")

# the shapes, grids and ghost layouts of the warm scheme's tests; the 40-level one has rows longer than a wave and, with a CFL number
# above 3, gathers that span several levels
SHAPES = MR.SHAPES
SMALL = MR.SMALL
GCS = MR.GCS
CFLS = {"lo": 0.3, "hi": 3.5}
# the recording step asserts that no cell of a "sat" run lies on a threshold of conversion (near_threshold); where the first seed put
# one there, the next that does not
SEED_BUMP = {(130, 6, 40): 16}
STRIDE = 5          # of the two large shapes the golden file keeps every fifth column in i
grid_of = MR.grid_of


def exp_like(x):
    """(1 + x/32)^32 from + - * / alone: close enough to exp(x) for a realistic saturation humidity, the same bits on every host."""
    y = 1. + x/32.
    for _ in range(5):
        y = y*y
    return y


class IceCase:
    """Deep, mixed-phase inputs of one shape on ktot + 2 levels of jtot x itot columns (the same for every ghost layout): the
    temperature falls from about 293 K at the bottom to about 221 K at the top (the freezing level and the -40 C level both lie
    inside), qt scatters around saturation, ql and qi of their own for the "given" mode, rain, snow and graupel each in about half of
    the columns (a tenth of those in the top level only, a tenth in the bottom level only) between 1e-7 and 2e-3 kg/kg, a few cells
    at or below q_min, a few with 0.3 kg/kg and more (nothing less reaches the upper clamp of the terminal velocity), ghost levels
    that hold precipitation of their own, five non-zero tendencies. (20, 1, 12) carries a density of 60 kg m-3 in its upper levels:
    unphysical on purpose, nothing less reaches the LOWER clamp (with q > q_min and rho ~ 1 no species falls slower than 0.3 m/s)."""

    def __init__(self, shape):
        self.shape = shape
        self.key = "%dx%dx%d" % shape
        itot, jtot, ktot = shape
        rs = np.random.RandomState(9001 + itot + 7*ktot + 1000*SEED_BUMP.get(shape, 0))
        g = grid_of(shape, (1, 1, 1), np.float64)
        n3, n2 = (ktot + 2, jtot, itot), (1, jtot, itot)
        z = g.z.astype(np.float64)
        s = 1. - z/44000.
        self.p = f32exact(PBOT*s*s*s*s*s)
        self.exn = f32exact(M.exn_like(self.p))
        rho = 1.16*(1. - z/22000.)
        if shape == (20, 1, 12):
            rho[-4:] = 60.
        self.rho = f32exact(rho)
        frac = ((z - z[0])/(z[-1] - z[0]))[:, None, None]
        temp = 293. - 72.*frac + 6.*(rs.random_sample(n3) - 0.5)
        self.thl = f32exact(temp/self.exn[:, None, None])
        qs_a = 3.8e-3*exp_like(0.075*(temp - T0))*(1.e5/self.p[:, None, None])
        self.qt = f32exact(qs_a*(0.35 + 1.1*rs.random_sample(n3)))
        # cloud water and ice of the "given" mode: liquid above 233 K, ice below 273 K, some of it below ql_min / qi_min
        cloud = rs.random_sample(n3) < 0.5
        wl = np.clip((temp - 233.)/40., 0., 1.)
        u = rs.random_sample(n3)
        ql = np.where(cloud, wl*1.2e-3*u*u*u, 0.)
        u = rs.random_sample(n3)
        qi = np.where(cloud, (1. - wl)*1.2e-3*u*u*u, 0.)
        ql, qi = f32exact(np.minimum(ql, 0.45*self.qt)), f32exact(np.minimum(qi, 0.45*self.qt))
        all_in = rs.random_sample(n3) < 0.03                 # no vapour left: everything is liquid, or everything is ice
        self.ql = np.where(all_in, np.where(wl > 0.5, self.qt, 0.), ql)
        self.qi = np.where(all_in, np.where(wl > 0.5, 0., self.qt), qi)
        lev = np.arange(ktot + 2)[:, None, None]
        for name in SPECIES:
            kind = rs.random_sample(n2)                      # < 0.5: present; of those < 0.05 top only, < 0.10 bottom only
            wet = (kind < 0.5) & (rs.random_sample(n3) < 0.7)
            wet = np.where(kind < 0.05, lev >= ktot, np.where(kind < 0.10, lev <= 1, wet))
            u = rs.random_sample(n3)
            q = 1.e-7 + 2.e-3*u*u*u*u
            few = rs.random_sample(n3)
            q = np.where(few < 0.02, 1.e-12*few*40., q)                                # 0 < q <= q_min
            q = np.where((few > 0.02) & (few < 0.06), 1.e-12*(1. + 100.*few), q)       # just above q_min: the slowest fall
            q = np.where(few > 0.985, 0.3 + 10.*(few - 0.985), q)                      # the fastest
            setattr(self, name, f32exact(np.where(wet, q, 0.)))
        self.tend0 = {"qrt": f32exact(1.e-7*(rs.random_sample(n3) - 0.5)), "qst": f32exact(1.e-7*(rs.random_sample(n3) - 0.5)),
                      "qgt": f32exact(1.e-7*(rs.random_sample(n3) - 0.5)), "thlt": f32exact(1.e-3*(rs.random_sample(n3) - 0.5)),
                      "qtt": f32exact(1.e-6*(rs.random_sample(n3) - 0.5))}
        dzmin = float(np.min(g.dz[g.kstart:g.kend].astype(np.float64)))
        # 7 m/s: about the largest three-level mean of the fall velocities these fields reach
        self.dt = {name: float(np.float32(cfl*dzmin/7.)) for name, cfl in CFLS.items()}

    def digest(self):
        return refshim.digest(*[getattr(self, n) for n in ("thl", "qt", "ql", "qi") + SPECIES + ("p", "exn", "rho")], *[self.tend0[n] for n in OUT],
                              np.array([self.dt["lo"], self.dt["hi"]]))

    def embed(self, a3, g, fill=777.):
        out = np.full(g.shape3, fill, dtype=g.np_dtype)
        out[:, g.jstart:g.jend, g.istart:g.iend] = a3
        return out

    def inputs(self, g, zero_tend=False):
        """Host arrays of grid g: the seven fields, the five tendencies, the three surface rates and the tables."""
        t = g.np_dtype
        h = {n: self.embed(np.asarray(getattr(self, n), dtype=t), g) for n in ("thl", "qt", "ql", "qi") + SPECIES}
        for n in OUT:
            h[n] = self.embed(np.zeros_like(self.tend0[n], dtype=t) if zero_tend else np.asarray(self.tend0[n], dtype=t), g)
        for n in BOT:
            h[n] = np.full(g.shape2, 555., dtype=t)
        for n in ("rho", "p", "exn"):
            h[n] = np.ascontiguousarray(getattr(self, n), dtype=t)
        return h


_cases = {}


def ice_case(shape):
    if shape not in _cases:
        _cases[shape] = IceCase(shape)
    return _cases[shape]


# ---- the scheme once more, in numpy's float64: what test_inputs_cover_the_branches asserts on -------------------------------------
def diagnose(c, dt):
    """Branch diagnostics of conversion on the interior of case c with ql, qi given, from a float64 transcription of :193-570
    (std::tgamma through math.gamma): T, S_w, S_i, the six has_*, the six limit factors; and the unclamped terminal velocities."""
    from math import gamma as G, pi
    i = (slice(1, -1),)
    k3 = lambda a: a[1:-1, None, None]
    qr, qs, qg, qt, thl, ql, qi = (getattr(c, n)[i] for n in ("qr", "qs", "qg", "qt", "thl", "ql", "qi"))
    rho, p, exn = k3(c.rho), k3(c.p), k3(c.exn)
    Lv, Lf, cp, Rv, Rd = 2.501e6, 3.337e5, 1005., 461.5, 287.04
    Ls, ep = Lv + Lf, Rd/Rv
    T = exn*thl + Lv/cp*ql + Ls/cp*qi
    qv = qt - ql - qi
    has = {"vapor": qv > 1e-7, "liq": ql > 1e-7, "ice": qi > 1e-7, "rain": qr > 1e-12, "snow": qs > 1e-12, "graupel": qg > 1e-12}
    r0 = np.sqrt(c.rho[1]/rho)
    N0 = {"r": 8e6, "s": 3e6, "g": 4e6}; a = {"r": pi*1e3/6, "s": pi*1e2/6, "g": pi*4e2/6}
    cc = {"r": 130., "s": 4.84, "g": 82.5}; d = {"r": .5, "s": .25, "g": .5}
    f1 = {"r": .78, "s": .65, "g": .78}; f2 = {"r": .27, "s": .39, "g": .27}
    q = {"r": qr, "s": qs, "g": qg}
    lam = {x: (a[x]*N0[x]*G(4.)/(rho*(q[x] + 1e-15)))**0.25 for x in "rsg"}
    V = {x: np.where(q[x] > 1e-12, cc[x]*r0*G(4. + d[x])/G(4.)*lam[x]**(-d[x]), 0.) for x in "rsg"}
    W = lambda cond, v: np.where(cond, v, 0.)
    fac = lambda E, x: pi*E*N0[x]*cc[x]*G(3. + d[x])/4.*r0
    P_iacr = W(has["rain"] & has["ice"], pi*pi*8e6*130.*1e3*G(6.5)/(24.*4.19e-13)*r0/lam["r"]**6.5*qi)
    d1 = (qr >= 1e-4)*1.
    P_raci = W(has["rain"] & has["ice"], fac(1., "r")/lam["r"]**3.5*qi)
    P_racw = W(has["liq"] & has["rain"], fac(1., "r")/lam["r"]**3.5*ql)
    P_sacw = W(has["liq"] & has["snow"], fac(1., "s")/lam["s"]**3.25*ql)
    P_saci = W(has["snow"] & has["ice"], fac(1., "s")*np.exp(0.025*(T - T0))/lam["s"]**3.25*qi)
    P_gacw = W(has["graupel"] & has["liq"], fac(1., "g")/lam["g"]**3.5*ql)
    P_gaci = W(has["graupel"] & has["ice"], fac(.1, "g")/lam["g"]**3.5*qi)
    d2 = 1. - ((qr >= 1e-4) | (qs >= 1e-4))
    acc = lambda la, lb: 12./(la**4*lb**3) + 48./(la**5*lb**2) + 120./(la**6*lb)
    P_racs = W(has["rain"] & has["snow"], (1. - d2)*pi*a["s"]*np.abs(V["r"] - V["s"])*3e6*8e6/(4.*rho)*acc(lam["s"], lam["r"]))
    P_sacr = W(has["rain"] & has["snow"], pi*a["r"]*np.abs(V["r"] - V["s"])*3e6*8e6/(4.*rho)*acc(lam["r"], lam["s"]))
    E_gs = np.minimum(1., np.exp(0.09*(T - T0)))
    P_gacr = W(has["graupel"] & has["rain"], pi*a["r"]*np.abs(V["g"] - V["r"])*.1*4e6*8e6/(4.*rho)*acc(lam["r"], lam["g"]))
    P_gacs = W(has["graupel"] & has["snow"], pi*a["s"]*np.abs(V["g"] - V["s"])*E_gs*4e6*3e6/(4.*rho)*acc(lam["s"], lam["g"]))
    beta_1 = np.minimum(6e-3, 6e-3*np.exp(0.06*(T - T0)))
    D_d = 0.146 - 5.964e-2*np.log(NC0*1e-6/2e3)
    with np.errstate(divide="ignore", invalid="ignore"):
        P_raut = W(has["liq"], 16.7/rho*(rho*ql)**2/(5. + 3.66e-2*1e-6*NC0/(D_d*rho*ql)))
    P_saut = W(has["ice"], np.maximum(beta_1*qi, 0.))
    P_gaut = 0.*qs
    x = np.maximum(-75., T - T0)
    co = [6.1121e2, 4.439306727e1, 1.4279398448, 2.6415206946e-2, 3.029174916e-4, 2.1159987257e-6, 7.5015702516e-9, -1.5604873363e-12,
          -9.9726710231e-14, -4.8165754883e-17, 1.3839187032e-18]
    es_l = sum(cf*x**n for n, cf in enumerate(co))
    xi = np.maximum(-100., T - T0)
    es_i = 611.15*np.exp(22.452*xi/(272.55 + xi))
    G_w = 1./(Lv/(2.43e-2*T)*(Lv/(Rv*T) - 1.) + Rv*T/(2.26e-5*es_l))
    G_i = 1./(Ls/(2.43e-2*T)*(Ls/(Rv*T) - 1.) + Rv*T/(2.26e-5*es_i))
    S_w = qv/(ep*es_l/(p - (1. - ep)*es_l)); S_i = qv/(ep*es_i/(p - (1. - ep)*es_i))
    d3 = (S_i <= 1.)*1.
    vent = {x: f1[x]/lam[x]**2 + f2[x]*np.sqrt(cc[x]*r0/1.5e-5)*G(.5*(5. + d[x]))/lam[x]**(.5*(5. + d[x])) for x in "rsg"}
    P_revp = W(has["rain"], -2.*pi*8e6*(np.minimum(S_w, 1.) - 1.)*G_w/rho*vent["r"])
    sdss = 2.*pi*3e6*(S_i - 1.)*G_i/rho*vent["s"]; gdgs = 2.*pi*4e6*(S_i - 1.)*G_i/rho*vent["g"]
    P_sdep, P_gdep = W(has["vapor"], (1. - d3)*sdss), W(has["vapor"], (1. - d3)*gdgs)
    P_ssub, P_gsub = W(has["snow"], -d3*sdss), W(has["graupel"], -d3*gdgs)
    P_smlt = W(has["snow"], 2.*pi*2.43e-2*(T - T0)*3e6/(rho*Lf)*vent["s"] + 4218.*(T - T0)/Lf*(P_sacw + P_sacr))
    P_gmlt = W(has["graupel"], 2.*pi*2.43e-2*(T - T0)*4e6/(rho*Lf)*vent["g"] + 4218.*(T - T0)/Lf*(P_gacw + P_gacr))
    P_gfrz = W(has["rain"], 20.*pi*pi*100.*8e6*1e3/rho*(np.exp(0.66*(T0 - T)) - 1.)/lam["r"]**7)
    mx = {"v": qv/dt, "i": qi/dt, "l": ql/dt, "r": qr/dt, "s": qs/dt, "g": qg/dt}
    lim = lambda t, m: np.maximum(0., np.minimum(t, m))
    Tp = (T >= T0)*1.; Tn = 1. - Tp
    P_iacr_s, P_iacr_g = lim((1. - d1)*P_iacr, mx["r"]), lim(d1*P_iacr, mx["r"])
    P_raci_s, P_raci_g = lim((1. - d1)*P_raci, mx["i"]), lim(d1*P_raci, mx["i"])
    P_sacr_s, P_sacr_g = lim(d2*P_sacr, mx["r"]), lim((1. - d2)*P_sacr, mx["r"])
    P_racw, P_sacw, P_gacw, P_raut = (lim(t, mx["l"]) for t in (P_racw, P_sacw, P_gacw, P_raut))
    P_saci, P_gaci, P_saut = (lim(t, mx["i"]) for t in (P_saci, P_gaci, P_saut))
    P_racs, P_gacs, P_gaut, P_ssub, P_smlt = (lim(t, mx["s"]) for t in (P_racs, P_gacs, P_gaut, P_ssub, P_smlt))
    P_gacr, P_revp, P_gfrz = (lim(t, mx["r"]) for t in (P_gacr, P_revp, P_gfrz))
    P_sdep, P_gdep = lim(P_sdep, mx["v"]), lim(P_gdep, mx["v"])
    P_gsub, P_gmlt = lim(P_gsub, mx["g"]), lim(P_gmlt, mx["g"])
    v2s, v2g = P_sdep, P_gdep
    c2r, c2g, c2s = P_racw + P_sacw*Tp + P_raut, P_gacw, P_sacw*Tn
    r2v, r2g, r2s = P_revp, P_gacr + P_iacr_g + P_sacr_g*Tn + P_gfrz*Tn, P_sacr_s*Tn + P_iacr_s
    i2s, i2g = P_raci_s + P_saci + P_saut, P_raci_g + P_gaci
    s2g, s2r, s2v = P_gacs + P_racs + P_gaut, P_smlt, P_ssub
    g2r, g2v = P_gmlt*Tp, P_gsub
    net = {"v": -v2s - v2g, "l": -c2r - c2g - c2s, "i": -i2s - i2g, "r": c2r + s2r + g2r - r2v - r2g - r2s,
           "s": c2s + i2s + v2s - s2g - s2v - s2r, "g": c2g + r2g + i2g + v2g + s2g - g2r - g2v}
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = {x: np.where(net[x] < 0., np.minimum(-mx[x]/net[x], 1.), 1.) for x in net}
    busy = has["liq"] | has["ice"] | has["rain"] | has["snow"] | has["graupel"]
    return {"T": T, "S_w": S_w, "S_i": S_i, "has": has, "factor": factor, "V": V, "busy": busy, "qv": qv}


# ---- the shim ---------------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    lib.ref_nsw6_conversion.argtypes = [ci, C.POINTER(Dims), cd, cd] + [vp]*17; lib.ref_nsw6_conversion.restype = None
    lib.ref_nsw6_sedimentation.argtypes = [ci, C.POINTER(Dims), ci, cd] + [vp]*6; lib.ref_nsw6_sedimentation.restype = None
    lib.ref_nsw6_cfl.argtypes = [ci, C.POINTER(Dims), ci, cd] + [vp]*4; lib.ref_nsw6_cfl.restype = cd
    lib.ref_nsw6_ql_qi.argtypes = [ci, C.POINTER(Dims)] + [vp]*7; lib.ref_nsw6_ql_qi.restype = ci


shim = refshim.Shim("nsw6", ["ref_nsw6_shim.cpp"], _bind, ref_sources=refshim.MASTER)


def ref_ql_qi(g, h):
    """ql, qi and T of the reference's sat_adjust on the interior (zero elsewhere); asserts that it converged everywhere."""
    d = dims_of(g)
    ql, qi, T = (np.zeros(g.shape3, dtype=g.np_dtype) for _ in range(3))
    threw = shim().ref_nsw6_ql_qi(code(g.np_dtype), C.byref(d), cm.ptr(h["thl"]), cm.ptr(h["qt"]), cm.ptr(h["p"]), cm.ptr(h["exn"]), cm.ptr(ql), cm.ptr(qi),
                                  cm.ptr(T))
    assert threw == 0, "the seeded inputs must converge on the reference"
    return ql, qi, T


def ref_exec(shape, dtype, mask, dtname, mode, zero_tend=False, gc=(1, 1, 1)):
    """Microphys_nsw6::exec of the reference on the case, the parts of the mask in its order: the five tendencies, the three surface
    rates, and the ql, qi, T it ran on."""
    c, g = ice_case(shape), grid_of(shape, gc, dtype)
    h = c.inputs(g, zero_tend)
    d = dims_of(g)
    lib = shim()
    if mode == "sat":
        h["ql"], h["qi"], h["T"] = ref_ql_qi(g, h)
    if mask & CONV:
        lib.ref_nsw6_conversion(code(dtype), C.byref(d), NC0, c.dt[dtname], *[cm.ptr(h[n]) for n in ("qrt", "qst", "qgt", "qtt", "thlt")],
                                *[cm.ptr(h[n]) for n in ("qr", "qs", "qg", "qt", "thl", "ql", "qi", "rho", "exn", "p")], cm.ptr(g.dzi), cm.ptr(g.dzhi))
    for s in range(3):
        if mask & (SEDI_R << s):
            lib.ref_nsw6_sedimentation(code(dtype), C.byref(d), s, c.dt[dtname], cm.ptr(h[OUT[s]]), cm.ptr(h[BOT[s]]), cm.ptr(h[SPECIES[s]]),
                                       cm.ptr(h["rho"]), cm.ptr(g.dzi), cm.ptr(g.dz))
    return h


def ref_cfl(shape, dtype, dtname):
    """get_time_limit's cfl (:1125-1174): the largest of the three, at least 1e-5, a double."""
    c, g = ice_case(shape), grid_of(shape, (1, 1, 1), dtype)
    h = c.inputs(g)
    d = dims_of(g)
    cfl = max(shim().ref_nsw6_cfl(code(dtype), C.byref(d), s, c.dt[dtname], cm.ptr(h[SPECIES[s]]), cm.ptr(h["rho"]), cm.ptr(g.dzi), cm.ptr(g.dz))
              for s in range(3))
    return max(cfl, 1.e-5)


def near_threshold(r, g, dtype):
    """Interior cells of a "sat" run whose reference ql, qi, qv or T (the T conversion computes from ql and qi, :194) lies within a
    relative 1e-12 (fp64) / 1e-5 (fp32) of the threshold a branch of conversion compares it with."""
    tol = 1e-12 if np.dtype(dtype) == np.float64 else 1e-5
    i = g.interior
    ql, qi, qt = (r[n][i].astype(np.float64) for n in ("ql", "qi", "qt"))
    Tc = r["exn"].astype(np.float64)[g.kstart:g.kend, None, None]*r["thl"][i].astype(np.float64) + 2.501e6/1005.*ql + (2.501e6 + 3.337e5)/1005.*qi
    near = lambda a, t: np.abs(a - t) <= tol*t
    return near(ql, 1e-7) | near(qi, 1e-7) | near(qt - ql - qi, 1e-7) | near(Tc, T0)


def golden_runs():
    """(shape, mask name, mask, step name, mode) of every run the golden file holds."""
    runs = []
    for shape in SHAPES:
        for mode in MODES:
            runs.append((shape, "all", ALL, "hi", mode))
    for shape in SMALL:
        runs.append((shape, "conv", CONV, "hi", "given"))
        for name in ("sedi_r", "sedi_s", "sedi_g"):
            for dtname in ("lo", "hi"):
                runs.append((shape, name, MASKS[name], dtname, "given"))
    return runs


def stored(shape, mask, mode):
    """The outputs of a run that the golden file holds: everything of the small shapes; of the large ones every STRIDE-th column, and
    of their "sat" run thlt alone (the tendency every transfer but one enters)."""
    if shape in SMALL or mode == "given":
        return WRITES[mask]
    return ("thlt",)


def pick(shape, a):
    """What the golden file keeps of an interior array (3-D or 2-D) of the shape."""
    return a if shape in SMALL else np.ascontiguousarray(a[..., ::STRIDE])


def run_key(shape, name, dtname, mode, dtype):
    return "exec/%dx%dx%d/%s/%s/%s/%s/" % (shape + (name, dtname, mode, tag(dtype)))


def _compute_all():
    rec = {}
    for dt in cm.DTYPES:
        for shape, name, mask, dtname, mode in golden_runs():
            r = ref_exec(shape, dt, mask, dtname, mode, zero_tend=True)
            g = grid_of(shape, (1, 1, 1), dt)
            key = run_key(shape, name, dtname, mode, dt)
            for n in stored(shape, mask, mode):
                rec[key + n] = pick(shape, r[n][g.jstart:g.jend, g.istart:g.iend] if n in BOT else r[n][g.interior]).copy()
            if mode == "sat":
                near = near_threshold(r, g, dt)
                assert not near.any(), "the seeded inputs put %d cells of %s on a threshold of conversion: change the seed" % (near.sum(), key)
                rec[key + "excluded"] = np.flatnonzero(near).astype(np.int32)
        for shape in SHAPES:
            for dtname in CFLS:
                rec["cfl/%dx%dx%d/%s/%s" % (shape + (dtname, tag(dt)))] = np.array([ref_cfl(shape, dt, dtname)])
    for shape in SHAPES:
        rec["digest/%s" % ice_case(shape).key] = np.array(ice_case(shape).digest())
    return rec


GOLD = refshim.Golden("nsw6", _compute_all, "tests/test_nsw6_exec.py")
RECORD, golden, computed, exact_here, ref, record_if_asked = GOLD.record, GOLD.golden, GOLD.computed, GOLD.exact_here, GOLD.ref, GOLD.record_if_asked


# ---- the device -------------------------------------------------------------------------------------------------------------
class Dev:
    """The arrays of one (shape, gc, dtype) on a backend and the calls on them."""

    def __init__(self, be, shape, gc, dtype, zero_tend=False, host=None):
        from microhh_amd import capi
        self.capi = capi
        self.be, self.c, self.g = be, ice_case(shape), grid_of(shape, gc, dtype)
        self.h = self.c.inputs(self.g, zero_tend) if host is None else host
        self.G = be.grid(self.g)
        self.d = {n: be.arr(a) for n, a in self.h.items()}
        self.scratch = [be.arr(np.full(self.g.ncells, -9.e9, dtype=dtype)) for _ in range(6)]
        self.scratch_ptrs = (C.c_void_p*6)(*[be.ptr(a).value for a in self.scratch])
        self.work = be.zeros(16, np.float64)
        self.keep, self.cptr, self.count = M.counter(be)

    def args(self, mode):
        be, d = self.be, self.d
        cloud = [be.ptr(d["ql"]), be.ptr(d["qi"])] if mode == "given" else [None, None]
        return [be.ptr(d[n]) for n in ("qr", "qs", "qg", "thl", "qt")] + cloud + [be.ptr(d[n]) for n in OUT + BOT + ("rho", "p", "exn")] + \
               [self.scratch_ptrs, self.cptr, be.stream]

    def exec(self, mask, dt, mode, impl=None, nc0=NC0):
        be, d = self.be, self.d
        p = self.capi.MhhMicroParams(nc0, dt, mask)
        if impl is None:
            rc = be.lib.mhh_micro_nsw6_exec(self.G, C.byref(p), *self.args(mode))
        else:
            rc = be.lib.mhh_micro_nsw6_exec_impl(self.G, impl, C.byref(p), *self.args(mode))
        self.capi.check(rc, be.lib)
        be.sync()
        g = self.g
        out = {n: be.host(d[n]).reshape(g.shape3) for n in SPECIES + ("thl", "qt", "ql", "qi") + OUT}
        for n in BOT:
            out[n] = be.host(d[n]).reshape(g.shape2)
        return out

    def cfl(self, dt, impl=None):
        be, d = self.be, self.d
        out = C.c_double(0)
        a = [be.ptr(d[n]) for n in SPECIES + ("rho",)] + [dt, be.ptr(self.work), C.byref(out), be.stream]
        rc = be.lib.mhh_micro_nsw6_cfl(self.G, *a) if impl is None else be.lib.mhh_micro_nsw6_cfl_impl(self.G, impl, *a)
        self.capi.check(rc, be.lib)
        return out.value


