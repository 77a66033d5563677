"""Shared plumbing of the Buffer / Force tests (tests/test_force_buffer.py, tests/test_pres_ref.py): grids, settings, the numpy
restatement of the cited lines of src/buffer.cxx and src/force.cxx in their expression order, and the device side (Dev).

Dev takes the mean profiles and the two uflux sums either from mhh_field_mean_profile / mhh_field_mean_sum (the default) or, with
means= / sums=, from the caller: they are pointer inputs of mhh_force_params, so a test can feed recorded ones."""
import ctypes as C
import ctypes.util

import numpy as np

import backends as B
import common as cm
from common import same_bits as same
from microhh_amd import capi, forcing

SHAPES = [(70, 9, 10), (17, 9, 8), (20, 1, 12)]
NAMES = ["u", "v", "w", "s0", "s1"]

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.pow.restype, _libm.pow.argtypes = C.c_double, [C.c_double, C.c_double]
_libm.powf.restype, _libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]


def grid(shape, order, dtype, gc=None):
    if order == 2:
        return cm.grid_2nd(*shape, gc=gc or (1, 1, 1), dtype=dtype)
    gc = gc or (2, 2, 3)
    return cm.grid_4th(*shape, dtype=dtype, igc=gc[0], jgc=gc[1], kgc=gc[2])


def field(c, name, tend=False):
    if name in ("u", "v", "w"):
        return getattr(c, name + "t" if tend else name)
    return (c.st if tend else c.s)[int(name[1:])]


def prof(g, seed, scale=1., shift=0.):
    return (np.random.RandomState(seed).random_sample(g.kcells) * scale + shift).astype(g.np_dtype)


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------
def ref_sigma(g, zstart, sigma, beta, half):
    """sigmaz of calc_buffer (src/buffer.cxx:44,48), std::pow of a TF; 0 outside the sponge (never read)."""
    T = g.np_dtype.type
    z = g.zh if half else g.z
    out = np.zeros(g.kcells, dtype=g.np_dtype)
    zsizebuf = T(g.zsize) - T(zstart)
    for k in range(g.kstart, g.kend):
        if z[k] < T(zstart):
            continue
        x = (z[k] - T(zstart)) / zsizebuf
        out[k] = T(sigma) * (T(_libm.powf(float(x), float(T(beta)))) if T == np.float32 else T(_libm.pow(float(x), beta)))
    return out


def ref_kstart(g, zstart):
    ks = ksh = g.kstart
    for k in range(g.kstart, g.kend):
        ks += bool(g.z[k] < g.np_dtype.type(zstart))
        ksh += bool(g.zh[k] < g.np_dtype.type(zstart))
    return ks, ksh


def ref_buffer(g, tend, c, Bf):
    """Buffer::exec: tend = {name: array} updated in place. Bf: sigma, sigmah, ks, ksh, abuf {name: profile}."""
    J, I = slice(g.jstart, g.jend), slice(g.istart, g.iend)
    for n, ab in Bf["abuf"].items():
        k0 = Bf["ksh"] if n == "w" else Bf["ks"]
        sg = Bf["sigmah"] if n == "w" else Bf["sigma"]
        K = slice(k0, g.kend)
        tend[n][K, J, I] -= sg[K, None, None] * (field(c, n)[K, J, I] - ab[K, None, None])


def ref_force(g, tend, c, P, means, sums):
    """Force::exec (:581-729) in its order: pressure force, swls, swwls, nudging. means {name: profile}, sums = the two doubles."""
    T = g.np_dtype.type
    ks, ke = g.kstart, g.kend
    J, I, K = slice(g.jstart, g.jend), slice(g.istart, g.iend), slice(ks, ke)

    def sh(a, dj=0, di=0):
        return a[K, g.jstart+dj:g.jend+dj, g.istart+di:g.iend+di]
    lp = P.get("swlspres")
    if lp == "dpdx":
        tend["u"][K, J, I] += T(-1.) * T(P["dpdx"])
    elif lp == "uflux":
        den = T(g.itot * g.jtot) * T(g.zsize)
        u_mean, ut_mean = T(np.float64(sums[0]) / np.float64(den)), T(np.float64(sums[1]) / np.float64(den))
        fbody = (T(P["uflux"]) - u_mean - T(P["utrans"])) / T(P["dt"]) - ut_mean
        assert type(fbody) is T
        tend["u"][K, J, I] += fbody
    elif lp == "geo":
        fc, ut_, vt_ = T(P["fc"]), T(P["utrans"]), T(P["vtrans"])
        u, v = c.u, c.v
        ug, vg = P["ug"][K, None, None], P["vg"][K, None, None]
        if P["order"] == 2:
            tend["u"][K, J, I] += fc * (T(0.25)*(sh(v, 0, -1) + sh(v) + sh(v, 1, -1) + sh(v, 1, 0)) + vt_ - vg)
            tend["v"][K, J, I] -= fc * (T(0.25)*(sh(u, -1, 0) + sh(u) + sh(u, -1, 1) + sh(u, 0, 1)) + ut_ - ug)
        else:
            ci = [T(-1./16.), T(9./16.), T(9./16.), T(-1./16.)]

            def row(a, dj, d0):
                return ci[0]*sh(a, dj, d0) + ci[1]*sh(a, dj, d0+1) + ci[2]*sh(a, dj, d0+2) + ci[3]*sh(a, dj, d0+3)
            tend["u"][K, J, I] += fc * ((ci[0]*row(v, -1, -2) + ci[1]*row(v, 0, -2) + ci[2]*row(v, 1, -2) + ci[3]*row(v, 2, -2)) + vt_ - vg)
            tend["v"][K, J, I] -= fc * ((ci[0]*row(u, -2, -1) + ci[1]*row(u, -1, -1) + ci[2]*row(u, 0, -1) + ci[3]*row(u, 1, -1)) + ut_ - ug)
    for n, ls in P.get("ls", {}).items():
        tend[n][K, J, I] += ls[K, None, None]
    wls = P.get("wls")
    if P.get("swwls"):
        who = (["u", "v"] if P.get("mom") else []) + [n for n in tend if n[0] == "s"]
        for n in who:
            t, a = tend[n], field(c, n)
            for k in range(ks, ke):
                if P["swwls"] == "mean":
                    m = means[n]
                    d = wls[k] * (m[k]-m[k-1])*g.dzhi[k] if wls[k] > 0. else wls[k] * (m[k+1]-m[k])*g.dzhi[k+1]
                    assert type(d) is T
                elif wls[k] > 0.:
                    d = wls[k] * (a[k, J, I]-a[k-1, J, I])*g.dzhi[k]
                else:
                    d = wls[k] * (a[k+1, J, I]-a[k, J, I])*g.dzhi[k+1]
                t[k, J, I] -= d
        if P["swwls"] == "local" and P.get("mom"):
            w, t = c.w, tend["w"]
            for k in range(ks+1, ke):
                wl = T(0.5) * (wls[k-1] + wls[k])
                d = wl * (w[k, J, I]-w[k-1, J, I])*g.dzi[k-1] if wl > 0. else wl * (w[k+1, J, I]-w[k, J, I])*g.dzi[k]
                t[k, J, I] -= d
    for n, ref in P.get("nudge", {}).items():
        for k in range(ks, ke):
            tend[n][k, J, I] += -P["nfac"][k] * (means[n][k] - ref[k])


# ---- the device side -------------------------------------------------------------------------------------------------------------
def put(struct, stem, name, ptr):
    if name in ("u", "v", "w"):
        setattr(struct, "%s_%s" % (stem, name), ptr)
    else:
        getattr(struct, stem + "_s")[int(name[1:])] = ptr


class Dev:
    """A DevCase with the parameter structs of a settings dict, the device means it needs and the host copies of them."""

    def __init__(self, be, g, c, Bf=None, P=None, means=None, sums=None):
        """means {name: host profile}, sums (two doubles): used in place of the library's own where given."""
        self.be, self.g = be, g
        self.d = d = B.DevCase(be, c)
        self.f = d.fields()
        self.keep = []
        self.means, self.sums = {}, None
        P = P or {}
        need = set(P.get("nudge", {}))
        if P.get("swwls") == "mean":
            need |= {"s0", "s1"} | ({"u", "v"} if P.get("mom") else set())
        if Bf and Bf.get("swupdate"):
            need |= set(NAMES)
        dmeans = {}
        if need and means is not None:
            names = [n for n in NAMES if n in need]
            outs = [be.arr(np.ascontiguousarray(means[n], dtype=g.np_dtype)) for n in names]
            dmeans = dict(zip(names, outs))
            self.means = {n: be.host(o) for n, o in dmeans.items()}
            self.keep += outs
        elif need:
            names = [n for n in NAMES if n in need]
            flds = [field(d, n) for n in names]
            outs = [be.zeros(g.kcells, g.np_dtype) for _ in names]
            work = be.zeros(int(be.lib.mhh_field_mean_scratch_elems(d.G, len(names))), np.float64)
            B.ok(be, be.lib.mhh_field_mean_profile(d.G, self.ptrs(flds), len(names), self.ptrs(outs), be.ptr(work), be.stream))
            dmeans = dict(zip(names, outs))
            self.means = {n: be.host(o) for n, o in dmeans.items()}
            self.keep += outs
        self.b = b = capi.MhhBufferParams()
        if Bf:
            b.swbuffer, b.bufferkstart, b.bufferkstarth = 1, Bf["ks"], Bf["ksh"]
            b.sigma, b.sigmah = self.up(Bf["sigma"]), self.up(Bf["sigmah"])
            if Bf.get("swupdate"):
                Bf["abuf"] = dict(self.means)
            for n, a in Bf["abuf"].items():
                put(b, "abuf", n, be.ptr(dmeans[n]).value if Bf.get("swupdate") else self.up(a))
        self.p = p = capi.MhhForceParams()
        p.swlspres = forcing.LSPRES[P.get("swlspres")]
        p.order = P.get("order", 0)
        p.dpdx, p.uflux, p.dt, p.fc = P.get("dpdx", 0.), P.get("uflux", 0.), P.get("dt", 0.), P.get("fc", 0.)
        p.utrans, p.vtrans = P.get("utrans", 0.), P.get("vtrans", 0.)
        if P.get("swlspres") == "uflux":
            if sums is not None:
                dsums = be.arr(np.ascontiguousarray(sums, dtype=np.float64))
            else:
                dsums = be.zeros(2, np.float64)
                work = be.zeros(int(be.lib.mhh_field_mean_scratch_elems(d.G, 2)), np.float64)
                B.ok(be, be.lib.mhh_field_mean_sum(d.G, self.ptrs([d.u, d.ut]), 2, be.ptr(dsums), be.ptr(work), be.stream))
            self.sums = be.host(dsums)
            self.keep.append(dsums)
            p.uflux_sums = be.ptr(dsums).value
        if P.get("swlspres") == "geo":
            p.ug, p.vg = self.up(P["ug"]), self.up(P["vg"])
        for n, a in P.get("ls", {}).items():
            p.swls = 1
            put(p, "ls", n, self.up(a))
        p.swwls, p.swwls_mom = forcing.WLS[P.get("swwls")], int(bool(P.get("mom")))
        if p.swwls:
            p.wls = self.up(P["wls"])
        for n, t in dmeans.items():
            if n != "w":
                put(p, "mean", n, be.ptr(t).value)
        for n, a in P.get("nudge", {}).items():
            p.swnudge = 1
            p.nudge_factor = self.up(P["nfac"])
            put(p, "nudge", n, self.up(a))

    def ptrs(self, arrays):
        return (C.c_void_p * len(arrays))(*[self.be.ptr(a).value for a in arrays])

    def up(self, a):
        t = self.be.arr(a)
        self.keep.append(t)
        return self.be.ptr(t).value

    def tendencies(self):
        return {n: self.be.host(field(self.d, n, tend=True)) for n in NAMES}

    def buffer(self):
        return self.be.lib.mhh_buffer_exec(self.d.G, C.byref(self.f), C.byref(self.b), self.be.stream)

    def force(self):
        return self.be.lib.mhh_force_exec(self.d.G, C.byref(self.f), C.byref(self.p), self.be.stream)

    def fused(self):
        return self.be.lib.mhh_buffer_force_exec(self.d.G, C.byref(self.f), C.byref(self.b), C.byref(self.p), self.be.stream)


def host_tend(c):
    return {n: field(c, n, tend=True).copy() for n in NAMES}


def assert_same(got, want, what):
    for n in NAMES:
        assert same(got[n], want[n]), (what, n, cm.ulp_diff(got[n], want[n]))


def buffer_setup(be, g, swupdate=False):
    """zstart between a half level and the full level above it, two thirds up: bufferkstart != bufferkstarth."""
    k = g.kstart + (2 * g.kmax) // 3
    zstart = 0.5 * (float(g.zh[k]) + float(g.z[k]))
    ks, ksh = ref_kstart(g, zstart)
    assert ks != ksh and (ks, ksh) == forcing.buffer_kstart(g, zstart) and g.kstart < ksh < g.kend
    sg, sgh = forcing.sigma_tables(be.lib, g, zstart, 2., 2.3)
    assert same(sg, ref_sigma(g, zstart, 2., 2.3, 0)) and same(sgh, ref_sigma(g, zstart, 2., 2.3, 1))
    assert sg[ks:g.kend].all() and not sg[:ks].any()
    Bf = dict(ks=ks, ksh=ksh, sigma=sg, sigmah=sgh, swupdate=swupdate)
    if not swupdate:
        Bf["abuf"] = {n: prof(g, 11 + i, 1., -0.3) for i, n in enumerate(NAMES)}
    return Bf


def force_setup(g, term, order):
    """The settings of one Force term, or of all of them together."""
    P = {}
    ug, vg = prof(g, 21, 2., -1.), prof(g, 22, 2., -1.)
    wls = (0.01 * np.sin(np.arange(g.kcells) * 0.9)).astype(g.np_dtype)            # changes sign several times
    assert (wls[g.kstart:g.kend] > 0).any() and (wls[g.kstart:g.kend] < 0).any()
    if term == "dpdx":
        P.update(swlspres="dpdx", dpdx=-2.3e-4)
    if term in ("uflux", "all4"):
        P.update(swlspres="uflux", uflux=0.11, dt=0.37, utrans=0.07)             # dt is no power of two
    if term in ("geo", "all"):
        P.update(swlspres="geo", order=order, fc=1.39e-4, ug=ug, vg=vg, utrans=0.13, vtrans=-0.21)
    if term in ("swls", "all", "all4"):
        P["ls"] = {"u": prof(g, 31, 1e-3, -5e-4), "s1": prof(g, 32, 1e-3, -5e-4)}
    if term.startswith("wls"):
        P.update(swwls=term.split("_")[1], mom=term.endswith("_mom"), wls=wls)
    if term == "all":
        P.update(swwls="local", mom=True, wls=wls)
    if term == "all4":
        P.update(swwls="mean", mom=True, wls=wls)
    if term in ("nudge", "all", "all4"):
        P["nudge"] = {"v": prof(g, 41, 1., 0.), "s0": prof(g, 42, 1., 0.)}
        P["nfac"] = prof(g, 43, 1e-3, 1e-4)
    return P


TERMS = ["dpdx", "uflux", "geo", "swls", "wls_mean", "wls_mean_mom", "wls_local", "wls_local_mom", "nudge", "all", "all4"]


# every term at 2nd order (gc = (1, 1, 1)); at 4th order (gc = (2, 2, 3)) the Coriolis term, the one that depends on the order, alone and
# with the others, and moser600's uflux
TERM_ORDERS = [(t, 2) for t in TERMS] + [("geo", 4), ("all", 4), ("uflux", 4)]
