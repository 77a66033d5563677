"""Shared plumbing of the surface-layer tests (tests/test_surface_*.py): the seeded cases, the reference run and the device run.

The reference is the reference's OWN templates (Boundary_surface_kernels, Monin_obukhov) behind tests/cpp/ref_surface_shim.cpp,
compiled into a temporary directory where the reference tree exists. Where it is absent (the GPU box) the same cases read
tests/golden/surface_ref.npz, recorded with MHH_RECORD_SURFACE_GOLDEN=1 python -m pytest tests/test_surface_ref.py: the inputs
and the reference outputs of every case, and the digests of the four lookup tables (the tables themselves are 80 kB each).
"""
import ctypes as C

import numpy as np

import common as cm
import refshim
from refshim import digest, have_reference  # noqa: F401
from microhh_amd import capi
from microhh_amd.grid import Grid

NZL = 10000
DIRICHLET, NEUMANN, FLUX, USTAR = 0, 1, 2, 3
NONE, DRY, BUOY = 0, 1, 2
GRAV, THREF, THREFH, N2 = 9.81, 300., 299.9, 1.e-5
Z0M = Z0H = 0.1
UBOT, VBOT = 0.1, -0.05
ZL_LIMIT = 8.                      # |zsl/L| of every toleranced case: far beyond, the denominators of fm / fh cancel (~50 times at the table's end, -1e4)

# (itot, jtot, ktot, (igc, jgc, kgc))
SHAPES = [(70, 9, 10, (3, 3, 1)), (17, 9, 8, (3, 3, 1)), (20, 1, 12, (3, 3, 1)), (16, 6, 8, (4, 2, 1))]
SMALL = SHAPES[2]
# name: (mbcbot, thermo kind, [sbcbot per scalar]); scalar 0 is th / b
CONFIGS = {
    "flux":           (DIRICHLET, DRY,  [FLUX]),
    "dirichlet":      (DIRICHLET, DRY,  [DIRICHLET]),
    "ustar_buoy":     (USTAR,     BUOY, [FLUX, DIRICHLET]),
    "dirichlet_buoy": (DIRICHLET, BUOY, [DIRICHLET, FLUX]),
    "neutral":        (DIRICHLET, NONE, [DIRICHLET]),
}
CASES = [(c, s) for c in ("flux", "dirichlet") for s in SHAPES] + [(c, SMALL) for c in ("ustar_buoy", "dirichlet_buoy", "neutral")]
CASE_IDS = ["%s-%dx%dx%d" % (c, s[0], s[1], s[2]) for c, s in CASES]
OUT2D = ["dutot", "ustar", "obuk", "nobuk", "ufluxbot", "vfluxbot", "ugradbot", "vgradbot", "dudz", "dvdz", "dbdz"]
EXACT = ["nobuk", "obuk", "ugradbot", "vgradbot", "sgradbot0", "sgradbot1"]


def grid_of(shape, dtype, **kw):
    itot, jtot, ktot, gc = shape
    return Grid(itot, jtot, ktot, 3200., 3200., 10.*ktot, order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], dtype=dtype, **kw)   # zsl = z[kstart] = 5


def wrap(a, g):
    """Boundary_cyclic::exec_2d of a [jcells][icells] array (in place)."""
    a[:, :g.istart] = a[:, g.iend-g.igc:g.iend]; a[:, g.iend:] = a[:, g.istart:g.istart+g.igc]
    if g.jtot == 1:
        a[:g.jstart] = a[g.jstart]; a[g.jend:] = a[g.jstart]
    else:
        a[:g.jstart] = a[g.jend-g.jgc:g.jend]; a[g.jend:] = a[g.jstart:g.jstart+g.jgc]
    return a


class SurfCase:
    """Seeded inputs of one (config, shape); the float64 draws are the master copy, narrowed for fp32."""

    def __init__(self, config, shape, dtype, seed=2024):
        self.config, self.shape, self.dtype = config, shape, np.dtype(dtype)
        self.mbcbot, self.kind, self.sbc = CONFIGS[config]
        self.thermobc = self.sbc[0]
        self.g = g = grid_of(shape, dtype)
        self.id = "%s-%dx%dx%d-%s" % (config, shape[0], shape[1], shape[2], "f64" if self.dtype == np.float64 else "f32")
        rs = np.random.RandomState(seed + 7*shape[0] + len(config))
        n2 = g.shape2
        jj, ii = np.meshgrid(np.arange(g.jcells) - g.jstart, np.arange(g.icells) - g.istart, indexing="ij")
        # a wind whose filtered speed against (ubot, vbot) spans [0.5, 3]: smooth amplitude and direction, 5 % noise
        amp = 1.7 + 1.0*np.sin(2*np.pi*ii/g.itot)*np.cos(2*np.pi*jj/g.jtot)
        phi = 0.5 + 2.0*np.cos(2*np.pi*ii/g.itot + 1.)
        m = {}
        m["u"] = wrap(amp*np.cos(phi)*(1. + 0.05*(rs.random_sample(n2) - 0.5)) + UBOT, g)
        m["v"] = wrap(amp*np.sin(phi)*(1. + 0.05*(rs.random_sample(n2) - 0.5)) + VBOT, g)
        for n, bc in enumerate(self.sbc):
            thermo = (n == 0 and self.kind != NONE)
            if thermo and self.kind == BUOY:
                m["s%d" % n] = wrap(0.02*rs.random_sample(n2), g)                          # b at kstart
                bot = wrap(0.01 + 0.012*(rs.random_sample(n2) - 0.5), g)                   # db of both signs
                sign = np.where(rs.random_sample(n2) < 0.3, -0.2, 1.)
                flux = wrap(sign*(5.e-4 + 2.5e-3*rs.random_sample(n2)), g)                 # buoyancy flux, both signs, away from 0
            else:
                m["s%d" % n] = wrap(THREF + rs.random_sample(n2), g)                        # th at kstart
                bot = wrap(THREF + 0.5 + 0.4*(rs.random_sample(n2) - 0.5), g)              # db of both signs
                flux = wrap(0.02 + 0.08*rs.random_sample(n2), g)                           # theta flux in [0.02, 0.1]
            m["sbot%d" % n] = bot if bc == DIRICHLET else np.zeros(n2)
            m["sfluxbot%d" % n] = flux if bc == FLUX else np.zeros(n2)
        # values a float holds exactly: both dtypes see the same numbers, and the golden file stores them once and compresses them
        self.master = {k: v.astype(np.float32).astype(np.float64) for k, v in m.items()}

    # ---- inputs in the case's dtype ------------------------------------------------------------------
    def inputs(self, master=None):
        return {k: np.ascontiguousarray(v, dtype=self.dtype) for k, v in (master or self.master).items()}

    def state(self):
        g, t = self.g, self.dtype
        st = {"ustar": np.full(g.shape2, 0.3 if self.mbcbot == USTAR else 1e-2, dtype=t),     # set_ustar / init_surface (:565-573,807)
              "obuk": np.full(g.shape2, 1e-9, dtype=t), "nobuk": np.zeros(g.shape2, dtype=np.int32)}
        return st

    def out_names(self):
        names = list(OUT2D)
        for n in range(len(self.sbc)):
            names += ["sbot%d" % n, "sgradbot%d" % n, "sfluxbot%d" % n]
        if self.kind == NONE:
            names.remove("dbdz"); names.remove("nobuk")
        return names


# ---- the reference ---------------------------------------------------------------------------------------
class RefIO(C.Structure):
    _fields_ = [("dtype", C.c_int), ("itot", C.c_int), ("jtot", C.c_int), ("igc", C.c_int), ("jgc", C.c_int),
                ("mbcbot", C.c_int), ("thermobc", C.c_int), ("thermo_kind", C.c_int), ("thermo_index", C.c_int), ("nscalars", C.c_int),
                ("skip_dutot", C.c_int), ("sbcbot", C.c_int * 8),
                ("zsl", C.c_double), ("thref", C.c_double), ("threfh", C.c_double), ("grav", C.c_double), ("n2", C.c_double),
                ("zL", C.c_void_p), ("f", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("s", C.c_void_p * 8),
                ("ubot", C.c_void_p), ("vbot", C.c_void_p), ("z0m", C.c_void_p), ("z0h", C.c_void_p),
                ("dutot", C.c_void_p), ("ustar", C.c_void_p), ("obuk", C.c_void_p), ("nobuk", C.c_void_p),
                ("ufluxbot", C.c_void_p), ("vfluxbot", C.c_void_p), ("ugradbot", C.c_void_p), ("vgradbot", C.c_void_p),
                ("sbot", C.c_void_p * 8), ("sgradbot", C.c_void_p * 8), ("sfluxbot", C.c_void_p * 8),
                ("dudz", C.c_void_p), ("dvdz", C.c_void_p), ("dbdz", C.c_void_p)]


def _bind(lib):
    lib.ref_surface_exec.argtypes = [C.POINTER(RefIO)]; lib.ref_surface_exec.restype = None
    lib.ref_surface_lut.argtypes = [C.c_double]*3 + [C.c_int]*3 + [C.c_void_p]*2; lib.ref_surface_lut.restype = None


shim = refshim.Shim("surface", ["ref_surface_shim.cpp"], _bind)


def zsl_of(g):
    return float(g.z[g.kstart])


def lut(fn, g, mbcbot, thermobc):
    """(zL, f) from prepare_lut: fn = the shim's ref_surface_lut or a library's mhh_surface_lut_host."""
    zL, f = np.zeros(NZL, dtype=np.float32), np.zeros(NZL, dtype=np.float32)
    rc = fn(zsl_of(g), Z0M, Z0H, mbcbot, thermobc, g.dtype, cm.ptr(zL), cm.ptr(f))
    assert not rc, rc
    return zL, f


def ref_exec(case, inp, st, table, dutot=None):
    """Boundary_surface::exec of the reference on inputs `inp` and state `st` (updated in place); returns every 2-D output.
    dutot given: calc_dutot is skipped (the stage test)."""
    g, t = case.g, case.dtype
    out = {k: np.zeros(g.shape2, dtype=t) for k in OUT2D if k not in ("ustar", "obuk", "nobuk")}
    if dutot is not None:
        out["dutot"] = np.ascontiguousarray(dutot, dtype=t).copy()
    out.update(st)
    ns = len(case.sbc)
    for n in range(ns):
        out["sbot%d" % n] = inp["sbot%d" % n].copy(); out["sfluxbot%d" % n] = inp["sfluxbot%d" % n].copy()
        out["sgradbot%d" % n] = np.zeros(g.shape2, dtype=t)
    const = {"ubot": np.full(g.shape2, UBOT, dtype=t), "vbot": np.full(g.shape2, VBOT, dtype=t),
             "z0m": np.full(g.shape2, Z0M, dtype=t), "z0h": np.full(g.shape2, Z0H, dtype=t)}
    io = RefIO()
    io.dtype, io.itot, io.jtot, io.igc, io.jgc = g.dtype, g.itot, g.jtot, g.igc, g.jgc
    io.mbcbot, io.thermobc, io.thermo_kind, io.thermo_index, io.nscalars = case.mbcbot, case.thermobc, case.kind, 0, ns
    io.skip_dutot = 0 if dutot is None else 1
    io.zsl, io.thref, io.threfh, io.grav, io.n2 = zsl_of(g), THREF, THREFH, GRAV, N2
    io.zL, io.f = table[0].ctypes.data, table[1].ctypes.data
    io.u, io.v = inp["u"].ctypes.data, inp["v"].ctypes.data
    for k, a in const.items():
        setattr(io, k, a.ctypes.data)
    for k in OUT2D:
        setattr(io, k, out[k].ctypes.data)
    for n in range(ns):
        io.sbcbot[n] = case.sbc[n]; io.s[n] = inp["s%d" % n].ctypes.data
        io.sbot[n] = out["sbot%d" % n].ctypes.data; io.sgradbot[n] = out["sgradbot%d" % n].ctypes.data
        io.sfluxbot[n] = out["sfluxbot%d" % n].ctypes.data
    shim().ref_surface_exec(C.byref(io))
    return out


GOLD = refshim.Golden("surface", None, "tests/test_surface_ref.py")      # its first test holds every case and records them
RECORD, golden = GOLD.record, GOLD.golden


def golden_case(case):
    """(inputs, reference outputs) of a case from the golden file."""
    z = GOLD.need()
    mid = case.id.rsplit("-", 1)[0]
    master = {k: z["%s/in/%s" % (mid, k)] for k in case.master}
    return case.inputs(master), {k: z["%s/out/%s" % (case.id, k)] for k in case.out_names()}


# ---- the device ---------------------------------------------------------------------------------------------
class DevSurf:
    """The arrays of one case on a backend with mhh_fields / mhh_surface_params pointing at them."""

    def __init__(self, be, case, inp, st, lib_table=None):
        self.be, self.case, self.g = be, case, case.g
        g, t = case.g, case.dtype
        self.G = be.grid(g)
        ns = len(case.sbc)

        def lift(a2):           # the level kstart of a 3-D field; every other level holds a value no stage may read into a result
            a3 = np.full(g.shape3, 1.e3, dtype=t); a3[g.kstart] = a2
            return a3
        self.a = a = {}
        a["u"], a["v"] = be.arr(lift(inp["u"])), be.arr(lift(inp["v"]))
        for k, v in (("ubot", UBOT), ("vbot", VBOT), ("z0m", Z0M), ("z0h", Z0H)):
            a[k] = be.arr(np.full(g.shape2, v, dtype=t))
        for k in OUT2D:
            if k not in st:
                a[k] = be.zeros(g.shape2, t)
        for k, v in st.items():
            a[k] = be.arr(v)
        for n in range(ns):
            a["s%d" % n] = be.arr(lift(inp["s%d" % n]))
            a["sbot%d" % n], a["sfluxbot%d" % n] = be.arr(inp["sbot%d" % n]), be.arr(inp["sfluxbot%d" % n])
            a["sgradbot%d" % n] = be.zeros(g.shape2, t)
        table = lib_table if lib_table is not None else lut(be.lib.mhh_surface_lut_host, g, case.mbcbot, case.thermobc)
        a["zL"], a["f"] = be.arr(table[0]), be.arr(table[1])
        f = self.f = capi.MhhFields()
        f.u, f.v, f.nscalars = be.ptr(a["u"]).value, be.ptr(a["v"]).value, ns
        f.u_fluxbot, f.v_fluxbot = be.ptr(a["ufluxbot"]).value, be.ptr(a["vfluxbot"]).value
        f.dudz, f.dvdz, f.dbdz = be.ptr(a["dudz"]).value, be.ptr(a["dvdz"]).value, be.ptr(a["dbdz"]).value
        p = self.p = capi.MhhSurfaceParams()
        p.mbcbot, p.thermobc, p.thermo_kind, p.thermo_index, p.swconstantz0 = case.mbcbot, case.thermobc, case.kind, 0, 1
        p.thref_kstart, p.threfh_kstart, p.grav, p.bg_n2 = THREF, THREFH, GRAV, N2
        for k in ("zL", "f", "z0m", "z0h", "ustar", "obuk", "nobuk", "ubot", "vbot", "ugradbot", "vgradbot"):
            setattr(p, k, be.ptr(a[k]).value)
        for n in range(ns):
            f.s[n], f.s_fluxbot[n] = be.ptr(a["s%d" % n]).value, be.ptr(a["sfluxbot%d" % n]).value
            p.sbot[n], p.sgradbot[n], p.sbcbot[n] = be.ptr(a["sbot%d" % n]).value, be.ptr(a["sgradbot%d" % n]).value, case.sbc[n]

    def call(self, name, *args):
        capi.check(getattr(self.be.lib, name)(self.G, C.byref(self.f), C.byref(self.p), *args, self.be.stream), self.be.lib)

    def fill(self, name):
        capi.check(self.be.lib.mhh_boundary_cyclic_2d(self.G, self.be.ptr(self.a[name]), self.be.stream), self.be.lib)

    def staged(self, dutot_given=False):
        """The five stage calls with the cyclic fills between them: the reference's sequence."""
        d = self.be.ptr(self.a["dutot"])
        if not dutot_given:
            self.call("mhh_surface_dutot", d)
            self.fill("dutot")
        self.call("mhh_surface_stability", d)
        self.call("mhh_surface_momentum")
        self.fill("ufluxbot"); self.fill("vfluxbot")
        for n in range(len(self.case.sbc)):
            self.call("mhh_surface_scalar", n)
        self.call("mhh_surface_mo_gradients")

    def fused(self):
        self.call("mhh_boundary_surface_exec", self.be.ptr(self.a["dutot"]))

    def outputs(self):
        self.be.sync()
        return {k: self.be.host(self.a[k]) for k in self.case.out_names()}


def rel(got, ref):
    """max |got - ref| / max |ref| of one array, in float64."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.max(np.abs(ref))
    return float(np.max(np.abs(got - ref)) / den) if den > 0 else float(np.max(np.abs(got)))
