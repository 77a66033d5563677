"""Shared test plumbing: library loading, synthetic inputs, call helpers.

Oracle (oracle/liborc.so) and the in-place reference build (oracle/_ref/libmhhref.so) are TEST
infrastructure; they are loaded here and nowhere under microhh_amd/.
"""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from microhh_amd import capi  # noqa: E402
from microhh_amd.grid import (Grid, MhhGrid, EDGE_EW, EDGE_NS, EDGE_BOTH,  # noqa: E402,F401
                              ADVEC_2, ADVEC_2I5, ADVEC_2I4, ADVEC_2I62, ADVEC_2I53, ADVEC_4M, ADVEC_4, DIFF_2, DIFF_4, DIFF_SMAG2, moser_z, uniform_z)

ORACLE_DIR = os.path.join(ROOT, "oracle")
_libs = {}

BACKENDS = [pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)]      # tests/backends.py
DTYPES = [np.float64, np.float32]

# Every environment variable the library reads (microhh_amd/csrc: per call; microhh_amd/model.py: per HotPath).
# tests/test_switches.py compares this tuple with the sources.
KNOWN_SWITCHES = (
    "MHH_ADVEC25_IMPL", "MHH_DIFF22_IMPL", "MHH_RHS25_IMPL", "MHH_RHS44_IMPL", "MHH_VISC_IMPL", "MHH_SCALAR_IMPL", "MHH_SCALAR_BATCH",
    "MHH_MARCH_DMA", "MHH_MARCH_HX", "MHH_MARCH_F32X2", "MHH_MARCH_KC_RT", "MHH_VISC_KC_RT",
    "MHH_PRES_LDS", "MHH_PRES_LDS_KC", "MHH_PRES_PITCH", "MHH_PRES_Y_TWISTED", "MHH_PRES_UNPACK_OUT", "MHH_PRES_RK_FUSED", "MHH_PRES4_WT",
    "MHH_PRES_SLAB_LDS", "MHH_OVERLAP", "MHH_FORCE_COMM", "MHH_PRES_CHUNKS",
)


def known_switches(names):
    """names, after checking that each is one the library reads: a misspelt switch would leave an A/B test comparing a form
    with itself."""
    unknown = sorted(set(names) - set(KNOWN_SWITCHES))
    if unknown:
        raise KeyError("not a switch the library reads (tests/common.py, KNOWN_SWITCHES): " + ", ".join(unknown))
    return names


@contextlib.contextmanager
def switches(**kw):
    """Environment switches for the duration of a block (the library reads them per call): NAME=value sets str(value), NAME=None
    takes the variable away. On the way out, through an exception as well, each is what it was before: its old value, or absent."""
    old = {k: os.environ.get(k) for k in known_switches(kw)}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    put(kw)
    try:
        yield
    finally:
        put(old)


def build_oracle():
    """make -C oracle (liborc*.so always; _ref only where /root/reference exists)."""
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "all"], check=True)


def _load(path):
    if path not in _libs:
        _libs[path] = C.CDLL(path)
    return _libs[path]


def oracle(perf=False):
    p = os.path.join(ORACLE_DIR, "liborc_perf.so" if perf else "liborc.so")
    if not os.path.exists(p):
        build_oracle()
    lib = _load(p)
    for n in ("orc_advec_cfl", "orc_smag2_dnmul", "orc_pres_divergence"):
        getattr(lib, n).restype = C.c_double
    return lib


def ref(perf=False):
    """The reference's own TUs compiled in place; None when neither source nor prebuilt lib exists."""
    p = os.path.join(ORACLE_DIR, "_ref", "libmhhref_perf.so" if perf else "libmhhref.so")
    if not os.path.exists(p):
        if os.path.isdir("/root/reference/src"):
            build_oracle()
        else:
            return None
    lib = _load(p)
    for n in ("ref_advec_2_cfl", "ref_advec_2i5_cfl", "ref_advec_2i4_cfl", "ref_advec_2i62_cfl", "ref_advec_2i53_cfl", "ref_advec_4m_cfl", "ref_advec_4_cfl", "ref_smag2_dnmul"):
        getattr(lib, n).restype = C.c_double
    return lib


def ptr(a):
    """void* of a numpy array (None -> NULL)."""
    if a is None:
        return C.c_void_p(0)
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


def dbl(x):
    return C.c_double(float(x))


class Case:
    """Synthetic inputs in the style of the reference's kernel_tuner harness (kernel_tuner/helpers.py:9,70-76:
    numpy.random.seed(666), uniform [0,1) fields in the order u, v, w, s, then rhoref, rhorefh), on a
    PHYSICAL grid instead of random metrics."""

    def __init__(self, grid, seed=666, nscalars=1, rho="random", tend_scale=1e-3, vel_shift=0.5, periodic=False):
        self.grid = g = grid
        t = g.np_dtype
        rs = np.random.RandomState(seed)
        n3, n2 = g.shape3, g.shape2

        def f3():
            return rs.random_sample(n3).astype(t)

        def f2(scale=1.0):
            return (rs.random_sample(n2) * scale).astype(t)
        # velocities centred around zero so that |u| upwind branches see both signs
        self.u = (f3() - t.type(vel_shift)).astype(t)
        self.v = (f3() - t.type(vel_shift)).astype(t)
        self.w = (f3() - t.type(vel_shift)).astype(t)
        self.s = [f3() for _ in range(nscalars)]
        if rho == "random":
            self.rhoref = (0.5 + rs.random_sample(g.kcells)).astype(t)
            self.rhorefh = (0.5 + rs.random_sample(g.kcells)).astype(t)
        else:
            self.rhoref = np.ones(g.kcells, dtype=t)
            self.rhorefh = np.ones(g.kcells, dtype=t)
        # walls: w = 0 at kstart and kend as the model keeps them (no-penetration)
        self.w[g.kstart] = 0
        self.w[g.kend] = 0
        self.ut = (f3() * tend_scale).astype(t)
        self.vt = (f3() * tend_scale).astype(t)
        self.wt = (f3() * tend_scale).astype(t)
        self.wt[g.kstart] = 0
        self.wt[g.kend:] = 0
        self.st = [(f3() * tend_scale).astype(t) for _ in range(nscalars)]
        self.evisc = (f3() * 0.1).astype(t)
        self.N2 = ((f3() - t.type(0.3)) * 1e-3).astype(t)
        self.dudz = f2(1e-2); self.dvdz = f2(1e-2); self.dbdz = f2(1e-4)
        self.z0m = np.full(n2, 0.1, dtype=t)
        self.u_fluxbot = f2(1e-2); self.u_fluxtop = f2(1e-2)
        self.v_fluxbot = f2(1e-2); self.v_fluxtop = f2(1e-2)
        self.s_fluxbot = f2(1e-2); self.s_fluxtop = f2(1e-2)
        self.p = np.zeros(n3, dtype=t)
        if periodic:   # what Boundary::set_prognostic_cyclic_bcs leaves behind (src/boundary.cxx:447-458)
            G = g.host_struct()
            for a in [self.u, self.v, self.w] + self.s:
                oracle().orc_boundary_cyclic(G, ptr(a), EDGE_BOTH)

    def copy_of(self, name):
        a = getattr(self, name)
        return [x.copy() for x in a] if isinstance(a, list) else a.copy()


def ulp_diff(a, b):
    """max |a-b| in units of the last place of max(|a|,|b|) (0 where bit-identical)."""
    a = np.asarray(a); b = np.asarray(b)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    m = np.maximum(np.abs(a), np.abs(b)).astype(a.dtype)
    sp = np.spacing(np.where(m == 0, np.finfo(a.dtype).tiny, m)).astype(np.float64)
    return float(np.max(d / sp)) if d.size else 0.0


SMALL_GRIDS_2 = [
    # (itot, jtot, ktot, igc, jgc, kgc)
    (16, 12, 10, 3, 3, 1),
    (24, 20, 18, 3, 3, 2),
    (8, 8, 6, 3, 3, 1),
]


def grid_2nd(itot=16, jtot=12, ktot=10, gc=(3, 3, 1), dtype=np.float64, stretched=True, z=None, **kw):
    """z: a stored stretched profile instead of moser_z's (whose last bits follow the host's numpy)."""
    if z is None and stretched:
        z = moser_z(ktot, 1200.)
    return Grid(itot, jtot, ktot, 3200., 3200., 1200., order=2, igc=gc[0], jgc=gc[1], kgc=gc[2], z=z, dtype=dtype, **kw)


def grid_4th(itot=16, jtot=12, ktot=12, dtype=np.float64, z=None, **kw):
    return Grid(itot, jtot, ktot, 2*np.pi, np.pi, 2., order=4, z=moser_z(ktot, 2.) if z is None else z, dtype=dtype, **kw)


def limiter_inputs(c, dtype):
    """Signed velocities (both upwind branches), a scalar with plateaus (the eps-guarded denominator), and with
    monotone as well as oscillating stretches (all pieces of the limiter function)."""
    u, v, w = (c.u - dtype(0.5)).astype(dtype), (c.v - dtype(0.5)).astype(dtype), (c.w - dtype(0.5)).astype(dtype)
    s = (np.round(c.s[0] * 6) / 6).astype(dtype)
    s.flat[::7] = c.s[0].flat[::7]
    return u, v, w, np.ascontiguousarray(s)


def same(a, b):
    return np.array_equal(a, b)


def same_bits(a, b):
    """same, for the modules whose reference is numpy itself: shape, dtype and every byte (-0. is not 0.)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def diff_params(sm, **kw):
    """mhh_diff_params as the tests start from it (cs 0.23, tPr 1/3, the given surface model), further members by name."""
    p = capi.MhhDiffParams(); p.cs = 0.23; p.tPr = 1./3.; p.surface_model = sm
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def tendencies(be, d):
    """ut, vt, wt and the list of every st of a backends.DevCase as host arrays: what oracle_rhs returns."""
    return be.host(d.ut), be.host(d.vt), be.host(d.wt), [be.host(x) for x in d.st]


def flat(tend):
    """[ut, vt, wt, st0, st1, ...] of what tendencies and oracle_rhs return."""
    return list(tend[:3]) + list(tend[3])


def oracle_rhs(c, adv, dif, sm, tPr=1./3., visc=1e-5, svisc=1e-5, limited=(), buoy=None):
    """Advec::exec followed by Diff::exec on the oracle; returns the tendencies (ut, vt, wt, [st]). dif None: Advec::exec alone.
    svisc: one diffusivity or one per scalar; limited: the scalars of advec.fluxlimit_list; buoy = (order, scalar, threfh, grav):
    Thermo_dry's buoyancy first."""
    O = oracle(); g = c.grid; Gh = g.host_struct()
    ut, vt, wt, st = c.ut.copy(), c.vt.copy(), c.wt.copy(), [x.copy() for x in c.st]
    sv = list(svisc) if isinstance(svisc, (list, tuple)) else [svisc] * len(st)
    a = (ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))
    if buoy is not None:          # Thermo_dry::exec runs before Advec::exec (src/model.cxx:365,388)
        order, n, threfh, grav = buoy
        O.orc_buoyancy_tend(Gh, order, ptr(wt), ptr(c.s[n]), ptr(threfh), dbl(grav))
    O.orc_advec_u(Gh, adv, ptr(ut), *a); O.orc_advec_v(Gh, adv, ptr(vt), *a); O.orc_advec_w(Gh, adv, ptr(wt), *a)
    for n in range(len(st)):
        if n in limited:
            O.orc_advec_s_lim(Gh, ptr(st[n]), ptr(c.s[n]), *a)
        else:
            O.orc_advec_s(Gh, adv, ptr(st[n]), ptr(c.s[n]), *a)
    if dif is None:
        return ut, vt, wt, st
    if dif in (DIFF_2, DIFF_4):
        o = 2 if dif == DIFF_2 else 4
        O.orc_diff_c(Gh, o, ptr(ut), ptr(c.u), dbl(visc)); O.orc_diff_c(Gh, o, ptr(vt), ptr(c.v), dbl(visc)); O.orc_diff_w(Gh, o, ptr(wt), ptr(c.w), dbl(visc))
        for n in range(len(st)):
            O.orc_diff_c(Gh, o, ptr(st[n]), ptr(c.s[n]), dbl(sv[n]))
    else:
        O.orc_smag2_diff_u(Gh, sm, ptr(ut), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(c.u_fluxbot), ptr(c.u_fluxtop), ptr(c.rhoref), ptr(c.rhorefh), dbl(visc))
        O.orc_smag2_diff_v(Gh, sm, ptr(vt), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(c.v_fluxbot), ptr(c.v_fluxtop), ptr(c.rhoref), ptr(c.rhorefh), dbl(visc))
        O.orc_smag2_diff_w(Gh, ptr(wt), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(c.rhoref), ptr(c.rhorefh), dbl(visc))
        for n in range(len(st)):
            O.orc_smag2_diff_c(Gh, sm, ptr(st[n]), ptr(c.s[n]), ptr(c.evisc), ptr(c.s_fluxbot), ptr(c.s_fluxtop), ptr(c.rhoref), ptr(c.rhorefh), dbl(tPr), dbl(sv[n]))
    return ut, vt, wt, st
