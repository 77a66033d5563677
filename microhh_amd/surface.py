"""Boundary_surface of a sub-step (src/boundary_surface.cxx; src/model.cxx:374-375): the Monin-Obukhov surface layer with the
lookup solver, and the vertical ghost cells that follow it. The parameter struct of the C ABI, the state the reference keeps
between calls (ustar, obuk, nobuk), and the per-step calls HotPath makes with ``HotPath(..., surface=Surface(...))``.

Per-scalar settings are lists with one entry per scalar of the HotPath (or one value for all of them).
Time-dependent surface values (gabls1's th_sbot) are the caller's: refill ``surface.sbot[n]`` between steps.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import MhhSurfaceParams  # noqa: F401

DIRICHLET, NEUMANN, FLUX, USTAR = 0, 1, 2, 3
MBC = {"noslip": DIRICHLET, "ustar": USTAR}                      # Boundary::process_bcs (src/boundary.cxx:196-204)
MBCTOP = {"noslip": DIRICHLET, "freeslip": NEUMANN, "neumann": NEUMANN}
SBC = {"dirichlet": DIRICHLET, "neumann": NEUMANN, "flux": FLUX}   # (:238-258)
NZL = 10000
GRAV = 9.81


def _per_scalar(v, n, what):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * n
    if len(v) != n:
        raise ValueError("%s: one entry per scalar (%d)" % (what, n))
    return v


class Surface:
    """[boundary] with swboundary = surface, as far as the library covers it.

    mbcbot "noslip" (ubot, vbot) or "ustar" (ustar); sbcbot per scalar "dirichlet" | "flux" | "neumann" with sbot the value,
    flux or gradient that set_bc fills in; z0m, z0h (uniform: swconstantz0); mbctop / sbctop / stop: the top conditions, used for
    the ghost cells. thermo: None = the case's (Thermo_buoy where the case says so, Thermo_dry with scalar 0 = th otherwise,
    "0" without scalars, Thermo_moist where the HotPath has thermo=Moist(...)), or "0" | "dry" | "buoy" | "moist". With "moist"
    scalar 0 is thl, scalar 1 is qt, both with the same kind of bottom bc, and the kernels read thvref, thvrefh at kstart from the
    device tables the base state writes.

    bind() raises on what the library refuses: swconstantz0 = False (the iterative solvers), swcharnock, igc < 2 or jgc < 2.
    """

    def __init__(self, mbcbot="noslip", ubot=0., vbot=0., ustar=None, sbcbot="flux", sbot=0., z0m=0.1, z0h=0.1,
                 mbctop="freeslip", utop=0., vtop=0., sbctop="neumann", stop=0., thermo=None, thref_kstart=300., threfh_kstart=300., bg_n2=0.,
                 swconstantz0=True, swcharnock=False):
        if mbcbot not in MBC or mbctop not in MBCTOP:
            raise ValueError("mbcbot: noslip | ustar; mbctop: noslip | freeslip | neumann")
        if mbcbot == "ustar" and ustar is None:
            raise ValueError("mbcbot = ustar needs ustar")
        if thermo not in (None, "0", "dry", "buoy", "moist"):
            raise ValueError("thermo: 0 | dry | buoy | moist")
        self.mbcbot, self.ubot, self.vbot, self.ustar_in = mbcbot, ubot, vbot, ustar
        self.sbcbot, self.sbot_in, self.z0m, self.z0h = sbcbot, sbot, z0m, z0h
        self.mbctop, self.utop, self.vtop, self.sbctop, self.stop_in = mbctop, utop, vtop, sbctop, stop
        self.thermo, self.thref_kstart, self.threfh_kstart, self.bg_n2 = thermo, thref_kstart, threfh_kstart, bg_n2
        self.swconstantz0, self.swcharnock = swconstantz0, swcharnock

    # -- made once per HotPath -------------------------------------------------------------------------------------
    def bind(self, hp):
        torch, g = hp.torch, hp.grid
        if not self.swconstantz0:
            raise ValueError("swconstantz0 = False: the iterative Obukhov-length solvers are not built, only the lookup solver")
        if self.swcharnock:
            raise ValueError("swcharnock: the Charnock roughness update is not built")
        if g.igc < 2 or g.jgc < 2:
            raise ValueError("the surface layer needs igc >= 2 and jgc >= 2: calc_dutot reads u[i+2] and v[j+2]")
        if hp.cfg["order"] != 2:
            raise ValueError("the surface layer runs with the second-order cases (swspatialorder = 2)")
        self.hp = hp
        ns = self.ns = len(hp.s)
        n2 = g.shape2
        moist = getattr(hp, "thermo", None)
        thermo = self.thermo if self.thermo is not None else ("0" if ns == 0 else "moist" if moist is not None else
                                                              "buoy" if hp.cfg.get("thermo") == "buoy" else "dry")
        if thermo != "0" and ns == 0:
            raise ValueError("thermo = %s needs scalar 0 (th or b)" % thermo)
        self.kind = {"0": 0, "dry": 1, "buoy": 2, "moist": 3}[thermo]
        bcs = [SBC[b] for b in _per_scalar(self.sbcbot, ns, "sbcbot")]
        if self.kind == 3:
            if moist is None or ns < 2:
                raise ValueError("thermo = moist needs HotPath(..., thermo=Moist(...)) and the scalars 0 = thl, 1 = qt")
            if bcs[1] != bcs[0]:
                raise ValueError("thermo = moist: qt has another kind of bottom bc than thl (sbcbot %s): the buoyancy flux and the "
                                 "surface buoyancy need both scalars' fluxes or both surface values" % (self.sbcbot,))
        self.bctop = [SBC[b] for b in _per_scalar(self.sbctop, ns, "sbctop")]
        vals, tops = _per_scalar(self.sbot_in, ns, "sbot"), _per_scalar(self.stop_in, ns, "stop")
        mbc = MBC[self.mbcbot]
        if self.kind and not (bcs[0] == FLUX or (bcs[0] == DIRICHLET and mbc == DIRICHLET)):
            raise ValueError("thermo bc: flux, or dirichlet with mbcbot = noslip (the cases of Boundary_surface's stability)")

        def full(v=0.):
            return torch.full(n2, float(v), device=hp.device, dtype=hp.td)
        # init_surface (src/boundary_surface.cxx:537-574) and set_values / set_ustar (:748-809)
        self.obuk, self.ustar = full(1e-9), full(1e-2)
        if mbc == USTAR:
            self.ustar.fill_(max(0.0001, float(self.ustar_in)))
        self.nobuk = torch.zeros(n2, device=hp.device, dtype=torch.int32)
        self.z0m_t, self.z0h_t = hp.surf["z0m"], full(self.z0h)
        self.z0m_t.fill_(float(self.z0m))
        self.ubot_t, self.vbot_t, self.ugradbot, self.vgradbot = full(self.ubot), full(self.vbot), full(), full()
        self.utop_t, self.vtop_t = full(self.utop), full(self.vtop)          # value (noslip) or gradient (freeslip) at the top
        self.dutot = full()
        # one bottom value / gradient / flux per scalar (set_bc, include/boundary_surface_kernels.h:37-75), and the top condition
        self.sbot = [full(v if b == DIRICHLET else 0.) for v, b in zip(vals, bcs)]
        self.sgradbot = [full(v if b == NEUMANN else 0.) for v, b in zip(vals, bcs)]
        self.sfluxbot = [full(v if b == FLUX else 0.) for v, b in zip(vals, bcs)]
        self.stop = [full(v) for v in tops]
        for n in range(ns):
            hp.fields.s_fluxbot[n] = self.sfluxbot[n].data_ptr()
        # init_solver (:812-826): the table on the host with the host C library
        zL, f = np.zeros(NZL, dtype=np.float32), np.zeros(NZL, dtype=np.float32)
        zsl = float(g.z[g.kstart])
        capi.check(hp.lib.mhh_surface_lut_host(zsl, float(g.np_dtype.type(self.z0m)), float(g.np_dtype.type(self.z0h)), mbc,
                                               bcs[0] if self.kind else DIRICHLET, g.dtype, zL.ctypes.data, f.ctypes.data), hp.lib)
        self.zL, self.f = torch.from_numpy(zL).to(hp.device), torch.from_numpy(f).to(hp.device)
        self.params = p = MhhSurfaceParams()
        p.mbcbot, p.thermobc, p.thermo_kind, p.thermo_index = mbc, (bcs[0] if self.kind else 0), self.kind, 0
        p.swconstantz0, p.swcharnock = 1, 0
        p.thref_kstart, p.threfh_kstart, p.grav, p.bg_n2 = self.thref_kstart, self.threfh_kstart, GRAV, self.bg_n2
        for k, t in (("zL", self.zL), ("f", self.f), ("z0m", self.z0m_t), ("z0h", self.z0h_t), ("ustar", self.ustar), ("obuk", self.obuk),
                     ("nobuk", self.nobuk), ("ubot", self.ubot_t), ("vbot", self.vbot_t), ("ugradbot", self.ugradbot), ("vgradbot", self.vgradbot)):
            setattr(p, k, t.data_ptr())
        for n in range(ns):
            p.sbot[n], p.sgradbot[n], p.sbcbot[n] = self.sbot[n].data_ptr(), self.sgradbot[n].data_ptr(), bcs[n]
        if self.kind == 3:
            p.qt_index, p.thvref, p.thvrefh = 1, moist.tab["thvref"].data_ptr(), moist.tab["thvrefh"].data_ptr()
        self.bcs, self.mbc = bcs, mbc
        return self

    # -- per sub-step ---------------------------------------------------------------------------------------------
    def _call(self, name, *args):
        hp = self.hp
        capi.check(getattr(hp.lib, name)(hp.G, C.byref(hp.fields), C.byref(self.params), *args, hp.stream), hp.lib)

    def exec(self):
        """boundary->exec (src/model.cxx:374): one rank, the fused call; a slab, the stages with the north-south rows of dutot,
        ufluxbot and vfluxbot exchanged between them (nobuk stays per rank: a ghost row walks from its own history, which is its
        image's)."""
        hp = self.hp
        if not hp.slab:
            self._call("mhh_boundary_surface_exec", self.dutot.data_ptr())
            return
        self._call("mhh_surface_dutot", self.dutot.data_ptr())
        hp._halo2d(self.dutot)
        self._call("mhh_surface_stability", self.dutot.data_ptr())
        self._call("mhh_surface_momentum")
        hp._halo2d(hp.surf["u_fluxbot"]); hp._halo2d(hp.surf["v_fluxbot"])
        for n in range(self.ns):
            self._call("mhh_surface_scalar", n)
        self._call("mhh_surface_mo_gradients")

    def staged(self):
        """The same as separate stage calls with the cyclic fills between them (tests; one rank)."""
        hp, d = self.hp, self.dutot.data_ptr()
        fill = lambda t: capi.check(hp.lib.mhh_boundary_cyclic_2d(hp.G, t.data_ptr(), hp.stream), hp.lib)      # noqa: E731
        self._call("mhh_surface_dutot", d); fill(self.dutot)
        self._call("mhh_surface_stability", d)
        self._call("mhh_surface_momentum"); fill(hp.surf["u_fluxbot"]); fill(hp.surf["v_fluxbot"])
        for n in range(self.ns):
            self._call("mhh_surface_scalar", n)
        self._call("mhh_surface_mo_gradients")

    def ghost_cells(self):
        """boundary->set_ghost_cells (src/model.cxx:375; src/boundary.cxx:919-948): u and v from mbcbot (noslip: the surface value;
        ustar: the reference's kernels match neither branch and leave the level alone), a scalar from its surface value (dirichlet)
        or from the gradient surfs has just written (flux, neumann); the top from mbctop / sbctop."""
        hp = self.hp
        mb = 0 if self.mbc == DIRICHLET else -1
        mt = 0 if MBCTOP[self.mbctop] == DIRICHLET else 1
        gc = hp.lib.mhh_boundary_ghost_cells
        for a, bot, grad, top in ((hp.u, self.ubot_t, self.ugradbot, self.utop_t), (hp.v, self.vbot_t, self.vgradbot, self.vtop_t)):
            capi.check(gc(hp.G, 2, a.data_ptr(), mb, mt, bot.data_ptr(), grad.data_ptr(), top.data_ptr(), top.data_ptr(), hp.stream), hp.lib)
        for n in range(self.ns):
            sb = 0 if self.bcs[n] == DIRICHLET else 1
            st = 0 if self.bctop[n] == DIRICHLET else 1
            capi.check(gc(hp.G, 2, hp.s[n].data_ptr(), sb, st, self.sbot[n].data_ptr(), self.sgradbot[n].data_ptr(),
                          self.stop[n].data_ptr(), self.stop[n].data_ptr(), hp.stream), hp.lib)

    def outputs(self):
        """Every 2-D array the surface layer writes, by name (host copies)."""
        hp = self.hp
        out = {"dutot": self.dutot, "ustar": self.ustar, "obuk": self.obuk, "nobuk": self.nobuk, "ugradbot": self.ugradbot, "vgradbot": self.vgradbot,
               "ufluxbot": hp.surf["u_fluxbot"], "vfluxbot": hp.surf["v_fluxbot"], "dudz": hp.surf["dudz"], "dvdz": hp.surf["dvdz"], "dbdz": hp.surf["dbdz"]}
        for n in range(self.ns):
            out["sbot%d" % n], out["sgradbot%d" % n], out["sfluxbot%d" % n] = self.sbot[n], self.sgradbot[n], self.sfluxbot[n]
        return {k: t.detach().cpu().numpy().copy() for k, t in out.items()}
