"""Microphys_2mom_warm, Microphys_nsw6 and Limiter on the host side: the drivers of csrc/microphys_2mom_warm.h and csrc/microphys_nsw6.h
behind HotPath(..., micro=Warm2mom(Nc0)) and HotPath(..., micro=Nsw6(Nc0)).

swmicro = 2mom_warm (src/microphys_2mom_warm.cxx: Seifert & Beheng 2006 warm rain, Stevens & Seifert 2008 sedimentation) carries two
more scalars beside Thermo_moist's thl and qt: qr, the rain water specific humidity, and nr, the number density of rain drops. Every
case of the reference that uses it lists both in the limiter's limitlist, so Limiter::exec (src/limiter.cxx) lives here too.
"""
import ctypes as C

import numpy as np

from . import capi

AUTO, ACCR, EVAP, SCBR, SEDI, CLIP = 1, 2, 4, 8, 16, 32
ALL = AUTO | ACCR | EVAP | SCBR | SEDI | CLIP
NAMES = ("thl", "qt", "qr", "nr")        # the scalars of a HotPath with micro=, in this order


def synthetic_rain(z, n3, rs, rho=1.1):
    """A synthetic rain field on n3 = (ktot, jtot, itot) cells drawn from the numpy generator rs: rain in about half of the columns,
    in about 70 % of their levels; qr between 1e-7 and 1e-3 kg/kg, nr such that the mean drop diameter lies between 0.06 and 2.3 mm
    (beyond both clamps of the mean drop mass). Returns qr [kg/kg] and nr [m-3]."""
    wet = (rs.random_sample((1,) + tuple(n3[1:])) < 0.5) & (rs.random_sample(n3) < 0.7)
    u = rs.random_sample(n3)
    qr = 1.e-7 + 1.e-3*u**4
    u = rs.random_sample(n3)
    dr = 6.e-5 + 2.2e-3*u*u
    nr = rho*qr/(np.pi*1.e3/6.*dr**3)
    return np.where(wet, qr, 0.), np.where(wet, nr, 0.)


class Warm2mom:
    """Microphys_2mom_warm for HotPath(..., thermo=Moist(pbot), micro=Warm2mom(Nc0)): scalar 0 is thl, 1 qt, 2 qr, 3 nr.

    Nc0: the fixed cloud droplet number [m-3] (micro.Nc0). cflmax: the largest sedimentation CFL number time_limit allows
    (micro.cflmax, 2 by default as in the reference). limit: the limiter's limitlist, names out of thl, qt, qr, nr. dt: the FULL time
    step sedimentation integrates over (timeloop->get_dt(), not the sub-step; default: the HotPath's dt); set `dt` again when the
    step changes. processes: the mask of the C ABI, everything by default.

    Per sub-step (src/model.cxx:369, :415): exec() right behind thermo->exec -- remove_negative_values on qr and nr, the tendencies of
    the four scalars, the surface rain rate -- and limit() behind the pressure solve with the sub-step. Everything is column-local:
    a slab rank exchanges nothing, only time_limit's maximum goes through Master."""

    def __init__(self, Nc0, cflmax=2., limit=("qr", "nr"), dt=None, processes=ALL):
        if not Nc0 > 0.:
            raise ValueError("Nc0 must be positive (micro.Nc0 has no default in the reference)")
        bad = [n for n in limit if n not in NAMES]
        if bad:
            raise ValueError("limit: %r is not one of %s" % (bad[0], ", ".join(NAMES)))
        self.Nc0, self.cflmax, self.limitlist, self.dt, self.processes = float(Nc0), float(cflmax), tuple(limit), dt, int(processes)

    def bind(self, hp):
        from .thermo import Moist
        if not isinstance(hp.thermo, Moist):
            raise ValueError("micro=Warm2mom needs thermo=Moist(pbot): ql is Thermo_moist's saturation adjustment of thl and qt")
        if len(hp.s) != 4:
            raise ValueError("micro=Warm2mom needs four scalars, 0 = thl, 1 = qt, 2 = qr, 3 = nr: this HotPath carries %d" % len(hp.s))
        self.hp = hp
        g, torch = hp.grid, hp.torch
        if self.dt is None:
            self.dt = float(hp.dt)
        self.rr_bot = torch.zeros(g.shape2, device=hp.device, dtype=hp.td)
        self.scratch = torch.zeros((4, g.ncells), device=hp.device, dtype=hp.td)
        self.scratch_ptrs = (C.c_void_p*4)(*[self.scratch[n].data_ptr() for n in range(4)])
        return self

    # -- per sub-step ------------------------------------------------------------------------------------------------
    def exec(self, impl=None):
        """Microphys_2mom_warm::exec (src/microphys_2mom_warm.cxx:639-752); impl names a form of the A/B (capi: 0 marching, 1 cell)."""
        hp, th = self.hp, self.hp.thermo
        p = capi.MhhMicroParams(self.Nc0, float(self.dt), self.processes)
        a = [hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.s[0].data_ptr(), hp.s[1].data_ptr(),
             hp.st[2].data_ptr(), hp.st[3].data_ptr(), hp.st[0].data_ptr(), hp.st[1].data_ptr(), self.rr_bot.data_ptr(),
             hp.rhoref.data_ptr(), th.tab["pref"].data_ptr(), th.tab["exnref"].data_ptr(), self.scratch_ptrs, th.nonconv.data_ptr(), hp.stream]
        if impl is None:
            capi.check(hp.lib.mhh_micro_2mom_warm_exec(hp.G, C.byref(p), *a), hp.lib)
        else:
            capi.check(hp.lib.mhh_micro_2mom_warm_exec_impl(hp.G, int(impl), C.byref(p), *a), hp.lib)

    def limit(self, dt=None):
        """Limiter::exec (src/limiter.cxx:78-94) with the sub-step dt (default: the HotPath's dt) for every name of the limitlist."""
        hp = self.hp
        for name in self.limitlist:
            n = NAMES.index(name)
            capi.check(hp.lib.mhh_limiter_exec(hp.G, hp.st[n].data_ptr(), hp.s[n].data_ptr(), float(hp.dt if dt is None else dt), hp.stream), hp.lib)

    # -- outside the sub-step ----------------------------------------------------------------------------------------
    def cfl(self, dt):
        """calc_max_sedimentation_cfl for the step dt, the maximum over the ranks."""
        hp = self.hp
        out = C.c_double(0)
        capi.check(hp.lib.mhh_micro_2mom_warm_cfl(hp.G, hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.rhoref.data_ptr(), float(dt), hp.work.data_ptr(),
                                                  C.byref(out), hp.stream), hp.lib)
        return hp.master.max(out.value)

    def time_limit(self, idt, dt):
        """Microphys_2mom_warm::get_time_limit (:965-982): idt * cflmax / cfl in the grid's dtype, truncated to an integer."""
        t = self.hp.grid.np_dtype.type
        return int(t(idt) * t(self.cflmax) / t(self.cfl(dt)))

    def rain_rate(self):
        """get_surface_rain_rate: rr_bot [kg m-2 s-1], the device tensor of the grid's 2-D shape (interior written by exec)."""
        return self.rr_bot


# ---- Microphys_nsw6 -----------------------------------------------------------------------------------------------------------
NSW6_CONV, NSW6_SEDI_R, NSW6_SEDI_S, NSW6_SEDI_G = 1, 2, 4, 8
NSW6_ALL = NSW6_CONV | NSW6_SEDI_R | NSW6_SEDI_S | NSW6_SEDI_G
NSW6_POW, NSW6_SQRT = 0, 1               # the two forms of the powers (include/mhh_hip.h)
NSW6_NAMES = ("thl", "qt", "qr", "qs", "qg")     # the scalars of a HotPath with micro=Nsw6, in this order


def synthetic_precip(z, n3, rs):
    """Synthetic rain, snow and graupel for a deep, mixed-phase domain on n3 = (ktot, jtot, itot) cells at the heights z [m], drawn
    from the numpy generator rs: each species in about half of the columns and about 70 % of the levels of its layer (rain below
    6 km, snow between 3 and 14 km, graupel between 2 and 12 km), between 1e-7 and 2e-3 kg/kg. Returns qr, qs, qg [kg/kg]."""
    z3 = np.asarray(z, dtype=np.float64)[:, None, None]
    out = []
    for lo, hi in ((0., 6000.), (3000., 14000.), (2000., 12000.)):
        wet = (rs.random_sample((1,) + tuple(n3[1:])) < 0.5) & (rs.random_sample(n3) < 0.7) & (z3 >= lo) & (z3 <= hi)
        u = rs.random_sample(n3)
        out.append(np.where(wet, 1.e-7 + 2.e-3*u**4, 0.))
    return out


class Nsw6:
    """Microphys_nsw6 for HotPath(..., thermo=Moist(pbot), micro=Nsw6(Nc0)): scalar 0 is thl, 1 qt, 2 qr, 3 qs, 4 qg.

    Nc0: the fixed cloud droplet number [m-3] (micro.Nc0). cflmax: the largest sedimentation CFL number time_limit allows
    (micro.cflmax, 1.2 by default as in the reference). limit: the limiter's limitlist, names out of thl, qt, qr, qs, qg (cases/rcemip
    lists qt, qr, qs, qg). dt: the FULL time step conversion's limits and sedimentation use (timeloop->get_dt(), not the sub-step;
    default: the HotPath's dt); set `dt` again when the step changes. processes: the mask of the C ABI, everything by default. impl:
    the form of the powers (NSW6_POW, NSW6_SQRT; None: the library's default).

    Per sub-step (src/model.cxx:369, :415): exec() right behind thermo->exec -- the tendencies of the five scalars from conversion
    (ql and qi by sat_adjust inline) and from the sedimentation of the three species, the three surface rates -- and limit() behind
    the pressure solve with the sub-step. Everything is column-local: a slab rank exchanges nothing, only time_limit's maximum goes
    through Master."""

    def __init__(self, Nc0, cflmax=1.2, limit=("qt", "qr", "qs", "qg"), dt=None, processes=NSW6_ALL, impl=None):
        if not Nc0 > 0.:
            raise ValueError("Nc0 must be positive (micro.Nc0 has no default in the reference)")
        bad = [n for n in limit if n not in NSW6_NAMES]
        if bad:
            raise ValueError("limit: %r is not one of %s" % (bad[0], ", ".join(NSW6_NAMES)))
        if impl not in (None, NSW6_POW, NSW6_SQRT):
            raise ValueError("impl: NSW6_POW, NSW6_SQRT or None")
        self.Nc0, self.cflmax, self.limitlist, self.dt, self.processes, self.impl = float(Nc0), float(cflmax), tuple(limit), dt, int(processes), impl

    def bind(self, hp):
        from .thermo import Moist
        if not isinstance(hp.thermo, Moist):
            raise ValueError("micro=Nsw6 needs thermo=Moist(pbot): ql and qi are Thermo_moist's saturation adjustment of thl and qt")
        if len(hp.s) != 5:
            raise ValueError("micro=Nsw6 needs five scalars, 0 = thl, 1 = qt, 2 = qr, 3 = qs, 4 = qg: this HotPath carries %d" % len(hp.s))
        self.hp = hp
        g, torch = hp.grid, hp.torch
        if self.dt is None:
            self.dt = float(hp.dt)
        self.bot = torch.zeros((3,) + tuple(g.shape2), device=hp.device, dtype=hp.td)
        self.scratch = torch.zeros((6, g.ncells), device=hp.device, dtype=hp.td)
        self.scratch_ptrs = (C.c_void_p*6)(*[self.scratch[n].data_ptr() for n in range(6)])
        return self

    # -- per sub-step ------------------------------------------------------------------------------------------------
    def exec(self, impl=None):
        """Microphys_nsw6::exec (src/microphys_nsw6.cxx:983-1073); impl names a form of the A/B (default: the object's)."""
        hp, th = self.hp, self.hp.thermo
        impl = self.impl if impl is None else impl
        p = capi.MhhMicroParams(self.Nc0, float(self.dt), self.processes)
        a = [hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.s[4].data_ptr(), hp.s[0].data_ptr(), hp.s[1].data_ptr(), None, None,
             hp.st[2].data_ptr(), hp.st[3].data_ptr(), hp.st[4].data_ptr(), hp.st[0].data_ptr(), hp.st[1].data_ptr(),
             self.bot[0].data_ptr(), self.bot[1].data_ptr(), self.bot[2].data_ptr(),
             hp.rhoref.data_ptr(), th.tab["pref"].data_ptr(), th.tab["exnref"].data_ptr(), self.scratch_ptrs, th.nonconv.data_ptr(), hp.stream]
        if impl is None:
            capi.check(hp.lib.mhh_micro_nsw6_exec(hp.G, C.byref(p), *a), hp.lib)
        else:
            capi.check(hp.lib.mhh_micro_nsw6_exec_impl(hp.G, int(impl), C.byref(p), *a), hp.lib)

    def limit(self, dt=None):
        """Limiter::exec (src/limiter.cxx:78-94) with the sub-step dt (default: the HotPath's dt) for every name of the limitlist."""
        hp = self.hp
        for name in self.limitlist:
            n = NSW6_NAMES.index(name)
            capi.check(hp.lib.mhh_limiter_exec(hp.G, hp.st[n].data_ptr(), hp.s[n].data_ptr(), float(hp.dt if dt is None else dt), hp.stream), hp.lib)

    # -- outside the sub-step ----------------------------------------------------------------------------------------
    def cfl(self, dt):
        """The largest of the three calc_cfl_ss08 for the step dt (at least 1e-5), the maximum over the ranks."""
        hp = self.hp
        out = C.c_double(0)
        a = [hp.s[2].data_ptr(), hp.s[3].data_ptr(), hp.s[4].data_ptr(), hp.rhoref.data_ptr(), float(dt), hp.work.data_ptr(), C.byref(out), hp.stream]
        if self.impl is None:
            capi.check(hp.lib.mhh_micro_nsw6_cfl(hp.G, *a), hp.lib)
        else:
            capi.check(hp.lib.mhh_micro_nsw6_cfl_impl(hp.G, int(self.impl), *a), hp.lib)
        return hp.master.max(out.value)

    def time_limit(self, idt, dt):
        """Microphys_nsw6::get_time_limit (:1119-1177): idt * cflmax in the grid's dtype over the CFL number, a double there,
        truncated to an integer."""
        t = self.hp.grid.np_dtype.type
        return int(float(t(idt) * t(self.cflmax)) / self.cfl(dt))

    def rain_rate(self):
        """rr_bot [kg m-2 s-1], the device tensor of the grid's 2-D shape (interior written by exec)."""
        return self.bot[0]

    def snow_rate(self):
        """rs_bot [kg m-2 s-1]."""
        return self.bot[1]

    def graupel_rate(self):
        """rg_bot [kg m-2 s-1]."""
        return self.bot[2]

    def surface_rate(self):
        """get_surface_rain_rate (:1194-1202): rain plus snow plus graupel, a new tensor."""
        return self.bot[0] + self.bot[1] + self.bot[2]
