"""Radiation_gcss on the host side: the driver of csrc/radiation_gcss.h behind HotPath(..., radiation=Gcss(...)).

swradiation = gcss (src/radiation_gcss.cxx) is the parameterised long- and short-wave flux of the DYCOMS-II stratocumulus case: the
long-wave flux from the liquid water path below and above each level plus a term above the inversion, the short-wave flux from a
two-stream solution over the cloud's optical depth, and thl's tendency from their vertical difference. It needs ql, which is
Thermo_moist's saturation adjustment of thl and qt. The parity target is the reference's CPU path.
"""
import ctypes as C

import numpy as np

from . import capi

LW, SW = 1, 2
FIELDS = ("lflx", "sflx")


def dycoms_profiles(z, zi=840.):
    """The DYCOMS-II RF01 initial profiles (Stevens et al. 2005, Mon. Wea. Rev. 133, 1443-1462): a well-mixed layer of thl = 289 K
    and qt = 9 g/kg under an inversion at zi, above it thl = 297.5 + (z - zi)^(1/3) K and qt = 1.5 g/kg. Returns thl [K], qt [kg/kg]."""
    z = np.asarray(z, dtype=np.float64)
    below = z < zi
    return np.where(below, 289.0, 297.5 + np.cbrt(np.maximum(z - zi, 0.))), np.where(below, 9.0e-3, 1.5e-3)


def synthetic_stratocumulus(z, n3, rs, zi=840., depth=250.):
    """A synthetic stratocumulus state on n3 = (ktot, jtot, itot) cells at the heights z, drawn from the numpy generator rs: the
    profiles of dycoms_profiles with the inversion at zi +- 60 m per column, noise of +-0.05 K and +-0.05 g/kg, and in four columns
    out of five qt raised by 0.5 to 1.5 g/kg in the `depth` metres below the inversion. The mixed layer's qt alone saturates its
    upper part; the raised band holds ql of 1e-4 and more (well above the 1e-5 of the optical depth). Returns thl [K] and qt [kg/kg]."""
    z3 = np.asarray(z, dtype=np.float64)[:, None, None]
    n2 = (1,) + tuple(n3[1:])
    top = zi + 60.*(2.*rs.random_sample(n2) - 1.)
    cloudy = rs.random_sample(n2) < 0.8
    thl, qt = dycoms_profiles(z3, top)
    thl = thl + 0.1*(rs.random_sample(n3) - 0.5)
    qt = qt + 1.e-4*(rs.random_sample(n3) - 0.5)
    band = (z3 < top) & (z3 > top - depth) & cloudy
    qt = qt + np.where(band, 0.5e-3 + 1.0e-3*rs.random_sample(n2), 0.)
    return thl, qt


class Gcss:
    """Radiation_gcss for HotPath(..., thermo=Moist(pbot), radiation=Gcss(xka, fr0, fr1, div, lat, lon, day_of_year)).

    xka, fr0, fr1, div: radiation.xka, fr0, fr1, div of the .ini file. lat, lon [degrees]: grid.lat, grid.lon. day_of_year: what
    Timeloop::calc_day_of_year gives, the day of the year counted from 1 plus the fraction of the day (2001-06-09 00:00 UTC: 160.0).
    parts: the terms thl's tendency takes, LW | SW by default.

    `mu`, the cosine of the zenith angle, is a host number (mhh_radiation_gcss_zenith_host, the host's C library in the grid's
    dtype): a captured step holds the value it was captured with; set_time() and capture again when the sun has moved.
    Per sub-step (src/model.cxx:372): exec() between microphys->exec and boundary->exec. Column-local: a slab rank exchanges nothing."""

    def __init__(self, xka, fr0, fr1, div, lat, lon, day_of_year, parts=LW | SW):
        if not parts or parts & ~(LW | SW):
            raise ValueError("parts: LW, SW or LW | SW")
        self.xka, self.fr0, self.fr1, self.div = float(xka), float(fr0), float(fr1), float(div)
        self.lat, self.lon, self.day_of_year, self.parts = float(lat), float(lon), float(day_of_year), int(parts)
        self.mu = None

    def bind(self, hp):
        from .thermo import Moist
        if not isinstance(hp.thermo, Moist):
            raise ValueError("radiation=Gcss needs thermo=Moist(pbot): ql is Thermo_moist's saturation adjustment of thl and qt")
        self.hp = hp
        g, torch = hp.grid, hp.torch
        self.scratch = torch.zeros((2, g.ncells), device=hp.device, dtype=hp.td)
        self.scratch_ptrs = (C.c_void_p*2)(*[self.scratch[n].data_ptr() for n in range(2)])
        self.set_time(self.day_of_year)
        return self

    def set_time(self, day_of_year):
        """calc_zenith (src/radiation_gcss.cxx:39-76) for the day of the year (with its fraction): sets and returns mu."""
        hp = self.hp
        mu = C.c_double(0)
        capi.check(hp.lib.mhh_radiation_gcss_zenith_host(hp.grid.dtype, self.lat, self.lon, float(day_of_year), C.byref(mu)), hp.lib)
        self.day_of_year, self.mu = float(day_of_year), mu.value
        return self.mu

    @property
    def daytime(self):
        t = self.hp.grid.np_dtype.type
        return bool(t(self.mu) > t(0.035))

    def _call(self, thlt, lflx, sflx, impl=None):
        hp, th = self.hp, self.hp.thermo
        p = capi.MhhRadiationGcssParams(self.xka, self.fr0, self.fr1, self.div, self.mu, self.parts)
        a = [thlt, None, hp.s[0].data_ptr(), hp.s[1].data_ptr(), hp.rhoref.data_ptr(), th.tab["pref"].data_ptr(), th.tab["exnref"].data_ptr(),
             lflx, sflx, self.scratch_ptrs, th.nonconv.data_ptr(), hp.stream]
        if impl is None:
            capi.check(hp.lib.mhh_radiation_gcss_exec(hp.G, C.byref(p), *a), hp.lib)
        else:
            capi.check(hp.lib.mhh_radiation_gcss_exec_impl(hp.G, int(impl), C.byref(p), *a), hp.lib)

    # -- per sub-step ------------------------------------------------------------------------------------------------
    def exec(self, impl=None):
        """Radiation_gcss::exec (src/radiation_gcss.cxx:353-379); impl names a form of the A/B (capi: 0 sweep, 1 plain)."""
        self._call(self.hp.st[0].data_ptr(), None, None, impl)

    # -- diagnostics -------------------------------------------------------------------------------------------------
    def fields(self, impl=None):
        """get_radiation_field for "lflx" and "sflx" (:392-436) as new device tensors; sflx is all zero at night."""
        hp, g = self.hp, self.hp.grid
        out = {n: hp.torch.zeros(g.shape3, device=hp.device, dtype=hp.td) for n in FIELDS}
        self._call(None, out["lflx"].data_ptr(), out["sflx"].data_ptr(), impl)
        return out

    def field(self, name):
        """get_radiation_field(name): other names than lflx and sflx are refused."""
        if name not in FIELDS:
            raise ValueError("get_radiation_field: %r is not one of %s" % (name, " | ".join(FIELDS)))
        return self.fields()[name]
