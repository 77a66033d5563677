"""Thermo_moist on the host side: the BOMEX initial state and the base-state tables of libmhh_hip.so's moist thermodynamics.

The kernels (csrc/thermo_moist.h) take thl and qt and the eight base-state profiles; `base_state` builds those profiles with the
host entry, as Thermo_moist::create_basestate does (src/thermo_moist.cxx:1189-1247).
"""
import ctypes as C

import numpy as np

from . import capi

BASE_STATE = ("pref", "prefh", "rhoref", "rhorefh", "thvref", "thvrefh", "exnref", "exnrefh")


def bomex_profiles(z):
    """The published BOMEX initial profiles (Siebesma et al. 2003, J. Atmos. Sci. 60, 1201-1219): piecewise linear in z with breaks
    at 520, 1480, 2000 and 3000 m. Returns thl [K] and qt [kg/kg] at the heights z [m]."""
    zb = [0., 520., 1480., 2000., 3000.]
    z = np.asarray(z, dtype=np.float64)
    return np.interp(z, zb, [298.7, 298.7, 302.4, 308.2, 311.85]), np.interp(z, zb, [17.0e-3, 16.3e-3, 10.7e-3, 4.2e-3, 3.0e-3])


def rcemip_profiles(z):
    """Initial profiles for the deep-convection case (cases/rcemip): a troposphere of 15 km in which thl rises by 4 K/km from the
    surface value of rcemip.ini (about 6.5 K/km in temperature: the freezing level lies near 4.3 km, -40 C near 10 km), a
    stratosphere close to isothermal above, and qt falling off with a scale height of 2.8 km from 19 g/kg, at least 1e-6. Returns
    thl [K] and qt [kg/kg] at the heights z [m]."""
    z = np.asarray(z, dtype=np.float64)
    thl = np.where(z < 15000., 298.7438128523857 + 4.e-3*z, 358.7438128523857 + 17.e-3*(z - 15000.))
    return thl, np.maximum(19.e-3*np.exp(-z/2800.), 1.e-6)


def rcemip_interior(z, n3, rs):
    """The synthetic state of the deep-convection case: the profiles plus uniform noise of +-0.5 K and +-60 % of qt drawn from the
    numpy generator rs. Liquid-only cloud forms below the freezing level, mixed-phase cloud between it and -40 C, ice cloud above."""
    thl0, qt0 = rcemip_profiles(z)
    thl = thl0[:, None, None] + rs.uniform(-.5, .5, n3)
    qt = qt0[:, None, None]*(1. + rs.uniform(-.6, .6, n3))
    return thl, qt


def bomex_interior(z, n3, rs):
    """The one recipe of the synthetic BOMEX state: thl and qt on n3 = (ktot, jtot, itot) cells at the heights z, the initial profiles
    plus uniform noise of +-0.5 K and +-3e-3 kg/kg drawn from the numpy generator rs, qt clipped at 0. The profiles alone are
    unsaturated everywhere (the smallest deficit is about 0.9 g/kg near 590 m): the noise is what makes cloud. model.synthetic_global,
    HotPath's own start and bomex_synthetic all come here."""
    thl0, qt0 = bomex_profiles(z)
    thl = thl0[:, None, None] + rs.uniform(-.5, .5, n3)
    qt = np.maximum(qt0[:, None, None] + rs.uniform(-3e-3, 3e-3, n3), 0.)
    return thl, qt


def bomex_synthetic(g, seed=0):
    """bomex_interior on grid g as [kcells][jcells][icells] arrays in the grid's dtype: ghost levels repeat the nearest level,
    horizontal ghost cells wrap."""
    thl, qt = bomex_interior(g.z[g.kstart:g.kend], (g.kmax, g.jmax, g.imax), np.random.RandomState(seed))
    out = []
    for a in (thl, qt):
        a = np.concatenate([a[:1]]*g.kgc + [a] + [a[-1:]]*g.kgc, axis=0)
        a = np.pad(a, ((0, 0), (g.jgc, g.jgc), (g.igc, g.igc)), mode="wrap")
        out.append(np.ascontiguousarray(a, dtype=g.np_dtype))
    return out[0], out[1]


def base_state(lib, g, thl0, qt0, pbot, swbasestate="anelastic", thvref0=None):
    """The eight base-state profiles of Thermo_moist::create_basestate as host arrays in g's dtype, by mhh_thermo_moist_base_state_host.
    thl0, qt0: the ktot initial values; returned with their ghost entries set (calc_top_and_bot) beside the profiles."""
    if swbasestate not in ("anelastic", "boussinesq"):
        raise ValueError("swbasestate must be 'anelastic' or 'boussinesq' (src/thermo_moist.cxx:1026-1032)")
    if swbasestate == "boussinesq" and thvref0 is None:
        raise ValueError("swbasestate = 'boussinesq' needs thvref0 (src/thermo_moist.cxx:1232)")
    t = g.np_dtype
    prof = {}
    for name, a in (("thl0", thl0), ("qt0", qt0)):
        prof[name] = np.zeros(g.kcells, dtype=t)
        prof[name][g.kstart:g.kend] = np.asarray(a, dtype=t)
    for name in BASE_STATE:
        prof[name] = np.zeros(g.kcells, dtype=t)
    nonconv = C.c_int(0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)    # noqa: E731
    capi.check(lib.mhh_thermo_moist_base_state_host(g.host_struct(), ptr(prof["thl0"]), ptr(prof["qt0"]), float(pbot),
                                                    1 if swbasestate == "boussinesq" else 0, float(thvref0 or 0.),
                                                    *[ptr(prof[n]) for n in BASE_STATE], C.byref(nonconv)), lib)
    if nonconv.value:
        raise RuntimeError("Non-converging saturation adjustment in the base state (%d levels)" % nonconv.value)
    return prof


class Moist:
    """Thermo_moist for HotPath(..., thermo=Moist(pbot)): scalar 0 is thl, scalar 1 is qt, second order.

    bind(hp) builds the base state with the host entry (create_basestate), uploads the eight tables, hands rhoref / rhorefh to the
    dynamics once (fields.rhoref = bs.rhoref: never updated, src/thermo_moist.cxx:1243-1246) and owns the counter of cells on which
    the reference would have thrown "Non-converging saturation adjustment". Per sub-step (Thermo_moist::exec, :1273-1303): with
    swupdatebasestate the base state is recomputed on the device from the horizontal means of thl and qt -- all eight profiles, as the
    reference's call does, in the Boussinesq mode too -- and the buoyancy tendency is added to wt in front of the RHS pass.
    thl0, qt0: the ktot initial values the base state starts from (default: the BOMEX profiles on the grid's levels; those of
    rcemip_profiles for the case rcemip)."""

    FIELDS = ("b", "ql", "qi", "T", "N2", "ql_h")

    def __init__(self, pbot, swbasestate="anelastic", thvref0=None, swupdatebasestate=True, thl0=None, qt0=None):
        if swbasestate not in ("anelastic", "boussinesq"):
            raise ValueError("swbasestate must be 'anelastic' or 'boussinesq' (src/thermo_moist.cxx:1026-1032)")
        if swbasestate == "boussinesq" and thvref0 is None:
            raise ValueError("swbasestate = 'boussinesq' needs thvref0 (src/thermo_moist.cxx:1232)")
        self.pbot, self.swbasestate, self.thvref0, self.swupdate = float(pbot), swbasestate, thvref0, bool(swupdatebasestate)
        self.thl0, self.qt0 = thl0, qt0

    def bind(self, hp):
        torch, g = hp.torch, hp.grid
        if len(hp.s) < 2:
            raise ValueError("thermo=Moist needs two scalars, 0 = thl and 1 = qt: this HotPath carries %d" % len(hp.s))
        if hp.cfg["order"] != 2:
            raise ValueError("thermo=Moist is second order only: the reference's calc_buoyancy_tend_4th is never called "
                             "and does not match buoyancy's signature")
        if hp.cfg.get("thermo") == "buoy":
            raise ValueError("thermo=Moist on a Thermo_buoy case: scalar 0 is the buoyancy b there, not thl")
        self.hp = hp
        profiles = rcemip_profiles if hp.case == "rcemip" else bomex_profiles
        thl0, qt0 = (self.thl0, self.qt0) if self.thl0 is not None else profiles(g.z[g.kstart:g.kend])
        prof = base_state(hp.lib, g, thl0, qt0, self.pbot, self.swbasestate, self.thvref0)
        self.tab = {n: torch.from_numpy(prof[n].copy()).to(hp.device) for n in BASE_STATE}
        self.mean = [torch.from_numpy(prof[n].copy()).to(hp.device) for n in ("thl0", "qt0")]
        self.nonconv = torch.zeros(1, dtype=torch.int32, device=hp.device)
        self.scratch = torch.zeros(int(hp.lib.mhh_field_mean_scratch_elems(hp.G, 2)), device=hp.device, dtype=torch.float64)
        # the dynamics' density: set here once, before the pressure plan is made from it
        hp.rhoref_h, hp.rhorefh_h = prof["rhoref"].copy(), prof["rhorefh"].copy()
        hp.rhoref, hp.rhorefh = torch.from_numpy(hp.rhoref_h.copy()).to(hp.device), torch.from_numpy(hp.rhorefh_h.copy()).to(hp.device)
        return self

    def diff_params(self, p):
        """get_thermo_field("N2") inside exec_viscosity: calc_N2 (:460-475) is the dry expression with thvref for thref."""
        p.buoyancy_kind, p.buoyancy, p.th_for_N2, p.thref, p.grav = 0, 0, 0, self.tab["thvref"].data_ptr(), 9.81

    def _p(self, *names):
        return [self.tab[n].data_ptr() for n in names]

    # -- per sub-step ------------------------------------------------------------------------------------------------
    def means(self):
        """The horizontal means of thl and qt (fields->exec, src/model.cxx:351): Forcing's profiles where it evaluates both,
        otherwise one call of the same reduction here; on a slab the ranks' shares are summed through Master. Returns whether
        Forcing's evaluation was the one."""
        hp, fo = self.hp, self.hp.forcing
        if fo is not None and "s0" in fo.mean_names and "s1" in fo.mean_names:
            fo.means()
            self.mean = [fo.mean_prof["s0"], fo.mean_prof["s1"]]
            return True
        capi.check(hp.lib.mhh_field_mean_profile(hp.G, hp._ptrs(hp.s[:2]), 2, hp._ptrs(self.mean), self.scratch.data_ptr(), hp.stream), hp.lib)
        if hp.npy > 1:                   # a slab rank holds its share: summed over the ranks through Master, as Forcing's are
            both = hp.master.sum_(hp.torch.stack(self.mean))
            for t, s in zip(self.mean, both):
                t.copy_(s)
        return False

    def update_base_state(self, names=BASE_STATE):
        hp = self.hp
        ptrs = [self.tab[n].data_ptr() if n in names else None for n in BASE_STATE]
        capi.check(hp.lib.mhh_thermo_moist_base_state(hp.G, self.mean[0].data_ptr(), self.mean[1].data_ptr(), self.pbot, *ptrs,
                                                      self.nonconv.data_ptr(), hp.stream), hp.lib)

    def tend(self):
        hp = self.hp
        capi.check(hp.lib.mhh_thermo_moist_buoyancy_tend(hp.G, hp.wt.data_ptr(), hp.s[0].data_ptr(), hp.s[1].data_ptr(),
                                                         *self._p("prefh", "exnrefh", "thvrefh"), self.nonconv.data_ptr(), hp.stream), hp.lib)

    # -- diagnostics -------------------------------------------------------------------------------------------------
    def field(self, name):
        """Thermo_moist::get_thermo_field for b | ql | qi | T | N2 | ql_h, as a new device tensor; with swupdatebasestate the pressure and
        Exner profiles are refreshed from the current means first (:1418-1432). Other names are refused."""
        if name not in self.FIELDS:
            raise ValueError("get_thermo_field: %r is not one of %s" % (name, " | ".join(self.FIELDS)))
        hp, g = self.hp, self.hp.grid
        out = hp.torch.zeros(g.shape3, device=hp.device, dtype=hp.td)
        if self.swupdate:
            self.means()
            self.update_base_state(("pref", "prefh", "exnref", "exnrefh"))
        if name == "N2":
            capi.check(hp.lib.mhh_calc_N2(hp.G, out.data_ptr(), hp.s[0].data_ptr(), self.tab["thvref"].data_ptr(), 9.81, hp.stream), hp.lib)
            return out
        if name == "ql_h":               # calc_liquid_water_h (:368-411): the half levels kstart .. kend
            capi.check(hp.lib.mhh_thermo_moist_ql_h(hp.G, hp.s[0].data_ptr(), hp.s[1].data_ptr(), *self._p("prefh", "exnrefh"), out.data_ptr(),
                                                    self.nonconv.data_ptr(), hp.stream), hp.lib)
            return out
        ptrs = [out.data_ptr() if n == name else None for n in ("b", "ql", "qi", "T")]
        capi.check(hp.lib.mhh_thermo_moist_fields(hp.G, hp.s[0].data_ptr(), hp.s[1].data_ptr(), *self._p("pref", "exnref", "thvref"), *ptrs,
                                                  self.nonconv.data_ptr(), hp.stream), hp.lib)
        return out

    def check(self):
        """Synchronises and raises where the reference would have thrown; step() never calls it."""
        self.hp.sync()
        n = int(self.nonconv.cpu()[0])
        if n:
            raise RuntimeError("Non-converging saturation adjustment on %d cells since the last check" % n)
