"""Source and Decay on the host side: the drivers of csrc/source_decay.h behind HotPath(..., source=Sources([...]), decay=Decay({...})).

Sources: point and line releases of passive tracers and emission inventories whose sources share vertical emission profiles
(src/source.cxx). A source is a dict with the reference's namelist names: scalar (index of the target among the HotPath's scalars),
x0, y0, z0, sigma_x, sigma_y, sigma_z, and optionally line_x, line_y, line_z (0), strength (1), swvmr (False) and profile_index
(None). The emission profiles are an array [nprofiles][kcells] (what Source::create reads from the NetCDF input; the reading is
the caller's). Binding runs Source::create on the host inside the library; a sub-step's exec() is ONE launch for all sources of all
scalars. update() moves sources or changes their strength between steps: what Source::exec does under swtimedep_location and
swtimedep_strength, with the time interpolation of Timedep left to the caller.

Decay: st -= s/max(timescale, dt_sub) for the scalars named (src/decay.cxx), one launch for all of them.

A sub-step calls decay then source after Buffer and in front of Force (src/model.cxx:395-404).
"""
import ctypes as C

import numpy as np

from . import capi

KEYS = ("x0", "y0", "z0", "sigma_x", "sigma_y", "sigma_z", "line_x", "line_y", "line_z", "strength")
DEFAULTS = {"line_x": 0., "line_y": 0., "line_z": 0., "strength": 1., "sigma_z": 1., "z0": 0.}


def descs(sources):
    """The mhh_source_desc table of a list of source dicts."""
    tab = (capi.MhhSourceDesc * max(1, len(sources)))()
    for d, s in zip(tab, sources):
        unknown = set(s) - set(KEYS) - {"scalar", "swvmr", "profile_index"}
        if unknown:
            raise ValueError("source: unknown key(s) " + ", ".join(sorted(unknown)))
        d.scalar, d.swvmr = int(s["scalar"]), int(bool(s.get("swvmr", False)))
        d.profile_index = -1 if s.get("profile_index") is None else int(s["profile_index"])
        for k in KEYS:
            setattr(d, k, float(s[k] if k in s else DEFAULTS[k]))
    return tab


class Handle:
    """An mhh_source handle of `lib`: create, the accessors, update, exec, destroy."""

    def __init__(self, lib, grid, sources, profiles, rhoref, stream=None):
        self.lib, self.grid, self.n = lib, grid, len(sources)
        t = grid.np_dtype
        prof = np.zeros((0, grid.kcells), dtype=t) if profiles is None else np.ascontiguousarray(profiles, dtype=t)
        if prof.ndim != 2 or prof.shape[1] != grid.kcells:
            raise ValueError("emission profiles: an array [nprofiles][kcells = %d]" % grid.kcells)
        rho = np.ascontiguousarray(rhoref, dtype=t)
        if rho.shape != (grid.kcells,):
            raise ValueError("rhoref holds kcells = %d elements" % grid.kcells)
        self.h = C.c_void_p()
        capi.check(lib.mhh_source_create(grid.host_struct(), descs(sources), self.n, prof.ctypes.data if prof.size else None, prof.shape[0],
                                         rho.ctypes.data, stream, C.byref(self.h)), lib)

    def ranges(self, n):
        """(range_x, range_y, range_z) of source n as six array indices of this rank."""
        r = (C.c_int * 6)()
        capi.check(self.lib.mhh_source_ranges(self.h, n, r), self.lib)
        return tuple(r)

    def norm(self, n):
        v = C.c_double(0)
        capi.check(self.lib.mhh_source_norm(self.h, n, C.byref(v)), self.lib)
        return v.value

    @property
    def tiles(self):
        return int(self.lib.mhh_source_tiles(self.h))

    def update(self, n=None, x0=None, y0=None, z0=None, strength=None, stream=None):
        """New centre and / or strength of source n (scalars), or of every source (n = None: sequences of all sources)."""
        count = 1 if n is not None else self.n

        def arr(v):
            if v is None:
                return None
            a = (C.c_double * count)(*np.atleast_1d(np.asarray(v, dtype=np.float64)))
            return a
        capi.check(self.lib.mhh_source_update(self.h, -1 if n is None else int(n), arr(x0), arr(y0), arr(z0), arr(strength), stream), self.lib)

    def exec(self, G, fields, stream=None):
        capi.check(self.lib.mhh_source_exec(self.h, G, C.byref(fields), stream), self.lib)

    def close(self):
        if self.h:
            self.lib.mhh_source_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sources:
    def __init__(self, sources, profiles=None):
        self.sources, self.profiles = [dict(s) for s in sources], profiles

    def bind(self, hp):
        self.hp = hp
        for s in self.sources:
            if not 0 <= int(s["scalar"]) < len(hp.s):
                raise ValueError("source: scalar %d of %d" % (int(s["scalar"]), len(hp.s)))
        self.handle = Handle(hp.lib, hp.grid, self.sources, self.profiles, hp.rhoref_h, hp.stream)
        return self

    def exec(self):
        """source->exec (src/model.cxx:401): one launch."""
        self.handle.exec(self.hp.G, self.hp.fields, self.hp.stream)

    def update(self, n=None, x0=None, y0=None, z0=None, strength=None):
        """Host work between steps. A graph captured before it holds the old tables' address and launch size, so every graph of
        hp.capture_step() is reset first: replaying one raises; capture again after the update."""
        self.hp.drop_graphs()
        self.handle.update(n, x0, y0, z0, strength, self.hp.stream)

    def norm(self, n):
        return self.handle.norm(n)

    def ranges(self, n):
        return self.handle.ranges(n)


class Decay:
    """Decay({scalar: timescale}, nstd_couvreux=1., names=None): swdecay = exponential for those scalars (src/decay.cxx:66-88). A
    scalar is an index, "th" (0), "s<N>", or a name that `names` maps to an index -- the HotPath's scalars carry no names of their own:
    Decay({"couvreux": 600.}, names={"couvreux": 2}). A scalar called couvreux makes the `couvreux` mask of Decay::get_mask
    (:123-187) available to Stats(masks=(..., "couvreux")): s - mean - nstd_couvreux*std per level, its interpolation to the half
    levels, set_mask_thres(..., 0, Plus)."""

    def __init__(self, timescales, nstd_couvreux=1., names=None):
        self.names, self.nstd_couvreux = dict(names or {}), float(nstd_couvreux)
        self.timescales = {self.index(k): float(v) for k, v in dict(timescales).items()}
        self.params = capi.MhhDecayParams()
        for n, ts in self.timescales.items():
            if not 0 <= n < capi.MAX_SCALARS:
                raise ValueError("decay: scalar %r" % (n,))
            self.params.exponential[n], self.params.timescale[n] = 1, ts
        self.couvreux_index = self.names.get("couvreux")

    def index(self, key):
        if isinstance(key, str):
            if key in self.names:
                return int(self.names[key])
            if key == "th":
                return 0
            if key[:1] == "s" and key[1:].isdigit():
                return int(key[1:])
            raise ValueError("decay: no scalar called %r (names= maps a name to an index)" % key)
        return int(key)

    def bind(self, hp):
        self.hp = hp
        for n in list(self.timescales) + ([self.couvreux_index] if self.couvreux_index is not None else []):
            if int(n) >= len(hp.s):
                raise ValueError("decay: scalar %d of %d" % (int(n), len(hp.s)))
        self._cv = None
        return self

    def exec(self, dt_sub=None):
        """decay->exec(timeloop->get_sub_time_step()) (src/model.cxx:398): one launch."""
        hp = self.hp
        capi.check(hp.lib.mhh_decay_exec(hp.G, C.byref(hp.fields), C.byref(self.params), hp.dt if dt_sub is None else dt_sub, hp.stream), hp.lib)

    # -- Decay::get_mask("couvreux") ---------------------------------------------------------------------------------------------
    def has_mask(self, name):
        return name == "couvreux"

    def couvreux_sums(self):
        """[2][kcells] doubles on the device: the sums of s and s*s per level, over all slab ranks."""
        hp, torch = self.hp, self.hp.torch
        if self.couvreux_index is None:
            raise ValueError("Couvreux mask not available without couvreux scalar")
        if self._cv is None:
            n = int(hp.lib.mhh_decay_couvreux_scratch_elems(hp.G))
            self._cv = dict(scratch=torch.zeros(n, device=hp.device, dtype=torch.float64),
                            sums=torch.zeros((2, hp.grid.kcells), device=hp.device, dtype=torch.float64),
                            out=torch.zeros(hp.grid.shape3, device=hp.device, dtype=hp.td), outh=torch.zeros(hp.grid.shape3, device=hp.device, dtype=hp.td))
        cv = self._cv
        capi.check(hp.lib.mhh_decay_couvreux_sums(hp.G, hp.s[self.couvreux_index].data_ptr(), cv["scratch"].data_ptr(), cv["sums"].data_ptr(), hp.stream), hp.lib)
        if hp.npy > 1:
            cv["sums"].copy_(hp.master.sum_(cv["sums"].clone()))
        return cv["sums"]

    def couvreux(self):
        """The mask field s - mean - nstd*std (interior; zero elsewhere); couvreux_h() is its interpolation to the half levels."""
        hp = self.hp
        sums = self.couvreux_sums()
        cv = self._cv
        capi.check(hp.lib.mhh_decay_couvreux_field(hp.G, hp.s[self.couvreux_index].data_ptr(), sums.data_ptr(), self.nstd_couvreux,
                                                   cv["out"].data_ptr(), cv["outh"].data_ptr(), hp.stream), hp.lib)
        return cv["out"]

    def couvreux_h(self):
        """The half-level field of the last couvreux()."""
        if self._cv is None:
            self.couvreux()
        return self._cv["outh"]
