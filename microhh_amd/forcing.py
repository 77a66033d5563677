"""Buffer and Force of a sub-step (src/buffer.cxx, src/force.cxx; src/model.cxx:395,404) and the horizontal means they read
(Field3d_operators, src/model.cxx:351): the parameter structs of the C ABI, the host tables, and the per-step calls HotPath makes
with ``HotPath(..., forcing=Forcing(...))``.

Profiles are numpy arrays of kcells elements (ghost levels included), keyed by field name: "u", "v", "w", "s0", "s1", ...
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import MhhBufferParams, MhhForceParams  # noqa: F401

LSPRES = {None: 0, "0": 0, "dpdx": 1, "uflux": 2, "geo": 3}
WLS = {None: 0, "0": 0, "mean": 1, "local": 2}


def buffer_kstart(g, zstart):
    """Buffer::create (src/buffer.cxx:107-126): (bufferkstart, bufferkstarth), the first full and half level inside the sponge."""
    ks = g.kstart + int(np.count_nonzero(g.z[g.kstart:g.kend] < g.np_dtype.type(zstart)))
    ksh = g.kstart + int(np.count_nonzero(g.zh[g.kstart:g.kend] < g.np_dtype.type(zstart)))
    if ksh == g.kend:
        raise RuntimeError("Buffer is too close to the model top")
    return ks, ksh


def sigma_tables(lib, g, zstart, sigma=2., beta=2.):
    """(sigmaz at full levels, at half levels): sigma*pow((z-zstart)/(zsize-zstart), beta) with the host C library's pow of the
    grid's dtype (src/buffer.cxx:44,48)."""
    out = []
    for half in (0, 1):
        t = np.zeros(g.kcells, dtype=g.np_dtype)
        capi.check(lib.mhh_buffer_sigma_host(g.host_struct(), zstart, sigma, beta, half, t.ctypes.data), lib)
        out.append(t)
    return out


def field_names(nscalars):
    return ["u", "v", "w"] + ["s%d" % n for n in range(nscalars)]


class Forcing:
    """The switches of [buffer] and [force] (src/buffer.cxx:62-77, src/force.cxx:315-420) that the library covers.

    swbuffer with zstart, sigma, beta; swupdate (the mean profiles as the sponge's target) or bufferprofs {name: profile}.
    swlspres "dpdx" (dpdx), "uflux" (uflux; the sub-step's dt is HotPath.dt) or "geo" (fc, ug, vg, order from the case).
    lsprofs {name: profile} (swls), swwls "mean" | "local" with wls and swwls_mom, nudgeprofs {name: profile} with nudge_factor.

    The sponge acts on u, v, w and every scalar, as the reference's does: without swupdate, bufferprofs must hold a profile for
    each of them (bind() raises otherwise). lsprofs and nudgeprofs take u, v and the scalars; w has no slot.

    swlspres "uflux" together with swbuffer: HotPath.step() takes the volume sum of ut BEFORE the fused pass, so the sum does
    not hold the sponge's term on ut, while the reference, running buffer->exec and then force->exec, includes it. For the
    reference's order call mhh_buffer_exec, mhh_field_mean_sum, mhh_force_exec in turn.
    """

    def __init__(self, swbuffer=False, zstart=None, sigma=2., beta=2., swupdate=False, bufferprofs=None,
                 swlspres=None, dpdx=0., uflux=0., fc=0., ug=None, vg=None, utrans=0., vtrans=0.,
                 lsprofs=None, swwls=None, swwls_mom=False, wls=None, nudgeprofs=None, nudge_factor=None):
        if swlspres not in LSPRES or swwls not in WLS:
            raise ValueError("swlspres: dpdx | uflux | geo; swwls: mean | local")
        self.swbuffer, self.zstart, self.sigma, self.beta, self.swupdate = swbuffer, zstart, sigma, beta, swupdate
        self.swlspres, self.dpdx, self.uflux, self.fc, self.ug, self.vg = swlspres, dpdx, uflux, fc, ug, vg
        self.utrans, self.vtrans = utrans, vtrans
        self.swwls, self.swwls_mom, self.wls, self.nudge_factor = swwls, swwls_mom, wls, nudge_factor
        self.lsprofs, self.nudgeprofs, self.bufferprofs = dict(lsprofs or {}), dict(nudgeprofs or {}), dict(bufferprofs or {})

    # -- made once per HotPath -------------------------------------------------------------------------------------
    def bind(self, hp):
        torch, g = hp.torch, hp.grid
        self.hp = hp
        names = self.names = field_names(len(hp.s))
        self._keep = []
        for what, d in (("lsprofs", self.lsprofs), ("nudgeprofs", self.nudgeprofs)):
            bad = [n for n in d if n == "w" or n not in names]
            if bad:
                raise ValueError("%s: %s: not u, v or one of this case's scalars" % (what, ", ".join(bad)))
        if self.swbuffer and not self.swupdate:
            missing = [n for n in names if n not in self.bufferprofs]
            if missing:
                raise ValueError("swbuffer without swupdate: bufferprofs holds no profile for " + ", ".join(missing))

        def up(a):
            a = np.ascontiguousarray(np.asarray(a, dtype=g.np_dtype))
            if a.shape != (g.kcells,):
                raise ValueError("a profile holds kcells = %d elements" % g.kcells)
            t = torch.from_numpy(a.copy()).to(hp.device)
            self._keep.append(t)
            return t

        def put(struct, stem, name, t):
            if name in ("u", "v", "w"):
                setattr(struct, "%s_%s" % (stem, name), t.data_ptr())
            else:
                getattr(struct, stem + "_s")[int(name[1:])] = t.data_ptr()
        # which mean profiles the switches read
        need = set()
        if self.swbuffer and self.swupdate:
            need |= set(names)
        if WLS[self.swwls] == 1:
            need |= set(n for n in names if n[0] == "s") | ({"u", "v"} if self.swwls_mom else set())
        need |= set(self.nudgeprofs)
        self.mean_names = [n for n in names if n in need]
        self.mean_prof = {n: torch.zeros(g.kcells, device=hp.device, dtype=hp.td) for n in self.mean_names}
        nred = max(len(self.mean_names), 2)
        self.scratch = torch.zeros(int(hp.lib.mhh_field_mean_scratch_elems(hp.G, nred)), device=hp.device, dtype=torch.float64)
        self.sums = torch.zeros(2, device=hp.device, dtype=torch.float64)

        self.bparams = b = MhhBufferParams()
        if self.swbuffer:
            b.swbuffer = 1
            b.bufferkstart, b.bufferkstarth = buffer_kstart(g, self.zstart)
            sg, sgh = (up(t) for t in sigma_tables(hp.lib, g, self.zstart, self.sigma, self.beta))
            b.sigma, b.sigmah = sg.data_ptr(), sgh.data_ptr()
            for n in names:
                put(b, "abuf", n, self.mean_prof[n] if self.swupdate else up(self.bufferprofs[n]))
        self.fparams = p = MhhForceParams()
        p.swlspres, p.order = LSPRES[self.swlspres], hp.cfg["order"]
        p.dpdx, p.uflux, p.dt, p.fc, p.utrans, p.vtrans = self.dpdx, self.uflux, hp.dt, self.fc, self.utrans, self.vtrans
        p.uflux_sums = self.sums.data_ptr()
        if p.swlspres == 3:
            p.ug, p.vg = up(self.ug).data_ptr(), up(self.vg).data_ptr()
        if self.lsprofs:
            p.swls = 1
            for n, a in self.lsprofs.items():
                put(p, "ls", n, up(a))
        p.swwls, p.swwls_mom = WLS[self.swwls], int(bool(self.swwls_mom))
        if p.swwls:
            p.wls = up(self.wls).data_ptr()
        for n in self.mean_names:
            if n != "w":
                put(p, "mean", n, self.mean_prof[n])
        if self.nudgeprofs:
            p.swnudge = 1
            p.nudge_factor = up(self.nudge_factor).data_ptr()
            for n, a in self.nudgeprofs.items():
                put(p, "nudge", n, up(a))
        return self

    # -- per sub-step ---------------------------------------------------------------------------------------------
    def _field(self, name, tend=False):
        hp = self.hp
        if name in ("u", "v", "w"):
            return getattr(hp, name + "t" if tend else name)
        return (hp.st if tend else hp.s)[int(name[1:])]

    def means(self):
        """fields->exec() (src/model.cxx:351) for what the switches need: the mean profiles, and for uflux the two volume sums. A
        slab rank computes its share; the shares are summed over the ranks before they are consumed."""
        hp, lib = self.hp, self.hp.lib
        if self.mean_names:
            flds = [self._field(n) for n in self.mean_names]
            profs = [self.mean_prof[n] for n in self.mean_names]
            capi.check(lib.mhh_field_mean_profile(hp.G, hp._ptrs(flds), len(flds), hp._ptrs(profs), self.scratch.data_ptr(), hp.stream), lib)
            if hp.npy > 1:
                both = hp.master.sum_(hp.torch.stack(profs))
                for t, s in zip(profs, both):
                    t.copy_(s)
        if self.fparams.swlspres == 2:
            flds = [hp.u, hp.ut]
            capi.check(lib.mhh_field_mean_sum(hp.G, hp._ptrs(flds), 2, self.sums.data_ptr(), self.scratch.data_ptr(), hp.stream), lib)
            if hp.npy > 1:
                self.sums.copy_(hp.master.sum_(self.sums.clone()))

    def exec(self):
        """buffer->exec and force->exec (src/model.cxx:395,404) as one pass over the tendencies."""
        hp = self.hp
        capi.check(hp.lib.mhh_buffer_force_exec(hp.G, C.byref(hp.fields), C.byref(self.bparams), C.byref(self.fparams), hp.stream), hp.lib)

    def exec_buffer(self):
        """buffer->exec (src/model.cxx:395) on its own: a stage sits between it and force->exec."""
        hp = self.hp
        capi.check(hp.lib.mhh_buffer_exec(hp.G, C.byref(hp.fields), C.byref(self.bparams), hp.stream), hp.lib)

    def exec_force(self):
        """force->exec (src/model.cxx:404) on its own."""
        hp = self.hp
        capi.check(hp.lib.mhh_force_exec(hp.G, C.byref(hp.fields), C.byref(self.fparams), hp.stream), hp.lib)
