"""Budget_2 on the host side: the driver of csrc/budget_2.h, alone (Budget2Sampler) or behind
HotPath(..., stats=Stats(masks=(...)), budget=Budget2()).

Budget_2<TF>::exec_stats (src/budget_2.cxx) for second-order cases with the fields left on the device: the kinetic energies and the
shear, turbulent-transport, Coriolis, pressure-transport, redistribution and buoyancy terms of the u2, v2, w2, tke, uw, vw budgets and
the b2 and bw budgets, per mask, as fused evaluate-and-reduce passes. Every profile is averaged under the full-level flag over
kstart .. kend, the "zh" ones included, as the reference does; with diff_smag2 also the LES diffusion group (the *_diff profiles).
Not built: the DNS diffusion terms (*_visc, *_diss), Budget_4. On a slab (npy > 1) the double sums are added over the ranks (Master.sum_)
between every sums call and its finish call.
"""
import ctypes as C

from . import capi

KE, SHEAR, TURB, COR, PRES, RDSTR, DIFF, BUOY, BW_BUOY, ADV_S, PRES_S = (1 << n for n in range(11))
MOMENTUM = KE | SHEAR | TURB | PRES | RDSTR
THERMO = BUOY | BW_BUOY | ADV_S | PRES_S


class Budget2Sampler:
    """The budget passes over the masks of a stats.Sampler (its mask words, counts and stream)."""

    def __init__(self, sampler):
        s = self.s = sampler
        self.lib, self.grid, self.G, self.torch, self.device = s.lib, s.grid, s.G, s.torch, s.device
        nm = len(s.masks)
        z = lambda n: self.torch.zeros((n,), device=self.device, dtype=self.torch.float64)      # noqa: E731
        self.scratch = z(int(self.lib.mhh_budget_2_scratch_elems(self.G, nm)))
        self.mean_scratch = z(int(self.lib.mhh_field_mean_scratch_elems(self.G, 2)))

    def _ok(self, rc):
        capi.check(rc, self.lib)

    def names(self, groups):
        """[(name, "z" | "zh")] of a group set, in the order of the profiles."""
        n = int(self.lib.mhh_budget_2_nprofs(groups))
        if n < 0:
            raise ValueError("Budget2: unknown group bit in 0x%x" % groups)
        half, out = C.c_int(0), []
        for i in range(n):
            name = self.lib.mhh_budget_2_prof_name(groups, i, C.byref(half))
            out.append((name.decode(), "zh" if half.value else "z"))
        return out

    def model_profiles(self, u, v, w):
        """Stats::calc_mask_mean_profile of u, v, w: [3][nmasks][kcells] of the grid's dtype."""
        s, nm = self.s, len(self.s.masks)
        sums = self.torch.zeros((3, nm, self.grid.kcells), device=self.device, dtype=self.torch.float64)
        self._ok(self.lib.mhh_budget_2_model_sums(self.G, s.mfield.data_ptr(), nm, u.data_ptr(), v.data_ptr(), w.data_ptr(), sums.data_ptr(),
                                                  self.scratch.data_ptr(), s._stream()))
        s._all(sums)
        out = self.torch.zeros((3, nm, self.grid.kcells), device=self.device, dtype=s.td)
        self._ok(self.lib.mhh_budget_2_model_finish(self.G, nm, sums.data_ptr(), s.nmask.data_ptr(), out.data_ptr(), s._stream()))
        return out

    def mean_profiles(self, b, p):
        """field3d_operators.calc_mean_profile of b and p: [2][kcells]."""
        out = self.torch.zeros((2, self.grid.kcells), device=self.device, dtype=self.s.td)
        flds = (C.c_void_p*2)(b.data_ptr(), p.data_ptr())
        profs = (C.c_void_p*2)(out[0].data_ptr(), out[1].data_ptr())
        self._ok(self.lib.mhh_field_mean_profile(self.G, flds, 2, profs, self.mean_scratch.data_ptr(), self.s._stream()))
        if self.s._sum is not None:                  # a slab rank holds its share
            out.copy_(self.s._sum(out))
        return out

    def desc(self, groups, fields, model, means=None, utrans=0., vtrans=0., fc=0., diff_scheme=0, order=None):
        """mhh_budget_2_desc of device tensors: fields {u, v, w[, p, evisc, b, u_fluxbot, v_fluxbot]}, model [3][nmasks][kcells],
        means [2][kcells] = bmean, pmean. The tensors must outlive the calls."""
        d = capi.MhhBudget2Desc()
        for n in ("u", "v", "w", "p", "evisc", "b", "u_fluxbot", "v_fluxbot"):
            t = fields.get(n)
            setattr(d, n, None if t is None else t.data_ptr())
        d.umodel, d.vmodel, d.wmodel = model[0].data_ptr(), model[1].data_ptr(), model[2].data_ptr()
        if means is not None:
            d.bmean, d.pmean = means[0].data_ptr(), means[1].data_ptr()
        d.utrans, d.vtrans, d.fc = float(utrans), float(vtrans), float(fc)
        d.order = int(self.grid.order if order is None else order)
        d.diff_scheme, d.groups = int(diff_scheme), int(groups)
        return d

    def sums(self, d):
        s, nm = self.s, len(self.s.masks)
        n = max(int(self.lib.mhh_budget_2_nprofs(d.groups)), 1)
        sums = self.torch.zeros((n, nm, self.grid.kcells), device=self.device, dtype=self.torch.float64)
        self._ok(self.lib.mhh_budget_2_sums(self.G, s.mfield.data_ptr(), nm, C.byref(d), sums.data_ptr(), self.scratch.data_ptr(), s._stream()))
        s._all(sums)
        return sums

    def finish(self, d, sums):
        s, nm = self.s, len(self.s.masks)
        out = self.torch.zeros(tuple(sums.shape), device=self.device, dtype=s.td)
        self._ok(self.lib.mhh_budget_2_finish(self.G, nm, C.byref(d), sums.data_ptr(), s.nmask.data_ptr(), out.data_ptr(), s._stream()))
        return out

    def profiles(self, d):
        """out[prof][mask][kcells] of the grid's dtype, in the order of names(d.groups)."""
        return self.finish(d, self.sums(d))


class Budget2:
    """The budget group of a HotPath's statistics: HotPath(..., stats=Stats(...), budget=Budget2()); hp.stats.sample() then returns
    the budget profiles per mask under the reference's names.

    The groups follow Budget_2::create (src/budget_2.cxx:1315-1412): the Coriolis terms with a geostrophic Forcing only; the
    buoyancy, b2 and bw terms where the case has a thermo (dry: b from th and thref; thermo=Moist: its b; a buoy case: scalar 0).
    The diffusion group (*_diff) with diff_smag2 only, which needs two horizontal ghost cells (Budget_2's constructor asks the grid for
    them: HotPath(..., igc=2) where the case has fewer, and a case with jgc >= 2); with diff_2 it is absent (the DNS terms are not built)."""

    def bind(self, hp):
        if hp.stats is None:
            raise ValueError("Budget2: budget= needs stats=Stats(...)")
        if hp.grid.order != 2:
            raise ValueError("Budget2: second-order grids only (Budget_4 is not built)")
        self.hp = hp
        self.sampler = Budget2Sampler(hp.stats.sampler)
        fo, kind = hp.forcing, hp.cfg.get("thermo")
        self.geo = fo is not None and fo.swlspres == "geo"
        # what gives b: Thermo_moist's field, Thermo_buoy's scalar, else Thermo_dry's calc_buoyancy of scalar 0
        self.b_from = None
        if hp.thermo is not None and hasattr(hp.thermo, "field"):
            self.b_from = "moist"
        elif kind == "buoy" and hp.s:
            self.b_from = "buoy"
        elif kind is None and hp.s:
            self.b_from = "dry"
        from .grid import DIFF_SMAG2
        self.les = hp.cfg["diff"] == DIFF_SMAG2
        if self.les and (hp.grid.igc < 2 or hp.grid.jgc < 2):
            raise ValueError("Budget2: the LES diffusion terms need two horizontal ghost cells (Budget_2 calls set_minimum_ghost_cells(2, 2, 1)); "
                             "this grid has igc = %d, jgc = %d" % (hp.grid.igc, hp.grid.jgc))
        self.groups = MOMENTUM | (COR if self.geo else 0) | (DIFF if self.les else 0) | (THERMO if self.b_from else 0)
        self._b = None               # the dry case's b, made once and refilled at every sample
        self.names = self.sampler.names(self.groups)
        return self

    def buoyancy(self):
        """get_thermo_field(b, "b", cyclic = true) of the case's thermo, on hp.stream."""
        hp = self.hp
        if self.b_from == "moist":
            b = hp.thermo.field("b")
        elif self.b_from == "buoy":
            return hp.s[0]
        elif self.b_from == "dry":
            if self._b is None:
                self._b = hp.torch.zeros(hp.grid.shape3, device=hp.device, dtype=hp.td)
            b = self._b
            capi.check(hp.lib.mhh_thermo_dry_buoyancy(hp.G, b.data_ptr(), hp.s[0].data_ptr(), hp.thref.data_ptr(), float(hp.params.grav), hp.stream), hp.lib)
        else:
            raise ValueError("Budget2: this case has no thermo: no buoyancy")
        # get_thermo_field(b, "b", cyclic = true)
        hp.halo([b])
        return b

    def enqueue(self):
        """The device part, on hp.stream after Stats' own passes (the masks are final): returns the profiles [prof][mask][kcells]."""
        hp, sm, st = self.hp, self.sampler, self.hp.stats
        fields = dict(u=hp.u, v=hp.v, w=hp.w, p=hp.p, evisc=hp.evisc, u_fluxbot=hp.surf["u_fluxbot"], v_fluxbot=hp.surf["v_fluxbot"])
        means = None
        if self.groups & THERMO:
            fields["b"] = self.buoyancy()
            means = sm.mean_profiles(fields["b"], hp.p)
        model = sm.model_profiles(hp.u, hp.v, hp.w)
        d = sm.desc(self.groups, fields, model, means, utrans=st.utrans, vtrans=st.vtrans, fc=(hp.forcing.fc if self.geo else 0.),
                    diff_scheme=hp.cfg["diff"])
        self._keep = (fields, means, model)
        return sm.profiles(d)
