"""Stats on the host side: the driver of csrc/stats.h, alone (Sampler) or behind HotPath(..., stats=Stats(...)).

The sampling of Stats<TF> (src/stats.cxx) for second-order cases, with the fields left on the device: the mask words
(initialize_masks, set_mask_thres, finalize_masks), the masked profiles of calc_stats in two passes (means; then moments, frac and
the vertical gradient, which read the means of the first from device memory), calc_tend, calc_stats_2d, and the column pass of
cover and path, and the resolved, diffusive and total fluxes (_w, _diff, _flux) of advec_2 / advec_2i5 / the limited scalar flux and
diff_2 / diff_smag2. The parity target is the reference's CPU path. With HotPath(..., budget=Budget2()) a sample also holds the
profiles of Budget_2 (budget.py). Not built here: covariances and the qlcore / bplus /
bmin masks (they need b at the half level). On a slab (npy > 1) the double sums and the counts of a rank's rows are added over the ranks (Master.sum_) between every sums call and its finish call.
"""
import ctypes as C

import numpy as np

from . import capi

PLUS, MIN = 0, 1
MEAN, MOMENT2, MOMENT3, MOMENT4, FRAC, GRAD, COUNT, MEAN2D, FLUX_W, FLUX_DIFF, FLUX_SUM = 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
MAX_MASKS, MAX_JOBS = 8, 16
# the operation names of Stats::add_profs that are built, and what each becomes
PASS_A = {"mean": MEAN}
PASS_B = {"2": MOMENT2, "3": MOMENT3, "4": MOMENT4, "frac": FRAC, "grad": GRAD}
COLUMN = ("path", "cover")
FLUXES = {"w": FLUX_W, "diff": FLUX_DIFF, "flux": FLUX_SUM}      # in this order in a call: _flux adds the two before it


def fill_value(dtype):
    """netcdf_fp_fillvalue (src/stats.cxx:51-53)."""
    return np.dtype(dtype).type(9.9692099683868690e+36)


def prof_name(var, op):
    return var if op == "mean" else "%s_%s" % (var, op)


class Sampler:
    """The masks and profiles of one grid on one device, on torch tensors (CPU tensors with the emulation build of the tests).

    masks: the names in the order of add_mask; mask n has flag 1 << 2n and flagh 1 << (2n+1). The call sequence is the
    reference's: initialize_masks(); set_mask_thres(...) per mask that is not "default"; finalize_masks(); then profiles(),
    columns(). Nothing here synchronises; host() does, once."""

    def __init__(self, lib, grid, G, torch, device, masks=("default",), stream=None, sum_=None):
        if not 1 <= len(masks) <= MAX_MASKS:
            raise ValueError("1 .. %d masks" % MAX_MASKS)
        if len(set(masks)) != len(masks):
            raise ValueError("mask names must differ")
        if grid.order != 2:
            raise ValueError("Stats: second-order grids only (calc_grad_4th and the fourth-order fluxes are not built)")
        if grid.npy != 1 and sum_ is None:
            raise ValueError("Stats: a slab rank needs sum_, the sum over the ranks (Master.sum_)")
        # a slab rank: the double sums and counts of its rows are added over the ranks between a sums call and its finish call
        self._sum = sum_ if grid.npy != 1 else None
        self.lib, self.grid, self.G, self.torch, self.device = lib, grid, G, torch, device
        self.masks = tuple(masks)
        self._stream = stream or (lambda: C.c_void_p(0))
        g, nm = grid, len(masks)
        self.td = torch.float64 if g.np_dtype == np.float64 else torch.float32
        z = lambda shape, dt: torch.zeros(shape, device=device, dtype=dt)      # noqa: E731
        self.mfield = z(g.shape3, torch.int32)             # the words are unsigned: read them through host_words()
        self.mfield_bot = z(g.shape2, torch.int32)
        self.csums = z((2, nm, g.kcells), torch.float64)
        self.nmask = z((nm, 2, g.kcells), torch.int32)
        self.nmask_bot = z((nm,), torch.int32)
        self.area, self.areah = z((nm, g.kcells), self.td), z((nm, g.kcells), self.td)
        self.scratch = z((int(lib.mhh_stats_scratch_elems(G, nm, MAX_JOBS)),), torch.float64)
        self.zero2d = z(g.shape2, self.td)

    def _ok(self, rc):
        capi.check(rc, self.lib)

    # -- masks ---------------------------------------------------------------------------------------------------
    def initialize_masks(self):
        self._ok(self.lib.mhh_stats_mask_init(self.G, self.mfield.data_ptr(), self.mfield_bot.data_ptr(), len(self.masks), self._stream()))

    def set_mask_thres(self, name, fld, fldh, fld_bot=None, threshold=0., mode=PLUS):
        """Stats::set_mask_thres(name, fld, fldh, threshold, mode); fld_bot is fldh's fld_bot (None: zeros)."""
        if name not in self.masks:
            raise ValueError("Invalid mask name in set_mask_thres()")
        bot = self.zero2d if fld_bot is None else fld_bot
        self._ok(self.lib.mhh_stats_mask_thres(self.G, self.mfield.data_ptr(), self.mfield_bot.data_ptr(), self.masks.index(name), fld.data_ptr(),
                                               fldh.data_ptr(), bot.data_ptr(), float(threshold), int(mode), self._stream()))

    def finalize_masks(self):
        nm = len(self.masks)
        self._ok(self.lib.mhh_stats_mask_count(self.G, self.mfield.data_ptr(), self.mfield_bot.data_ptr(), nm, self.csums.data_ptr(),
                                               self.scratch.data_ptr(), self._stream()))
        self._all(self.csums)
        self._ok(self.lib.mhh_stats_mask_finish(self.G, nm, self.csums.data_ptr(), self.nmask.data_ptr(), self.nmask_bot.data_ptr(),
                                                self.area.data_ptr(), self.areah.data_ptr(), self._stream()))

    def _all(self, t):
        """The sum over the ranks, in place (master.sum of the reference; one rank: nothing)."""
        if self._sum is not None:
            t.copy_(self._sum(t))

    # -- profiles ------------------------------------------------------------------------------------------------
    def sums(self, jobs):
        """The double sums [job][mask][kcells] of up to MAX_JOBS jobs (fld, loc, op, offset, threshold, mean[, flux]); flux is a
        dict of what a flux job takes beyond that (the members of mhh_stats_job: tensors for w, wmean, evisc, flux_bot, flux_top)."""
        nm, nj = len(self.masks), len(jobs)
        arr = (capi.MhhStatsJob*nj)()
        for n, job in enumerate(jobs):
            fld, loc, op, offset, threshold, mean = job[:6]
            arr[n] = capi.MhhStatsJob(fld.data_ptr(), None if mean is None else mean.data_ptr(), int(loc), int(op), float(offset), float(threshold))
            for k, v in (job[6] if len(job) > 6 else {}).items():
                setattr(arr[n], k, v.data_ptr() if hasattr(v, "data_ptr") else v)
        s = self.torch.zeros((nj, nm, self.grid.kcells), device=self.device, dtype=self.torch.float64)
        self._ok(self.lib.mhh_stats_sums(self.G, self.mfield.data_ptr(), nm, arr, nj, s.data_ptr(), self.scratch.data_ptr(), self._stream()))
        self._all(s)
        return arr, s

    def finish(self, arr, sums):
        nm, nj = len(self.masks), len(arr)
        out = self.torch.zeros((nj, nm, self.grid.kcells), device=self.device, dtype=self.td)
        self._ok(self.lib.mhh_stats_finish(self.G, nm, arr, nj, sums.data_ptr(), self.nmask.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def profiles(self, jobs):
        """out[job][mask][kcells] of the grid's dtype, in batches of MAX_JOBS."""
        outs = []
        for b in range(0, len(jobs), MAX_JOBS):
            arr, s = self.sums(jobs[b:b+MAX_JOBS])
            outs.append(self.finish(arr, s))
        return self.torch.cat(outs) if len(outs) > 1 else outs[0]

    def column_sums(self, fld, loc, offset, threshold, rhoref):
        nm = len(self.masks)
        s = self.torch.zeros((nm, 3), device=self.device, dtype=self.torch.float64)
        self._ok(self.lib.mhh_stats_columns(self.G, self.mfield.data_ptr(), nm, fld.data_ptr(), int(loc), float(offset), float(threshold),
                                            rhoref.data_ptr(), s.data_ptr(), self.scratch.data_ptr(), self._stream()))
        self._all(s)
        return s

    def columns(self, fld, loc, offset, threshold, rhoref):
        """out[mask][2] = cover, path of one variable."""
        nm = len(self.masks)
        s = self.column_sums(fld, loc, offset, threshold, rhoref)
        out = self.torch.zeros((nm, 2), device=self.device, dtype=self.td)
        self._ok(self.lib.mhh_stats_columns_finish(self.G, nm, s.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def host_words(self):
        """mfield and mfield_bot as unsigned words on the host."""
        return self.mfield.cpu().numpy().view(np.uint32).copy(), self.mfield_bot.cpu().numpy().view(np.uint32).copy()


class Stats:
    """The statistics of a HotPath: HotPath(..., stats=Stats(masks=("default",))), then hp.stats.sample().

    bind() registers what Fields::exec_stats (src/fields.cxx:647-665) and Diff_smag2::exec_stats register, as far as their
    operations are built: w; u and v with utrans / vtrans as offsets; every scalar and its _bot; p; evisc. add() registers more, e.g.
    a ql field with ("mean", "frac", "path", "cover") at its threshold. Built-in masks: "default"; "wplus" and "wmin" as
    Fields::get_mask builds them; "ql" as Thermo_moist::get_mask does (needs thermo=Moist); "couvreux" as Decay::get_mask does (needs
    decay=Decay(..., names={"couvreux": n})). Any other name is a mask whose thresholds
    the caller registers with mask_thres(); all are applied, in the order given, at every sample()."""

    def __init__(self, masks=("default",), utrans=None, vtrans=None):
        self.masks = tuple(masks)
        for m in self.masks:
            if m in ("qlcore", "bplus", "bmin"):
                raise ValueError("Stats: the built-in mask %r is not built (it needs b at the half level); "
                                 "register a threshold of your own with mask_thres()" % m)
        self.utrans, self.vtrans = utrans, vtrans                  # gd.utrans, gd.vtrans; None: the Forcing's, else 0
        self.vars, self.vars2d, self.thresholds, self.flux = [], [], [], {}

    def bind(self, hp):
        self.hp = hp
        self.sampler = Sampler(hp.lib, hp.grid, hp.G, hp.torch, hp.device, self.masks, stream=lambda: hp.stream, sum_=hp.master.sum_)
        # ql and ql_h as callables for mask_thres() and add(): one object each, so that a sample evaluates each once
        self.ql = lambda: hp.thermo.field("ql")      # noqa: E731
        self.ql_h = lambda: hp.thermo.field("ql_h")      # noqa: E731
        for m in self.masks:
            if m in ("wplus", "wmin"):
                # Fields::get_mask (src/fields.cxx:631-643): w interpolated to the full level, and the arguments in the order the
                # reference passes them -- w itself as `fld`, the interpolated field as `fldh`, whose fld_bot is a tmp field's
                self.mask_thres(m, hp.w, self.w_full, None, 0., PLUS if m == "wplus" else MIN)
            elif m == "ql":
                # Thermo_moist::get_mask (src/thermo_moist.cxx:1314-1329). The reference passes the stale fld_bot of the tmp field
                # that holds ql_h; a zero 2-D array here. nmask_bot is overwritten by finalize_masks in any case.
                if hp.thermo is None or not hasattr(hp.thermo, "field"):
                    raise ValueError("Stats: the ql mask needs thermo=Moist(pbot)")
                self.mask_thres(m, self.ql, self.ql_h, None, 0., PLUS)
            elif m == "couvreux":
                # Decay::get_mask (src/decay.cxx:123-187): the decaying tracer less its level mean and nstd_couvreux standard
                # deviations, and its interpolation to the half levels, at threshold 0; the reference throws without the scalar
                dec = getattr(hp, "decay", None)
                if dec is None or dec.couvreux_index is None:
                    raise ValueError("Couvreux mask not available without couvreux scalar")
                self.mask_thres(m, dec.couvreux, dec.couvreux_h, None, 0., PLUS)
            elif m == "ib" and getattr(hp, "ib", None) is not None:
                # Immersed_boundary::get_mask (src/immersed_boundary.cxx:930-946): calc_mask's two fields at threshold 0.5; without
                # ib= the name stays a mask of the caller's
                self.mask_thres(m, hp.ib.mask, hp.ib.maskh, None, 0.5, PLUS)
        std = ("mean", "2", "3", "4", "grad")
        fo = hp.forcing
        self.utrans = float(self.utrans if self.utrans is not None else (fo.utrans if fo is not None else 0.))
        self.vtrans = float(self.vtrans if self.vtrans is not None else (fo.vtrans if fo is not None else 0.))
        # the fluxes where the case's schemes are ones whose flux is built (advec 2 / 2i5, diff 2 / smag2)
        from .grid import ADVEC_2, ADVEC_2I5, DIFF_2, DIFF_SMAG2
        cfg = hp.cfg
        fl = ("w", "diff", "flux") if cfg["advec"] in (ADVEC_2, ADVEC_2I5) and cfg["diff"] in (DIFF_2, DIFF_SMAG2) else ()
        self.add("w", hp.w, 1, std)
        self.add("u", hp.u, 0, std + fl, offset=self.utrans, flux=dict(kind=1, visc=cfg["visc"], flux_bot=hp.surf["u_fluxbot"], flux_top=hp.surf["u_fluxtop"]))
        self.add("v", hp.v, 0, std + fl, offset=self.vtrans, flux=dict(kind=2, visc=cfg["visc"], flux_bot=hp.surf["v_fluxbot"], flux_top=hp.surf["v_fluxtop"]))
        for n, s in enumerate(hp.s):
            # flux_bot / flux_top are read from hp.fields at every sample: a surface layer binds its own per scalar
            self.add("s%d" % n, s, 0, std + fl, flux=dict(kind=0, visc=cfg["visc"], scalar=n, limit=int(hp.fields.s_fluxlimit[n])))
        sbot = getattr(hp.surface, "sbot", None) if hp.surface is not None else None
        if sbot is not None:
            for n, b in enumerate(sbot):
                self.add_2d("s%d_bot" % n, b)
        self.add("p", hp.p, 0, ("mean", "2"))
        self.add("evisc", hp.evisc, 0, ("mean", "2"))
        return self

    def w_full(self):
        """grid.interpolate_2nd(wf, w, wloc, sloc): w at the full level, a new device tensor."""
        hp = self.hp
        wf = hp.torch.empty(hp.grid.shape3, device=hp.device, dtype=hp.td)
        capi.check(hp.lib.mhh_stats_interpolate_w(hp.G, hp.w.data_ptr(), wf.data_ptr(), hp.stream), hp.lib)
        return wf

    def add(self, name, tensor, loc, ops, offset=0., threshold=0., flux=None):
        """Stats::add_profs + calc_stats of one variable: loc 0 full level, 1 half level; ops of "mean", "2", "3", "4", "frac",
        "grad", "path", "cover". tensor: a device tensor of the grid's shape, or a callable that returns one at every sample()
        (a diagnostic field such as hp.thermo.field("ql"))."""
        for op in ops:
            if op not in PASS_A and op not in PASS_B and op not in COLUMN and op not in FLUXES:
                raise ValueError("Stats: unknown operation %r" % op)
        if any(op in FLUXES for op in ops):
            if loc == 1:
                raise ValueError("Stats: the flux of a half-level variable (w itself) cannot be delivered at that location")
            if "mean" not in ops:
                raise ValueError("Stats: a flux needs the mean of its variable")
            if "flux" in ops and not ("w" in ops and "diff" in ops):
                raise ValueError("Stats: _flux = _w + _diff needs both")
            if flux is None:
                raise ValueError("Stats: a flux needs flux=dict(kind=, visc=, flux_bot=, flux_top=, limit=): where the variable lives and its diffusion")
        if any(op in ("2", "3", "4") for op in ops) and "mean" not in ops:
            raise ValueError("Stats: a moment needs the mean of its variable")
        if loc == 1 and any(op in COLUMN for op in ops):
            raise ValueError("Stats: path and cover are taken of full-level variables")
        self.flux[name] = flux
        self.vars.append((name, tensor, int(loc), tuple(ops), float(offset), float(threshold)))

    def add_2d(self, name, tensor, offset=0.):
        """calc_stats_2d: a time series, the horizontal mean of a 2-D field."""
        self.vars2d.append((name, tensor, float(offset)))

    def mask_thres(self, name, fld, fldh, fld_bot=None, threshold=0., mode=PLUS):
        """Register set_mask_thres(name, fld, fldh, fld_bot, threshold, mode) for every sample()."""
        if name not in self.masks or name == "default":
            raise ValueError("Invalid mask name in set_mask_thres()")
        self.thresholds.append((name, fld, fldh, fld_bot, float(threshold), int(mode)))

    def enqueue(self):
        """The device part of a sample, on hp.stream, without a synchronisation: the masks, pass A, pass B, the column pass. Returns
        (names of pass A, its profiles, names of pass B, its profiles, {variable: cover and path}) as device tensors."""
        sm, hp = self.sampler, self.hp
        sm.initialize_masks()
        made = {}

        def now(x):                  # a callable is evaluated once per sample, however often it is registered
            if not callable(x):
                return x
            if id(x) not in made:
                made[id(x)] = x()
            return made[id(x)]
        for name, fld, fldh, bot, thr, mode in self.thresholds:
            sm.set_mask_thres(name, now(fld), now(fldh), now(bot), thr, mode)
        sm.finalize_masks()
        live = [(name, now(t), loc, ops, off, thr) for name, t, loc, ops, off, thr in self.vars]
        # pass A: the means
        ja, na = [], []
        for name, t, loc, ops, off, thr in live:
            if "mean" in ops:
                ja.append((t, loc, MEAN, off, thr, None)); na.append(name)
        for name, t, off in self.vars2d:
            ja.append((t, 0, MEAN2D, off, 0., None)); na.append(name)
        outa = sm.profiles(ja) if ja else None
        # pass B: what reads the means
        jb, nb = [], []
        for name, t, loc, ops, off, thr in live:
            for op in ops:
                if op in PASS_B:
                    jb.append((t, loc, PASS_B[op], off, thr, outa[na.index(name)] if op in ("2", "3", "4") else None)); nb.append(prof_name(name, op))
        outb = sm.profiles(jb) if jb else None
        # the fluxes: _w, _diff and their sum per variable, in one call each (the sum names the two jobs before it)
        outc, nc = [], []
        for name, t, loc, ops, off, thr in live:
            fo = [op for op in ("w", "diff", "flux") if op in ops]
            if not fo:
                continue
            f, cfg = self.flux[name], hp.cfg
            if "w" not in na:
                raise ValueError("Stats: the resolved flux needs the variable w registered with its mean")
            bot, top = f.get("flux_bot"), f.get("flux_top")
            if "scalar" in f:
                bot, top = int(hp.fields.s_fluxbot[f["scalar"]]), int(hp.fields.s_fluxtop[f["scalar"]])
            extra = {"w": dict(kind=f["kind"], scheme=cfg["advec"], limit=int(f.get("limit", 0)), w=hp.w, wmean=outa[na.index("w")]),
                     "diff": dict(kind=f["kind"], scheme=cfg["diff"], surface_model=int(cfg["sm"]), w=hp.w, evisc=hp.evisc, flux_bot=bot, flux_top=top,
                                  visc=float(f["visc"]), tPr=float(hp.params.tPr)),
                     "flux": dict(a=0, b=1)}
            outc.append(sm.profiles([(t, loc, FLUXES[op], off, thr, outa[na.index(name)], extra[op]) for op in fo]))
            nc += [prof_name(name, op) for op in fo]
        if outc:
            outb = hp.torch.cat(([outb] if outb is not None else []) + outc)
            nb = nb + nc
        cols = {name: sm.columns(t, loc, off, thr, hp.rhoref) for name, t, loc, ops, off, thr in live if any(op in COLUMN for op in ops)}
        return na, outa, nb, outb, cols

    def sample(self):
        """One sample on hp.stream, outside the captured step: {mask: {name: numpy profile of kcells | float}} with the fill value
        where the reference has it, and nmask, nmaskh, area, areah per mask."""
        sm, hp = self.sampler, self.hp
        na, outa, nb, outb, cols = self.enqueue()
        # Budget_2::exec_stats (src/budget_2.cxx:1414-1818) after Stats' own passes, under the masks they left
        bud = getattr(hp, "budget", None)
        outd = bud.enqueue() if bud is not None else None
        hp.sync()
        hd = outd.cpu().numpy() if outd is not None else None
        ha = outa.cpu().numpy() if outa is not None else None
        hb = outb.cpu().numpy() if outb is not None else None
        nmask, area, areah = sm.nmask.cpu().numpy(), sm.area.cpu().numpy(), sm.areah.cpu().numpy()
        res = {}
        n2d = {v[0] for v in self.vars2d}
        hc = {name: c.cpu().numpy() for name, c in cols.items()}
        for m, mask in enumerate(self.masks):
            r = res[mask] = {"nmask": nmask[m, 0].copy(), "nmaskh": nmask[m, 1].copy(), "area": area[m].copy(), "areah": areah[m].copy()}
            for n, name in enumerate(na):
                r[name] = float(ha[n, m, 0]) if name in n2d else ha[n, m].copy()
            for n, name in enumerate(nb):
                r[name] = hb[n, m].copy()
            if hd is not None:
                for n, (name, _) in enumerate(bud.names):
                    r[name] = hd[n, m].copy()
            for name, t, loc, ops, off, thr in self.vars:
                if name in hc:
                    c = hc[name]
                    if "cover" in ops:
                        r[name + "_cover"] = float(c[m, 0])
                    if "path" in ops:
                        r[name + "_path"] = float(c[m, 1])
        return res
