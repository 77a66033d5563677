"""Host-side driver of one RK sub-step's hot path: the slice of ``Model<TF>::exec`` (src/model.cxx:346-411)
that this package accelerates, expressed as calls into the C ABI.

    boundary->set_prognostic_cyclic_bcs   -> mhh_boundary_cyclic_n (+ N-S neighbour exchange)   (src/model.cxx:346)
    diff->exec_viscosity(thermo)          -> mhh_diff_exec_viscosity (+ N-S exchange of evisc)   (:354)
    thermo->exec (Thermo_moist)           -> mhh_thermo_moist_base_state, mhh_thermo_moist_buoyancy_tend (thermo=..., opt-in) (:366)
    microphys->exec ; limiter->exec       -> mhh_micro_2mom_warm_exec or mhh_micro_nsw6_exec, mhh_limiter_exec (micro=..., opt-in) (:369, :415)
    radiation->exec (Radiation_gcss)      -> mhh_radiation_gcss_exec (radiation=..., opt-in)      (:372)
    boundary->exec ; set_ghost_cells      -> mhh_boundary_surface_exec, mhh_boundary_ghost_cells (surface=..., opt-in) (:374-375)
    ib->exec_scalars ; ib->exec_momentum  -> mhh_ib_set_ghost_cells + the cyclic fills (ib=..., opt-in)  (:380, :407)
    advec->exec ; diff->exec              -> mhh_rhs_exec (fused, same bits)                     (:388, :392)
    fields->exec ; buffer->exec ; force->exec -> mhh_field_mean_*, mhh_buffer_force_exec (forcing=..., opt-in) (:351, :395, :404)
    pres->exec(dt)                        -> mhh_pres_exec, or its slab form around 2 all-to-alls (:411)

One process per GPU. With ``npy`` > 1 the grid is slab-decomposed in y (npx = 1): halos travel as ring
send/recv and the pressure solver's x<->y transposes as all_to_all (backend "nccl" = RCCL over xGMI).
The exchanges live in master.py: its ``Master`` decides once how messages travel (local copy, direct,
host-staged), HotPath packs, calls it and unpacks. PyTorch provides device memory, streams and the process
group only; every kernel is the hand-written HIP behind the C ABI. Case recipes follow SURVEY.md §8(d).
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

from . import capi
from .master import Master
from .grid import Grid, ADVEC_2, ADVEC_2I5, ADVEC_4, DIFF_2, DIFF_4, DIFF_SMAG2, EDGE_BOTH, EDGE_EW, moser_z

CASES = {
    # name: advec, diff, pres order, spatial order, ghost cells, domain, scalars, surface model
    "taylorgreen": dict(advec=ADVEC_2, diff=DIFF_2, pres=2, order=2, gc=(1, 1, 1), size=(1., 1., 0.5), nscalars=0, sm=0, visc=(8.*math.pi**2*1000.)**-1),
    "drycblles": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(3200., 3200., 1200.), nscalars=1, sm=1, visc=1e-5),
    # gabls1 (cases/gabls1/gabls1.ini: cs = 0.1, 400 m domain at 32^2 columns, scaled with the column count)
    "gabls1": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(12800., 12800., 400.), nscalars=1, sm=1, visc=1e-5, cs=0.1),
    "moser600": dict(advec=ADVEC_4, diff=DIFF_4, pres=4, order=4, gc=(3, 3, 3), size=(2*math.pi, math.pi, 2.), nscalars=0, sm=0, visc=1e-5),
    # Thermo_buoy cases (swthermo=buoy, src/thermo_buoy.cxx): scalar 0 is the buoyancy b, whose flat-form tendency of w is folded
    # into the RHS pass and whose N2 feeds exec_viscosity inline. drycbl: cases/drycbl/drycbl.ini (its jtot = 1 is the usual shape
    # of the family; 512^3 and 1024 x 1 x 384 = vanheerwaarden2016 are the sizes the tests run). sbl: cases/SBL_Smag/SBL1800.ini
    # (tPr = 10, surface model) with the 2i5 advection of the second-order LES cases.
    "drycbl": dict(advec=ADVEC_4, diff=DIFF_4, pres=4, order=4, gc=(3, 3, 3), size=(1., 1., 1.2908699973147109), nscalars=1, sm=0, visc=8e-5,
                   thermo="buoy"),
    "sbl": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(27.386127875258303, 27.386127875258303, 18.074844397670482),
                nscalars=1, sm=1, visc=1.5e-5, tPr=10., thermo="buoy"),
    # bomex (cases/bomex): Thermo_moist with scalar 0 = thl, 1 = qt, pbot = 101500 Pa; HotPath(..., thermo=thermo.Moist(pbot)) switches
    # the thermodynamics on. The schemes are upstream's choice for the case; this fork's cases/bomex/bomex.ini says swadvec=2.
    "bomex": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(6400., 6400., 3000.), nscalars=2, sm=1, visc=1e-5,
                  thermo="moist", pbot=101500.),
    # rico (cases/rico/rico.ini): Thermo_moist with Microphys_2mom_warm, scalars 0 = thl, 1 = qt, 2 = qr, 3 = nr, pbot = 101540 Pa, the
    # schemes of bomex; HotPath(..., thermo=thermo.Moist(pbot), micro=microphys.Warm2mom(Nc0)) switches the physics on.
    "rico": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(12800., 12800., 4000.), nscalars=4, sm=1, visc=1e-5,
                 thermo="moist", pbot=101540., micro="2mom_warm", Nc0=70.e6),
    # dycoms (cases/dycoms/dycoms.ini): rico's physics plus Radiation_gcss, pbot = 101780 Pa, datetime_utc = 2001-06-09 00:00:00 (day 160
    # of the year plus the day fraction); HotPath(..., thermo=thermo.Moist(pbot), micro=microphys.Warm2mom(Nc0),
    # radiation=radiation.Gcss(xka, fr0, fr1, div, lat, lon, day_of_year)) switches the physics on. The schemes are those of bomex and
    # rico; this fork's dycoms.ini names advec_2i3.
    "dycoms": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(6400., 6400., 1500.), nscalars=4, sm=1, visc=1e-5,
                   thermo="moist", pbot=101780., micro="2mom_warm", Nc0=70.e6,
                   radiation="gcss", xka=85., fr0=70., fr1=22., div=3.75e-6, lat=32.5, lon=0., day_of_year=160.),
    # rcemip (cases/rcemip/rcemip.ini: 1600 m x 1600 m x 32250 m at 8 x 8 columns, the horizontal size scaled with the column count):
    # Thermo_moist with Microphys_nsw6, scalars 0 = thl, 1 = qt, 2 = qr, 3 = qs, 4 = qg, pbot = 101480 Pa;
    # HotPath(..., thermo=thermo.Moist(pbot), micro=microphys.Nsw6(Nc0)) switches the physics on. Its radiation (rrtmgp) is not here.
    "rcemip": dict(advec=ADVEC_2I5, diff=DIFF_SMAG2, pres=2, order=2, gc=(3, 3, 1), size=(12800., 12800., 32250.), nscalars=5, sm=1, visc=1e-5,
                   thermo="moist", pbot=101480., micro="nsw6", Nc0=100.e6),
}

FIELDS3 = ("u", "v", "w", "ut", "vt", "wt")
SURF = ("u_fluxbot", "u_fluxtop", "v_fluxbot", "v_fluxtop", "s_fluxbot", "s_fluxtop", "dudz", "dvdz", "dbdz", "z0m")


def synthetic_global(case, itot, jtot, ktot, dtype=np.float64, seed=666, nscalars=None):
    """Global synthetic fields on the host (interior only; ghosts are filled by the halo code). For tests that
    compare a slab-decomposed run with a single-rank run. nscalars: scalars to make (None = the case's count); every
    one follows scalar 0's recipe."""
    cfg = CASES[case]
    rs = np.random.RandomState(seed)
    n3, n2 = (ktot, jtot, itot), (jtot, itot)
    out = {"u": rs.uniform(-1, 1, n3), "v": rs.uniform(-1, 1, n3), "w": rs.uniform(-.5, .5, n3),
           "ut": rs.uniform(0, 1e-3, n3), "vt": rs.uniform(0, 1e-3, n3), "wt": rs.uniform(0, 1e-3, n3)}
    out["w"][0] = 0; out["wt"][0] = 0
    z = (np.arange(ktot) + 0.5) * cfg["size"][2] / ktot
    for n in range(cfg["nscalars"] if nscalars is None else nscalars):
        out["s%d" % n] = 300. + 0.003*z[:, None, None] + rs.uniform(-.05, .05, n3)
        out["st%d" % n] = rs.uniform(0, 1e-4, n3)
    if cfg.get("thermo") == "moist" and "s1" in out:
        from .thermo import bomex_interior
        out["s0"], out["s1"] = bomex_interior(z, n3, rs)
    if case == "rcemip" and "s1" in out:
        from .thermo import rcemip_interior
        out["s0"], out["s1"] = rcemip_interior(z, n3, rs)
    if cfg.get("radiation") == "gcss" and "s1" in out:
        from .radiation import synthetic_stratocumulus
        out["s0"], out["s1"] = synthetic_stratocumulus(z, n3, rs)
    if cfg.get("micro") == "2mom_warm" and "s3" in out:
        from .microphys import synthetic_rain
        out["s2"], out["s3"] = synthetic_rain(z, n3, rs)
        out["st2"], out["st3"] = rs.uniform(-1e-8, 1e-8, n3), rs.uniform(-1., 1., n3)
    if cfg.get("micro") == "nsw6" and "s4" in out:
        from .microphys import synthetic_precip
        out["s2"], out["s3"], out["s4"] = synthetic_precip(z, n3, rs)
        out["st2"], out["st3"], out["st4"] = (rs.uniform(-1e-8, 1e-8, n3) for _ in range(3))
    for k in SURF:
        out[k] = rs.uniform(0, 1e-4 if k == "dbdz" else 1e-2, n2)
    out["z0m"][:] = 0.1
    return {k: v.astype(dtype) for k, v in out.items()}


class HotPath:
    """Device-resident fields of ONE rank + the operator calls of one sub-step."""

    def __init__(self, case, itot, jtot, ktot, dtype=np.float64, device="cuda:0", seed=666, dt=1.0,
                 lib=None, npy=1, rank=0, group=None, global_init=None, force_slab=False, slim_halos=True, overlap=None, pres_chunks=None, igc=None,
                 nscalars=None, forcing=None, surface=None, thermo=None, micro=None, radiation=None, stats=None, budget=None, cross=None, ib=None,
                 source=None, decay=None, outflow=None):
        import torch
        if budget is not None and stats is None:
            raise ValueError("budget= needs stats=Stats(...): the budget profiles are averaged under the masks of the statistics")
        self.torch = torch
        self.lib = lib if lib is not None else capi.lib()
        self.cfg = cfg = CASES[case]
        self.case, self.dt, self.npy, self.rank, self.group = case, dt, npy, rank, group
        # scalars carried (None = the case's count): th plus, e.g., qt or passive tracers, each made like scalar 0
        nsc = cfg["nscalars"] if nscalars is None else int(nscalars)
        if not 0 <= nsc <= capi.MAX_SCALARS:
            raise ValueError("nscalars must lie in [0, %d]" % capi.MAX_SCALARS)
        # slab code path (halo pack/unpack, split pressure solve); force_slab runs it on ONE rank with the exchanges
        # degenerated to local copies, which is how the slab kernels are exercised on a single-GPU box
        self.slab = (npy > 1) or force_slab
        # slim_halos: exchange only what the next kernel reads across the slab edge (one row of vt and of p, one direction
        # each) and evaluate evisc on the two adjacent ghost rows locally instead of exchanging it
        self.slim = bool(slim_halos)
        # overlap: work the rows that need no north-south halo while the prognostic halos travel on a second stream
        # (halo_visc_rhs). The default with more than one rank (None = auto; MHH_OVERLAP=0 / overlap=False switch it off,
        # MHH_OVERLAP=1 / overlap=True force it, also on one rank with force_slab): the exchange it hides (25.5 MB each way per
        # rank at 512^3 / 8) costs more on the wire than the ~0.2 ms of smaller edge launches the split adds.
        env = os.environ.get("MHH_OVERLAP")
        if env in ("0", "1"):                        # the environment wins over the argument, both ways
            overlap = (env == "1")
        elif overlap is None:
            overlap = npy > 1
        self.overlap = bool(overlap)
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            # the C ABI allocates plan buffers with hipMalloc on the CURRENT device and launches on a raw stream handle: make
            # this HotPath's device the current one (cuda:N without a prior torch.cuda.set_device(N) would otherwise put the
            # plan on device 0 and the fields on device N)
            torch.cuda.set_device(self.device)
        # MHH_FORCE_COMM=1 (tests): with one rank, still send the halos / transposes / maxima through the process group (to
        # self) instead of the local-copy shortcuts -- exercises the real RCCL calls on a one-GPU box
        self.master = Master(npy, rank, group, self.device, os.environ.get("MHH_FORCE_COMM", "0") == "1")
        # bench.py: device-event pairs around every exchange (tag, start, end) while comm_timing is a list
        self.comm_timing = None
        z = moser_z(ktot, cfg["size"][2]) if case == "moser600" else None
        # igc: ghost cells in x beyond what the schemes need -- what the reference's grid produces when an operator calls
        # Grid::set_minimum_ghost_cells (src/grid.cxx:435-439; src/advec_2i5.cxx:42-45 uses it). igc = 16 with itot = 512 makes
        # rows of 544 cells = 34 whole 128-byte lines with istart on a line (fp64).
        self.grid = g = Grid(itot, jtot, ktot, *cfg["size"], order=cfg["order"], igc=max(cfg["gc"][0], igc or 0), jgc=cfg["gc"][1], kgc=cfg["gc"][2],
                             z=z, dtype=dtype, npy=npy, mpicoordy=rank)
        self.G = g.device_struct(self.device) if self.on_gpu else g.host_struct()
        self.td = td = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        n3, n2 = g.shape3, g.shape2
        if global_init is None and cfg.get("thermo") == "moist" and nsc >= 2:
            # thl and qt are the one BOMEX recipe (thermo.bomex_interior), which synthetic_global draws on the host
            global_init = synthetic_global(case, itot, jtot, ktot, dtype=dtype, seed=seed, nscalars=nsc)
        if global_init is None:
            gen = torch.Generator(device=self.device); gen.manual_seed(seed + 7919*rank)

            def rnd(shape, lo=0.0, hi=1.0):
                return (torch.rand(shape, generator=gen, device=self.device, dtype=td) * (hi - lo) + lo).contiguous()
            self.u, self.v, self.w = rnd(n3, -1, 1), rnd(n3, -1, 1), rnd(n3, -0.5, 0.5)
            self.ut, self.vt, self.wt = rnd(n3, 0, 1e-3), rnd(n3, 0, 1e-3), rnd(n3, 0, 1e-3)
            zc = torch.from_numpy(g.z.astype(np.float64)).to(self.device).to(td)
            s0 = 0. if cfg.get("thermo") == "buoy" else 300.          # a buoyancy b has no reference level
            self.s = [(s0 + 0.003*zc[:, None, None] + rnd(n3, -0.05, 0.05)).contiguous() for _ in range(nsc)]
            self.st = [rnd(n3, 0, 1e-4) for _ in range(nsc)]
            self.surf = {k: rnd(n2, 0, 1e-2) for k in SURF}
            self.surf["dbdz"] = rnd(n2, 0, 1e-4)
            self.surf["z0m"] = torch.full(n2, 0.1, device=self.device, dtype=td)
        else:
            j0 = rank * g.jmax

            def put3(a):
                t = torch.zeros(n3, dtype=td)
                t[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend] = torch.from_numpy(np.ascontiguousarray(a[:, j0:j0+g.jmax, :]))
                return t.to(self.device).contiguous()

            def put2(a):
                t = torch.zeros(n2, dtype=td)
                t[g.jstart:g.jend, g.istart:g.iend] = torch.from_numpy(np.ascontiguousarray(a[j0:j0+g.jmax, :]))
                return t.to(self.device).contiguous()
            for n in FIELDS3:
                setattr(self, n, put3(global_init[n]))
            self.s = [put3(global_init["s%d" % n]) for n in range(nsc)]
            self.st = [put3(global_init["st%d" % n]) for n in range(nsc)]
            self.surf = {k: put2(global_init[k]) for k in SURF}
            if cfg.get("thermo") == "moist":     # the mean profiles of thl and qt are read on the ghost levels too: zero gradient there
                for t in self.s[:2] + (self.s[2:] if micro is not None else []):       # (as are qr and nr, or qr, qs and qg, by sedimentation's slopes)
                    t[:g.kstart] = t[g.kstart]; t[g.kend:] = t[g.kend-1]
        if surface is not None:          # before the mixing-length table below is made from it
            self.surf["z0m"].fill_(float(surface.z0m))
        # solid walls: w and its tendency vanish at kstart and above kend-1
        self.w[:g.kstart+1] = 0; self.w[g.kend:] = 0
        self.wt[:g.kstart+1] = 0; self.wt[g.kend:] = 0
        self.evisc = torch.zeros(n3, device=self.device, dtype=td)
        self.p = torch.zeros(n3, device=self.device, dtype=td)
        ones = np.ones(g.kcells, dtype=g.np_dtype)
        self.rhoref_h, self.rhorefh_h = ones.copy(), ones.copy()
        self.rhoref, self.rhorefh = torch.from_numpy(ones.copy()).to(self.device), torch.from_numpy(ones.copy()).to(self.device)
        self.thref = torch.full((g.kcells,), 300., device=self.device, dtype=td)
        self.work = torch.zeros(16, device=self.device, dtype=torch.float64)
        # Thermo_moist (thermo.Moist): the base-state tables, and the density of the dynamics before the pressure plan is made from it
        self.thermo = None
        if thermo is not None:
            self.thermo = thermo.bind(self)
        # Diff_smag2::prepare_device: per-level mixing-length table from the host libm
        self.params = p = capi.MhhDiffParams()
        p.cs, p.tPr, p.surface_model, p.neutral, p.N2, p.th_for_N2, p.grav = cfg.get("cs", 0.23), cfg.get("tPr", 1./3.), cfg["sm"], 0, None, 0, 9.81
        p.thref = self.thref.data_ptr()
        # Thermo_buoy: scalar 0 is b. Its N2 is evaluated inside exec_viscosity, and Thermo_buoy::exec (flat form: no slope, no
        # background N2) is folded into the RHS pass as the first term of wt (src/model.cxx:366,388)
        self.buoyant = cfg.get("thermo") == "buoy" and nsc >= 1
        if self.buoyant:
            p.buoyancy, p.buoyancy_kind, p.bg_n2, p.alpha, p.utrans = cfg["order"], 1, 0., 0., 0.
        if self.thermo is not None:           # N2 inside exec_viscosity from thl and thvref; the tendency is a pass of its own
            self.thermo.diff_params(p)
        if cfg["diff"] == DIFF_SMAG2:
            ml = np.zeros(g.kcells, dtype=g.np_dtype)
            self._ok(self.lib.mhh_smag2_mlen0_host(g.host_struct(), p.cs, ml.ctypes.data))
            self.mlen0 = torch.from_numpy(ml).to(self.device)
            p.mlen0 = self.mlen0.data_ptr()
            # Diff_smag2::prepare_device, continued: a horizontally uniform roughness length makes the squared mixing length a
            # per-level table (same bits as the per-cell evaluation; three divisions and a square root per cell less)
            z0 = self.surf["z0m"]
            if bool((z0 == z0.flatten()[0]).all()):
                m2 = np.zeros(g.kcells, dtype=g.np_dtype)
                self._ok(self.lib.mhh_smag2_mlen2_host(g.host_struct(), p.surface_model, p.neutral, ml.ctypes.data, float(z0.flatten()[0]), m2.ctypes.data))
                self.mlen2 = torch.from_numpy(m2).to(self.device)
                p.mlen2 = self.mlen2.data_ptr()
        self.fields = self._fields()
        # Pres::init / set_values / prepare_device
        self.plan = capi.PLAN()
        Gh = g.host_struct()
        if not self.slab:
            self._ok(self.lib.mhh_pres_plan_create(Gh, cfg["pres"], g.dz.ctypes.data, g.dzhi.ctypes.data, g.dzi4.ctypes.data, g.dzhi4.ctypes.data,
                                                   self.rhoref_h.ctypes.data, self.rhorefh_h.ctypes.data, C.byref(self.plan)))
        else:
            self._ok(self.lib.mhh_pres_slab_plan_create_order(Gh, cfg["pres"], g.dz.ctypes.data, g.dzhi.ctypes.data, g.dzi4.ctypes.data, g.dzhi4.ctypes.data,
                                                              self.rhoref_h.ctypes.data, self.rhorefh_h.ctypes.data, C.byref(self.plan)))
            nx = int(self.lib.mhh_pres_slab_xbuf_elems(self.plan))
            self.xsend = torch.zeros(2*nx, device=self.device, dtype=td)
            self.xrecv = torch.zeros(2*nx, device=self.device, dtype=td)
            self._halo = {}
            # k-slices of the pressure solve: the all-to-all of slice c travels (second stream) while slice c+1 is transformed.
            # Default with more than one rank: 4 slices where ktot allows (MHH_PRES_CHUNKS / pres_chunks override; 1 = unsliced).
            if pres_chunks is None:
                env = os.environ.get("MHH_PRES_CHUNKS")
                pres_chunks = int(env) if env else (4 if npy > 1 else 1)
            pres_chunks = max(1, int(pres_chunks))
            while pres_chunks > 1 and (ktot % pres_chunks or not self.slim):
                pres_chunks -= 1
            self.pres_chunks = pres_chunks
            self._ok(self.lib.mhh_pres_slab_set_chunks(self.plan, pres_chunks))
        self._prog = [self.u, self.v, self.w] + self.s
        # (with a surface layer dudz, dvdz, dbdz change every sub-step and are written on the interior only, as in the reference:
        # evisc is then exchanged like any field instead of being re-evaluated on the ghost rows)
        # (with open boundaries for scalar 0, which feeds N2, the re-evaluated ghost rows would differ from the reference's cyclic
        # fill of evisc at South and North: exchanged too, see outflow.py)
        self.evisc_local_ghosts = (self.slab and self.slim and cfg["diff"] == DIFF_SMAG2 and g.jgc >= 2 and surface is None
                                   and not (outflow is not None and 0 in outflow.scalars))
        if self.evisc_local_ghosts:
            p.evisc_ghost_rows = 1
            for k in ("dudz", "dvdz", "dbdz", "z0m"):
                self._halo2d(self.surf[k])
        # Buffer and Force (forcing.Forcing): their tables, the mean profiles and the reduction scratch, made once
        self.forcing = forcing.bind(self) if forcing is not None else None
        # Boundary_surface (surface.Surface): its state (ustar, obuk, nobuk), the lookup table and one s_fluxbot / sbot / sgradbot per scalar
        self.surface = surface.bind(self) if surface is not None else None
        # Microphys_2mom_warm and Limiter (microphys.Warm2mom): the rain rate, sedimentation's scratch
        self.micro = micro.bind(self) if micro is not None else None
        # Radiation_gcss (radiation.Gcss): the zenith angle, two scratch fields
        self.radiation = radiation.bind(self) if radiation is not None else None
        # Immersed_boundary (ib.Dem): the ghost-cell tables of u, v, w and s, the mask fields and k_dem, made once on the host
        self.ib = ib.bind(self) if ib is not None else None
        # Source and Decay (source.Sources, source.Decay): the sources' ranges, norms and device tables, made once on the host;
        # in front of Stats, whose couvreux mask asks the decay for its scalar
        self.source = source.bind(self) if source is not None else None
        self.decay = decay.bind(self) if decay is not None else None
        # Boundary_outflow (outflow.Outflow): the inflow tables of the open scalars on the device, the edges this rank owns
        self.outflow = outflow.bind(self) if outflow is not None else None
        # Stats (stats.Stats): the mask words, counts and reduction scratch; sampled outside the step by hp.stats.sample()
        self.stats = stats.bind(self) if stats is not None else None
        # Budget_2 (budget.Budget2): the budget group of the statistics, sampled with them after Stats' own passes
        self.budget = budget.bind(self) if budget is not None else None
        # Cross (cross.Cross): the index lists, the job table and the staging buffers; sampled outside the step by hp.cross.sample(iotime)
        self.cross = cross.bind(self) if cross is not None else None
        self.cyclic_prognostic()
        self.sync()

    # -- plumbing -----------------------------------------------------------------------------------------
    def _ok(self, rc):
        capi.check(rc, self.lib)

    def sync(self):
        if self.on_gpu:
            self.torch.cuda.synchronize(self.device)

    _host_staged = property(lambda self: self.master.mode == "host_staged")
    _force_comm = property(lambda self: self.master.force_comm)

    @property
    def stream(self):
        if not self.on_gpu:
            return C.c_void_p(0)
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _fields(self):
        f = capi.MhhFields()
        for n in ("u", "v", "w", "ut", "vt", "wt", "evisc", "p", "rhoref", "rhorefh"):
            setattr(f, n, getattr(self, n).data_ptr())
        f.nscalars = len(self.s)
        for n in range(len(self.s)):
            f.s[n], f.st[n], f.svisc[n] = self.s[n].data_ptr(), self.st[n].data_ptr(), self.cfg["visc"]
            f.s_fluxbot[n], f.s_fluxtop[n] = self.surf["s_fluxbot"].data_ptr(), self.surf["s_fluxtop"].data_ptr()
        f.visc = self.cfg["visc"]
        for n in ("u_fluxbot", "u_fluxtop", "v_fluxbot", "v_fluxtop", "dudz", "dvdz", "dbdz", "z0m"):
            setattr(f, n, self.surf[n].data_ptr())
        return f

    @staticmethod
    def _ptrs(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    # -- halos ------------------------------------------------------------------------------------------------
    def halo(self, tensors, rows_south=None, rows_north=None):
        """Periodic ghost cells of 3-D fields: east-west wrap on the device, north-south wrap locally (npy == 1) or
        by exchanging rows with the ring neighbours (Boundary_cyclic::exec, src/boundary_cyclic.cxx:116-176).
        rows_south / rows_north: how many of my southernmost / northernmost interior rows travel to the south / north
        neighbour (default jgc each = the reference's full exchange)."""
        arr = self._ptrs(tensors)
        if not self.slab:
            self._ok(self.lib.mhh_boundary_cyclic_n(self.G, arr, len(tensors), EDGE_BOTH, self.stream))
            return
        self._ok(self.lib.mhh_boundary_cyclic_n(self.G, arr, len(tensors), EDGE_EW, self.stream))
        self._exchange_ns(tensors, rows_south, rows_north)

    def _exchange_ns(self, tensors, rows_south=None, rows_north=None):
        """North-south part of halo(): pack, ring exchange (or local swap on one rank), unpack -- on the current stream."""
        arr = self._ptrs(tensors)
        g, nf = self.grid, len(tensors)
        rs = g.jgc if rows_south is None else rows_south
        rn = g.jgc if rows_north is None else rows_north
        nn, ns = rn * nf * g.kcells * g.icells, rs * nf * g.kcells * g.icells
        if (nf, rs, rn) not in self._halo:                   # one send and one receive buffer, [northbound | southbound]
            self._halo[nf, rs, rn] = [self.torch.zeros(max(1, nn + ns), device=self.device, dtype=self.td) for _ in range(2)]
        send, recv = self._halo[nf, rs, rn]
        off_s = nn * send.element_size()                     # (an empty view has a null data_ptr: offsets by hand)
        self._ok(self.lib.mhh_halo_pack_rows(self.G, arr, nf, rs, rn, send.data_ptr() + off_s, send.data_ptr(), self.stream))
        with self._timed("halo"):
            self.master.ring(send, recv, nn, ns)
        self._ok(self.lib.mhh_halo_unpack_rows(self.G, arr, nf, rs, rn, recv.data_ptr(), recv.data_ptr() + off_s, self.stream))

    @contextlib.contextmanager
    def _timed(self, tag, on=True):
        """Records a pair of events on the current stream around an exchange when comm_timing is on."""
        on = on and self.comm_timing is not None and self.on_gpu
        if on:
            a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            a.record()
        yield
        if on:
            b.record(); self.comm_timing.append((tag, a, b))

    def _halo2d(self, t):
        """One-time periodic ghost cells of a 2-D surface array (Boundary_cyclic::exec_2d, src/boundary_cyclic.cxx:445-500)."""
        g = self.grid
        if self.master.mode == "local":
            self._ok(self.lib.mhh_boundary_cyclic_2d(self.G, t.data_ptr(), self.stream))
            return
        t[:, :g.igc] = t[:, g.iend-g.igc:g.iend].clone(); t[:, g.iend:] = t[:, g.istart:g.istart+g.igc].clone()
        send = self.torch.cat([t[g.jend-g.jgc:g.jend], t[g.jstart:g.jstart+g.jgc]]).reshape(-1)      # [northbound | southbound]
        recv = self.torch.empty_like(send)
        self.master.ring(send, recv, send.numel() // 2, send.numel() // 2)
        t[:g.jgc], t[g.jend:] = recv.view(2, g.jgc, -1)

    def cyclic_prognostic(self):
        self.halo(self._prog)

    def outflow_bcs(self):
        """boundary->set_prognostic_outflow_bcs (src/model.cxx:347, :383): nothing without `outflow`."""
        if self.outflow is not None:
            self.outflow.exec()

    # -- the north-south exchange of the prognostic fields hidden behind the rows that do not need it -------------------
    @property
    def can_overlap(self):
        g = self.grid
        return (self.slab and self.overlap and self.evisc_local_ghosts and self.outflow is None and self.cfg["advec"] == ADVEC_2I5 and self.cfg["diff"] == DIFF_SMAG2
                and len(self.s) >= 1 and g.jgc >= 3 and g.jmax >= 12)      # 1 .. MHH_MAX_SCALARS scalars, none flux-limited (HotPath limits none): as Substep_slab::can_overlap

    def halo_visc_rhs(self, ev=None):
        """cyclic_prognostic + exec_viscosity + rhs of a slab rank with the halo exchange of u, v, w, th (jgc rows of four
        fields each way: the largest message of the step) travelling on a second stream while the rows that need no
        north-south halo are worked: evisc on rows [jstart+1, jend-1), tendencies on rows [jstart+4, jend-4); then the
        edge rows. Row-wise calls give the bits of the whole-slab calls (tests/test_slab_gloo.py)."""
        g, lib, torch = self.grid, self.lib, self.torch
        adv, dif = self.cfg["advec"], self.cfg["diff"]
        F, P = C.byref(self.fields), C.byref(self.params)
        self._ok(lib.mhh_boundary_cyclic_n(self.G, self._ptrs(self._prog), len(self._prog), EDGE_EW, self.stream))
        if self.on_gpu:
            main = torch.cuda.current_stream(self.device)
            comm, cev = self.master.side_stream()
            cev[0].record(main)
            comm.wait_event(cev[0])
            with torch.cuda.stream(comm):
                self._exchange_ns(self._prog)
                cev[1].record(comm)
        else:
            self._exchange_ns(self._prog)
        ja, jb = g.jstart + 4, g.jend - 4
        if ev is not None:
            ev[2].record()
        self._ok(lib.mhh_diff_exec_viscosity_rows(self.G, dif, F, P, g.jstart + 1, g.jend - 1, self.stream))
        if ev is not None:
            ev[0].record()
        self._ok(lib.mhh_rhs_exec_rows(self.G, adv, dif, F, P, ja, jb, self.stream))
        if ev is not None:
            ev[1].record()
        self.rhs_rows_timed = jb - ja
        if self.on_gpu:
            torch.cuda.current_stream(self.device).wait_event(cev[1])
        # both edge strips in one launch each
        self._ok(lib.mhh_diff_exec_viscosity_rows2(self.G, dif, F, P, g.jstart - 1, g.jstart + 1, g.jend - 1, g.jend + 1, self.stream))
        self._ok(lib.mhh_rhs_exec_rows2(self.G, adv, dif, F, P, g.jstart, ja, jb, g.jend, self.stream))

    # -- the operator calls -----------------------------------------------------------------------------------
    def exec_viscosity(self):
        self._ok(self.lib.mhh_diff_exec_viscosity(self.G, self.cfg["diff"], C.byref(self.fields), C.byref(self.params), self.stream))
        if self.slab and self.cfg["diff"] == DIFF_SMAG2 and not self.evisc_local_ghosts:
            self.halo([self.evisc])

    def rhs(self):
        self._ok(self.lib.mhh_rhs_exec(self.G, self.cfg["advec"], self.cfg["diff"], C.byref(self.fields), C.byref(self.params), self.stream))

    def rhs_unfused(self):
        if self.buoyant:            # Thermo_buoy::exec on its own, then Advec::exec and Diff::exec
            p = self.params
            self._ok(self.lib.mhh_thermo_buoy_tend(self.G, p.buoyancy, C.byref(self.fields), p.th_for_N2, p.alpha, p.bg_n2, p.utrans, self.stream))
        self._ok(self.lib.mhh_advec_exec(self.G, self.cfg["advec"], C.byref(self.fields), self.stream))
        self._ok(self.lib.mhh_diff_exec(self.G, self.cfg["diff"], C.byref(self.fields), C.byref(self.params), self.stream))

    # the rows of vt the pressure input reads beyond the slab (rows_south, rows_north): pres_2 vt[j+1] (src/pres_2.cxx:181,193),
    # pres_4 vt[j-1..j+2] (src/pres_4.cxx:312-315)
    @property
    def _pres_vt_rows(self):
        return (2, 1) if self.cfg["pres"] == 4 else (1, 0)

    def pres(self):
        """Pres_2::exec / Pres_4::exec (src/pres_2.cxx:66-94, src/pres_4.cxx:64-140). On a slab, in pres_chunks k-slices: per slice x
        transform + pack, its all-to-all (with more than one slice: on the exchange stream while the next slice is transformed), y
        transform as each slice arrives; the column solves over all levels; the same on the way back. Same kernels per plane
        whatever the slice count (tests/test_slab_gloo.py, tests/test_slab4_gloo.py compare one slice with several)."""
        if not self.slab:
            self._ok(self.lib.mhh_pres_exec(self.plan, self.G, C.byref(self.fields), self.dt, self.stream))
            return
        lib, torch, n, order = self.lib, self.torch, self.pres_chunks, self.cfg["pres"]
        P, G, F = self.plan, self.G, C.byref(self.fields)
        if self.slim or order == 4: self.halo([self.vt], *self._pres_vt_rows)
        else:                       self.halo([self.vt])
        # x stages with the transforms in LDS where the plan has them (pres_2; needs the slim halos: p's y halo is the one row): input
        # + x transform write the send buffer, x transform + p + output read the receive buffer -- no packed array, no pack / unpack;
        # the y transforms read / write the transposes' buffers directly
        lds_x = self.slim and lib.mhh_pres_slab_has_lds(P) == 1
        packed = lib.mhh_pres_slab_packed(P)
        xs, xr = self.xsend.data_ptr(), self.xrecv.data_ptr()
        if lds_x:
            x_in = lambda c: lib.mhh_pres_slab_lds_fwd(P, G, F, self.dt, xs, c, self.stream)      # noqa: E731
            y_in = lambda c: lib.mhh_pres_slab_lds_fwd_y(P, G, xr, c, self.stream)                # noqa: E731
            y_out = lambda c: lib.mhh_pres_slab_lds_bwd_y(P, G, xs, c, self.stream)               # noqa: E731
            x_out = lambda c: lib.mhh_pres_slab_lds_bwd(P, G, xr, F, c, self.stream)              # noqa: E731
        else:
            self._ok(lib.mhh_pres_input_packed(G, order, F, self.dt, packed, self.stream))
            x_in = lambda c: lib.mhh_pres_fwd_x_pack_chunk(P, G, packed, xs, c, self.stream)      # noqa: E731
            y_in = lambda c: lib.mhh_pres_fwd_y_chunk(P, G, xr, c, self.stream)                   # noqa: E731
            y_out = lambda c: lib.mhh_pres_bwd_y_chunk(P, G, xs, c, self.stream)                  # noqa: E731
            x_out = lambda c: lib.mhh_pres_bwd_x_chunk(P, G, xr, c, self.stream)                  # noqa: E731
        # one slice: the transposes run on the caller's stream
        two_streams = n > 1 and self.on_gpu and self.master.mode == "direct"
        if two_streams:
            main = torch.cuda.current_stream(self.device)
            comm, sl_ev = self.master.side_stream()[0], self.master.slice_events(n)
        seg = self.xsend.numel() // n

        def exchange(c, way):
            """all-to-all of slice c (way 0: Transpose::exec_xy, 2: exec_yx): on the exchange stream once `ready` (recorded on the
            main stream) has passed"""
            a, b = self.xsend[c*seg:(c+1)*seg], self.xrecv[c*seg:(c+1)*seg]
            if not two_streams:
                self._transpose(a, b)
                return
            ready, done = sl_ev[way][c], sl_ev[way+1][c]
            ready.record(main)
            comm.wait_event(ready)
            with torch.cuda.stream(comm):
                self._transpose(a, b)
                done.record(comm)

        def arrived(c, way):
            if two_streams:
                main.wait_event(sl_ev[way+1][c])

        for c in range(n):
            self._ok(x_in(c)); exchange(c, 0)
        for c in range(n):
            arrived(c, 0); self._ok(y_in(c))
        self._ok(lib.mhh_pres_solve_y(P, G, self.stream))
        for c in range(n):
            self._ok(y_out(c)); exchange(c, 2)
        for c in range(n):
            arrived(c, 2); self._ok(x_out(c))
        if order == 2 and self.slim:
            # unpack + Pres_2::output in one kernel (the LDS x stage has done both) for everything but vt on the southernmost row,
            # whose p[j-1] arrives with the one-row halo of p (pres_2.cxx:383-385)
            if not lds_x:
                self._ok(lib.mhh_pres_unpack_output_slab(P, G, F, self.stream))
            self.halo([self.p], rows_south=0, rows_north=1)
            self._ok(lib.mhh_pres_output_south_row(G, F, self.stream))
        else:
            # the unpack writes p's mirrored ghost levels and its x halo, the exchange its y halo (pres_4: the output reads
            # p[j-2..j+1], src/pres_4.cxx:555-569)
            self._ok(lib.mhh_pres_unpack_slab(P, G, F, self.stream))
            if order == 4: self.halo([self.p], rows_south=1, rows_north=2)
            else:          self.halo([self.p])
            self._ok(lib.mhh_pres_output_order(G, order, F, self.stream))

    def pres_rk(self, rkorder, substep, dt):
        """pres->exec(self.dt) followed by timeloop.exec() for u, v, w (src/model.cxx:411,484) with the sub-step applied in the
        kernel that stores the corrected tendencies (mhh_pres_exec_rk); on a slab: pres() + three mhh_rk_substep calls."""
        if not self.slab:
            self._ok(self.lib.mhh_pres_exec_rk(self.plan, self.G, C.byref(self.fields), self.dt, rkorder, substep, dt, self.stream))
            return
        self.pres()
        for a, at in ((self.u, self.ut), (self.v, self.vt), (self.w, self.wt)):
            self._ok(self.lib.mhh_rk_substep(self.G, rkorder, substep, dt, a.data_ptr(), at.data_ptr(), self.stream))

    def _transpose(self, xsend, xrecv):
        """x<->y transpose of the spectral pressure (or of one k-slice of it): Master.all_to_all, timed where it is direct."""
        with self._timed("transpose", self.master.mode == "direct"):
            self.master.all_to_all(xsend, xrecv)

    def forcing_means(self):
        """fields->exec() (src/model.cxx:351): the horizontal means the forcing switches read, summed over the slab ranks."""
        self.forcing.means()

    def buffer_force(self):
        """buffer->exec and force->exec (src/model.cxx:395,404) in one pass over the tendencies."""
        self.forcing.exec()

    def decay_source(self):
        """decay->exec and source->exec (src/model.cxx:398,401), one launch each."""
        if self.decay is not None:
            self.decay.exec()
        if self.source is not None:
            self.source.exec()

    def thermo_moist(self):
        """thermo->exec (src/model.cxx:366; Thermo_moist::exec, src/thermo_moist.cxx:1273-1303): with swupdatebasestate the base state
        from the means on the device, then the buoyancy tendency of w."""
        if self.thermo.swupdate:
            self.thermo.update_base_state()
        self.thermo.tend()

    def surface_layer(self):
        """boundary->exec and boundary->set_ghost_cells (src/model.cxx:374-375)."""
        self.surface.exec()
        self.surface.ghost_cells()

    def step(self):
        """One full RHS + pressure evaluation (the BASELINE metric's unit of work); with `forcing`, the means it reads and the
        fused Buffer + Force pass between the RHS and the pressure solve. With `surface`, the order of src/model.cxx:346-392: the
        cyclic fills, exec_viscosity (which reads the PREVIOUS sub-step's dudz, dvdz, dbdz, as the reference does), the surface
        layer, the vertical ghost cells, then the RHS -- the plain sequence on a slab too (the overlapped sub-step fuses
        exec_viscosity with the RHS, and the surface layer sits between them). With `thermo` (thermo.Moist), the same plain sequence
        with the means of thl and qt in front of exec_viscosity and Thermo_moist::exec behind it. With `ib` (ib.Dem), the plain
        sequence on a slab too, with the two calls of src/model.cxx:380 and :407: the scalars' ghost cells after the surface layer and
        in front of the RHS, those of u, v, w after Buffer and Force and in front of the pressure solve. With `source` or `decay`
        (source.Sources, source.Decay), the order of src/model.cxx:395-404: Buffer, decay, source, Force -- Buffer and Force as their own
        passes, which have the bits of the fused one; without the two nothing changes. With `outflow` (outflow.Outflow), the open scalars'
        lateral ghost cells directly after the cyclic fills (:347) and once more after ib->exec_scalars (:383) -- the plain sequence on
        a slab too: the overlapped sub-step hides the exchange behind interior rows, and the fill has to follow that exchange."""
        means_done = False
        if self.thermo is not None:
            # Thermo_moist, in the order of Model::exec (src/model.cxx:346-392): the cyclic fills; fields->exec, the means of thl and qt
            # (:351); exec_viscosity, whose N2 reads the thvref the previous sub-step left (:354); thermo->exec, the base state from
            # the means and the buoyancy tendency in front of advec->exec (:366, :388)
            self.cyclic_prognostic()
            self.outflow_bcs()
            if self.thermo.swupdate:
                means_done = self.thermo.means()
            self.exec_viscosity()
            self.thermo_moist()
            if self.micro is not None:         # microphys->exec (:369), between thermo->exec and boundary->exec
                self.micro.exec()
            if self.radiation is not None:     # radiation->exec (:372), between microphys->exec and boundary->exec
                self.radiation.exec()
            if self.surface is not None:       # boundary->exec (:376) reads the thvref, thvrefh thermo->exec has just written
                self.surface_layer()
            if self.ib is not None:            # ib->exec_scalars (:380), after the vertical ghost cells
                self.ib.exec_scalars()
                self.outflow_bcs()
            self.rhs()
        elif self.surface is not None:
            self.cyclic_prognostic()
            self.outflow_bcs()
            self.exec_viscosity()
            self.surface_layer()
            if self.ib is not None:
                self.ib.exec_scalars()
                self.outflow_bcs()
            self.rhs()
        elif self.ib is not None:
            self.cyclic_prognostic()
            self.outflow_bcs()
            self.exec_viscosity()
            self.ib.exec_scalars()
            self.outflow_bcs()
            self.rhs()
        elif self.can_overlap:
            self.halo_visc_rhs()
        else:
            self.cyclic_prognostic()
            self.outflow_bcs()
            self.exec_viscosity()
            self.rhs()
        if self.forcing is not None:
            if not means_done:
                self.forcing_means()
            if self.source is None and self.decay is None:
                self.buffer_force()
            else:
                self.forcing.exec_buffer()
                self.decay_source()
                self.forcing.exec_force()
        elif self.source is not None or self.decay is not None:
            self.decay_source()
        if self.ib is not None:                # ib->exec_momentum (:407), after buffer->exec and force->exec
            self.ib.exec_momentum()
        self.pres()
        if self.micro is not None:             # limiter->exec with the sub-step (:415), the last tendency
            self.micro.limit()

    def capture_step(self):
        """One step recorded as a hipGraph (single GPU): every entry point of the library only enqueues work on the stream it is
        given -- no allocation, no synchronisation, no host round trip inside a step -- so the dozen launches of a step (cyclic
        fills, exec_viscosity, fused RHS, the pressure kernels or rocFFT's) replay as ONE graph launch. Matters where a step is
        short (256^3: 1.6 ms, 64^3: 0.1 ms); returns the graph, `graph.replay()` runs a step on the same fields."""
        assert self.on_gpu and not self.slab, "graph capture: single-GPU path"
        torch = self.torch
        self.step(); self.sync()                       # everything created lazily (rocFFT work areas) exists before the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self.step()
        self._graphs = getattr(self, "_graphs", []) + [graph]      # source.update() resets them: they hold the old tables' launch
        return graph

    def drop_graphs(self):
        """Reset every graph capture_step() has returned: a replay then raises instead of launching over tables that are gone."""
        for g in getattr(self, "_graphs", []):
            g.reset()
        self._graphs = []

    # -- reductions (local max, then Master.max over ranks) ------------------------------------------------------
    def divergence(self):
        out = C.c_double(0)
        self._ok(self.lib.mhh_pres_check_divergence(self.G, self.cfg["pres"], C.byref(self.fields), self.work.data_ptr(), C.byref(out), self.stream))
        return self.master.max(out.value)

    def projected_divergence(self):
        """(max |Pres::input| of the fields as they stand, max |Pres::input| of u, v, w alone), each without its horizontal mean per
        level, MAX over ranks: Pres::input is the
        divergence of u/dt + ut the solve has just removed (src/pres_2.cxx:156-196, src/pres_4.cxx:256-317; its halo and ghost-level
        side effects are the ones the next Pres::exec would apply anyway), the second number the scale to read the first against.
        A self-check of the (distributed) solve for bench.py and the tests, outside any timed region."""
        torch, g = self.torch, self.grid
        buf = torch.empty(g.imax*g.jmax*g.kmax, device=self.device, dtype=self.td)

        def residual(f, real):
            if self.slab:
                if real:
                    rs, rn = self._pres_vt_rows
                    self.halo([self.vt], rows_south=rs, rows_north=rn)
                self._ok(self.lib.mhh_pres_input_packed(self.G, self.cfg["pres"], C.byref(f), self.dt, buf.data_ptr(), self.stream))
            else:
                self._ok(self.lib.mhh_pres_input(self.plan, self.G, C.byref(f), self.dt, buf.data_ptr(), self.stream))
            self.sync()
            # without the horizontal mean of each level: the mode (0, 0) has a boundary condition of its own on top (Dirichlet:
            # src/pres_2.cxx:311-316, src/pres_4.cxx:421-446) and pres_4 does not enforce its equation on the top levels -- with
            # synthetic fields, whose w has a horizontal mean, that mode is left with a remainder that says nothing about the solve
            r = buf.view(g.kmax, g.jmax, g.imax)
            lev = self.master.sum_(r.sum(dim=(1, 2), dtype=torch.float64))
            mean = (lev / float(g.itot * g.jtot)).to(self.td)
            return self.master.max(float((r - mean[:, None, None]).abs().max().item()))
        d1 = residual(self.fields, True)
        zero = torch.zeros_like(self.ut)
        f0 = self._fields()
        f0.ut = f0.vt = f0.wt = zero.data_ptr()
        d0 = residual(f0, False)
        return d1, d0

    def cfl(self, dt):
        out = C.c_double(0)
        self._ok(self.lib.mhh_advec_cfl(self.G, self.cfg["advec"], self.u.data_ptr(), self.v.data_ptr(), self.w.data_ptr(), dt, self.work.data_ptr(), C.byref(out), self.stream))
        return self.master.max(out.value)

    # -- restart files in the reference's layout (microhh_amd/fieldio.py; src/field3d_io.cxx:54-230) ------------------
    def _restart_fields(self):
        names = [("u", self.u), ("v", self.v), ("w", self.w)]
        names += [("th" if n == 0 else "s%d" % n, t) for n, t in enumerate(self.s)]
        return names

    def save(self, path, iteration=0):
        """Write the prognostic fields as `name.NNNNNNN`; slab ranks write their rows of the one global file. Rank 0 creates
        every file at its full size, all ranks meet at a barrier, each writes its rows, and a second barrier ends the call
        (a reader on another rank then sees complete files)."""
        from . import fieldio
        names = [(fieldio.field_filename(path, name, iteration), t) for name, t in self._restart_fields()]
        if self.rank == 0:
            fieldio.save_grid(path, self.grid, jtot=self.grid.jmax * self.npy)
            if self.npy > 1:
                for fn, _ in names:
                    fieldio.prepare_global_file(fn, self.grid, self.npy)
        self.master.barrier()
        for fn, t in names:
            fieldio.save_field3d(fn, t.detach().cpu().numpy(), self.grid, rank=self.rank, npy=self.npy)
        self.master.barrier()

    def load(self, path, iteration=0):
        """Read the prognostic fields' interiors back (ghost cells are refreshed by the next cyclic_prognostic())."""
        from . import fieldio
        for name, t in self._restart_fields():
            a = fieldio.load_field3d(fieldio.field_filename(path, name, iteration), self.grid, rank=self.rank, npy=self.npy,
                                     out=t.detach().cpu().numpy().copy())
            t.copy_(self.torch.from_numpy(a.reshape(-1)).to(t.device).reshape(t.shape))

    def close(self):
        if self.plan:
            (self.lib.mhh_pres_slab_plan_destroy if self.slab else self.lib.mhh_pres_plan_destroy)(self.plan)
            self.plan = None

    # -- algorithmic bytes per interior cell (SURVEY.md §8d / BASELINE.md §3) -------------------------------------
    def alg_bytes_rhs(self):
        s = self.grid.np_dtype.itemsize
        F = 3 + len(self.s)
        return (3*F)*s if self.cfg["diff"] != DIFF_SMAG2 else (F + 1 + 2*F)*s   # smag2: pass B (tendencies); pass A below

    def alg_bytes_visc(self):
        s = self.grid.np_dtype.itemsize
        return (3 + len(self.s) + 1)*s if self.cfg["diff"] == DIFF_SMAG2 else 0

    def alg_bytes_pres(self):
        return 26*self.grid.np_dtype.itemsize
