"""Cross on the host side: the driver of csrc/cross.h behind HotPath(..., cross=Cross(...)).

The cross-section files of Cross<TF> (src/cross.cxx) with the fields left on the device. The reference runs Cross on the host, in
its GPU build after copying every prognostic field back (src/model.cxx:444-451); here a sample is one gather launch over a job
table (plus one launch per lngrad, path or threshold-height variable), ONE device-to-host copy of the packed staging buffer into a
pinned host buffer, and the writes of fieldio.save_*_slice. What is built, by the class that provides it in the reference:

  Fields (Fields::exec_cross, src/fields.cxx:1221-1271)   u, v, w, every scalar, p, evisc; the suffixes lngrad (fourth order only, as
                                                          check_added_cross has it, :513-518), fluxbot, fluxtop, path, and bot / top
                                                          where the surface layer holds those arrays
  Thermo_moist (src/thermo_moist.cxx:2073-2139)           b, blngrad, ql, qlpath, qlbase, qltop, qi, qipath, qlqipath, qlqibase, qlqitop
  Thermo_dry (src/thermo_dry.cxx:819-845)                 b, blngrad, thlngrad
  Thermo_buoy                                             b is scalar 0: b, blngrad, bfluxbot, ... through Fields
  Microphys (src/microphys_2mom_warm.cxx:950-960, src/microphys_nsw6.cxx:1098-1114)   rr_bot, rs_bot, rg_bot
  Boundary_surface (src/boundary_surface.cxx:688-712)     ustar, obuk
  Radiation_gcss (src/radiation_gcss.cxx:555-560)         lflx, sflx
  Immersed_boundary (src/immersed_boundary.cxx:950-985)   <scalar>fluxbot_ib, with HotPath(..., ib=Dem(...))

A scalar goes by HotPath's names (th, s1, s2, ...; s0 is th) and by the reference's name in the case (thl, qt, qr, nr, qs, qg; b in
a Thermo_buoy case). A name the case cannot provide raises ValueError("... is illegal") at bind time; the reference only warns
(src/cross.cxx:493-497). On a slab (npy > 1) the files are the global ones of the MPI writers (src/field3d_io.cxx:234-...).
"""
import ctypes as C
import os


from . import capi, fieldio

XY, XZ, YZ, PLANE = 0, 1, 2, 3
FILL_HEIGHT = -1e-9                                   # Cross::cross_height_threshold (src/cross.cxx:748)
MOIST_NAMES = {"moist": ("thl", "qt"), "2mom_warm": ("thl", "qt", "qr", "nr"), "nsw6": ("thl", "qt", "qr", "qs", "qg")}


def indices(lib, grid, kind, locations):
    """Cross::create (src/cross.cxx:323-460) for the locations of one direction: (full-level indices, half-level indices), global."""
    n = len(locations)
    loc = (C.c_double*max(n, 1))(*[float(x) for x in locations])
    full, half = (C.c_int*max(n, 1))(), (C.c_int*max(n, 1))()
    nf, nh = C.c_int(0), C.c_int(0)
    capi.check(lib.mhh_cross_indices_host(grid.host_struct(), kind, loc, n, full, C.byref(nf), half, C.byref(nh)), lib)
    return list(full[:nf.value]), list(half[:nh.value])


class Cross:
    """Cross(crosslist, xy=(), xz=(), yz=(), path="."): HotPath(..., cross=Cross(...)), then hp.cross.sample(iotime)."""

    def __init__(self, crosslist, xy=(), xz=(), yz=(), path=".", utrans=None, vtrans=None):
        self.crosslist = list(crosslist)
        if not self.crosslist:
            raise ValueError("Empty cross-section list")                   # src/cross.cxx:271-275
        self.xy, self.xz, self.yz, self.path = tuple(xy), tuple(xz), tuple(yz), path
        self.utrans, self.vtrans = utrans, vtrans

    # -- what the case provides ------------------------------------------------------------------------------------
    def _variables(self, hp):
        """{name: (op, source, loc, offset)}. op: simple | lngrad | plane | path | base | top; source: a device tensor or a callable
        that returns one per sample (a diagnostic field, evaluated once however many names read it); loc: s | u | v | w."""
        fo, sf = hp.forcing, hp.surface
        ut = float(self.utrans if self.utrans is not None else (fo.utrans if fo is not None else 0.))
        vt = float(self.vtrans if self.vtrans is not None else (fo.vtrans if fo is not None else 0.))
        out = {}
        # Fields: name -> (tensor, loc, offset, flux_bot, flux_top, bot, top)
        prog = {"u": (hp.u, "u", ut, hp.surf["u_fluxbot"], hp.surf["u_fluxtop"], getattr(sf, "ubot_t", None), getattr(sf, "utop_t", None)),
                "v": (hp.v, "v", vt, hp.surf["v_fluxbot"], hp.surf["v_fluxtop"], getattr(sf, "vbot_t", None), getattr(sf, "vtop_t", None)),
                "w": (hp.w, "w", 0., None, None, None, None)}
        micro = hp.cfg.get("micro") if hp.micro is not None else None
        ref_names = MOIST_NAMES.get(micro or "moist", ()) if hp.thermo is not None else (("b",) if hp.buoyant else ())
        for n, s in enumerate(hp.s):
            fb = sf.sfluxbot[n] if sf is not None else hp.surf["s_fluxbot"]
            row = (s, "s", 0., fb, hp.surf["s_fluxtop"], sf.sbot[n] if sf is not None else None, sf.stop[n] if sf is not None else None)
            for name in {"th" if n == 0 else "s%d" % n, "s%d" % n} | ({ref_names[n]} if n < len(ref_names) else set()):
                prog[name] = row
        # fluxbot and fluxtop get the offset the last plain section left behind (fields.cxx:1241-1245). cross_simple holds the listed
        # prognostic fields in the order of the map ap, by name, then the diagnostic ones of sd, whose offset is none (:482-497);
        # 0 where no plain section is listed, the reference's undefined case.
        last = 0.
        for name in sorted(n for n in self.crosslist if n in prog):
            last = prog[name][2]
        if any(n in ("p", "evisc") for n in self.crosslist):
            last = 0.
        second = hp.cfg["order"] == 2          # check_added_cross (:513-518): Fields gives no lngrad in second-order mode
        for name, (t, loc, off, fb, ft, bot, top) in prog.items():
            out[name] = ("simple", t, loc, off)
            if not second:
                out[name + "lngrad"] = ("lngrad", t, loc, 0.)
            out[name + "path"] = ("path", t, loc, 0.)
            for suffix, arr, o in (("fluxbot", fb, last), ("fluxtop", ft, last), ("bot", bot, off), ("top", top, off)):
                if arr is not None:
                    out[name + suffix] = ("plane", arr, loc, o)
        for name in ("p", "evisc"):                                      # the diagnostic fields of Fields (fields.cxx:493-497)
            out[name] = ("simple", getattr(hp, name), "s", 0.)
            if not second:
                out[name + "lngrad"] = ("lngrad", getattr(hp, name), "s", 0.)
        # Thermo
        if hp.thermo is not None:
            th = hp.thermo
            fld = {n: (lambda n=n: th.field(n)) for n in ("b", "ql", "qi")}
            fld["ql_qi"] = lambda: fld_now("ql") + fld_now("qi")      # get_thermo_field("ql_qi"): ql + qi

            def fld_now(n):
                return self._now(fld[n])
            out.update({"b": ("simple", fld["b"], "s", 0.), "blngrad": ("lngrad", fld["b"], "s", 0.),
                        "ql": ("simple", fld["ql"], "s", 0.), "qlpath": ("path", fld["ql"], "s", 0.),
                        "qlbase": ("base", fld["ql"], "s", 0.), "qltop": ("top", fld["ql"], "s", 0.),
                        "qi": ("simple", fld["qi"], "s", 0.), "qipath": ("path", fld["qi"], "s", 0.),
                        "qlqipath": ("path", fld["ql_qi"], "s", 0.), "qlqibase": ("base", fld["ql_qi"], "s", 0.),
                        "qlqitop": ("top", fld["ql_qi"], "s", 0.)})
        elif not hp.buoyant and hp.s:

            def dry_b():                  # Thermo_dry::get_thermo_field("b") (calc_buoyancy, src/thermo_dry.cxx:51-63)
                b = hp.torch.zeros(hp.grid.shape3, device=hp.device, dtype=hp.td)
                capi.check(hp.lib.mhh_thermo_dry_buoyancy(hp.G, b.data_ptr(), hp.s[0].data_ptr(), hp.thref.data_ptr(), 9.81, hp.stream), hp.lib)
                return b
            out.update({"b": ("simple", dry_b, "s", 0.), "blngrad": ("lngrad", dry_b, "s", 0.), "thlngrad": ("lngrad", hp.s[0], "s", 0.)})
        # Microphysics, surface layer, radiation
        if hp.micro is not None:
            bots = getattr(hp.micro, "bot", None) or [hp.micro.rr_bot]
            for name, t in zip(("rr_bot", "rs_bot", "rg_bot"), bots):
                out[name] = ("plane", t, "s", 0.)
        if sf is not None:
            out["ustar"], out["obuk"] = ("plane", sf.ustar, "s", 0.), ("plane", sf.obuk, "s", 0.)
        if hp.radiation is not None:
            rad = hp.radiation
            both = lambda: rad.fields()                              # noqa: E731   one call gives both
            out["lflx"] = ("simple", lambda: self._now(both)["lflx"], "s", 0.)
            out["sflx"] = ("simple", lambda: self._now(both)["sflx"], "s", 0.)
        # Immersed_boundary::exec_cross (src/immersed_boundary.cxx:950-985): <scalar>fluxbot_ib, a plane with no offset
        if getattr(hp, "ib", None) is not None:
            for name, row in list(prog.items()):
                if row[1] == "s":
                    n = next(m for m, t in enumerate(hp.s) if t is row[0])
                    out[name + "fluxbot_ib"] = ("plane", (lambda n=n: hp.ib.fluxbot(n)), "s", 0.)
        return out

    def _now(self, x):
        """A callable source is evaluated once per sample."""
        if not callable(x):
            return x
        if id(x) not in self._made:
            self._made[id(x)] = x()
        return self._made[id(x)]

    # -- bind ------------------------------------------------------------------------------------------------------
    def bind(self, hp):
        self.hp, self._made = hp, {}
        g, lib = hp.grid, hp.lib
        known = self._variables(hp)
        for name in self.crosslist:
            if name not in known:
                raise ValueError("field %s in [cross][crosslist] is illegal" % name)
        self.kxy, self.kxyh = indices(lib, g, XY, self.xy)
        self.jxz, self.jxzh = indices(lib, g, XZ, self.xz)
        self.ixz, self.ixzh = indices(lib, g, YZ, self.yz)
        self.entries = [(name,) + known[name] for name in self.crosslist]
        # the pieces: one plane of one variable each. (name, section, global index | None, op, source, job kind, local index, shape)
        self.pieces = []
        for name, op, src, loc, off in self.entries:
            if op in ("plane", "path", "base", "top"):
                self.pieces.append(dict(name=name, sect="xy", gidx=None, op=op, src=src, kind=PLANE, index=0, shape=(g.jmax, g.imax), offset=off))
                continue
            # cross_simple (src/cross.cxx:564-636): the half lists by the variable's location; cross_lngrad (:675-697): the full lists
            half = loc if op == "simple" else "s"
            for gj in (self.jxzh if half == "v" else self.jxz):
                # the row's owner; a half-level row jtot is the cyclic image of row 0, which the last rank holds as its north ghost row
                owner, lj = (hp.npy - 1, g.jend) if gj == g.jmax*hp.npy else (gj // g.jmax, gj % g.jmax + g.jgc)
                if owner == hp.rank:
                    self.pieces.append(dict(name=name, sect="xz", gidx=gj, op=op, src=src, kind=XZ, index=lj, shape=(g.kmax, g.imax), offset=off))
            for gi in (self.ixzh if half == "u" else self.ixz):
                self.pieces.append(dict(name=name, sect="yz", gidx=gi, op=op, src=src, kind=YZ, index=gi % g.imax + g.igc, shape=(g.kmax, g.jmax), offset=off))
            for gk in (self.kxyh if half == "w" else self.kxy):
                self.pieces.append(dict(name=name, sect="xy", gidx=gk, op=op, src=src, kind=XY, index=gk + g.kgc, shape=(g.jmax, g.imax), offset=off))
        pos = 0
        for p in self.pieces:
            p["pos"] = pos
            pos += p["shape"][0]*p["shape"][1]
        torch = hp.torch
        self.staging = torch.zeros(max(pos, 1), device=hp.device, dtype=hp.td)
        self.host = torch.zeros(max(pos, 1), dtype=hp.td, pin_memory=hp.on_gpu)
        self.order = hp.cfg["order"]
        return self

    # -- sample ----------------------------------------------------------------------------------------------------
    def filenames(self, iotime):
        """Every file a sample at iotime writes (the reference's names), in the order of the pieces; on a slab: this rank's share of
        the xz sections, and every xy, yz and plane file."""
        return [fieldio.cross_filename(self.path, p["name"], p["sect"], p["gidx"], iotime) for p in self.pieces]

    def enqueue(self):
        """The device part of a sample on hp.stream, without a synchronisation: the ghost cells, the kernels, the copy to the host."""
        hp, g, lib = self.hp, self.hp.grid, self.hp.lib
        self._made = {}
        es = self.staging.element_size()
        # the ghost cells a sample reads: lngrad's stencils, and the north ghost row of a half-level xz section at jtot. The same
        # list on every rank of a slab (the exchange is collective), whichever rank holds the row.
        need_halo, seen = [], set()
        jtot = g.jmax*hp.npy
        for name, op, src, loc, off in self.entries:
            if op == "lngrad" or (op == "simple" and jtot in (self.jxzh if loc == "v" else self.jxz)):
                t = self._now(src)
                if id(t) not in seen:
                    seen.add(id(t)); need_halo.append(t)
        if need_halo:
            hp.halo(need_halo)                # through the communicator, as Stats' fills
            # the cyclic fill has overwritten the lateral ghost cells of an open scalar (outflow.Outflow): the reference's sections
            # read them as set_prognostic_outflow_bcs left them (cross_lngrad, src/cross.cxx), so the outflow fill follows
            out = getattr(hp, "outflow", None)
            if out is not None and any(t is hp.s[n] for t in need_halo for n in out.index):
                hp.outflow_bcs()
        gather, lngrad = [], []
        for p in self.pieces:
            t, out = self._now(p["src"]), self.staging.data_ptr() + p["pos"]*es
            if p["op"] in ("simple", "plane"):
                gather.append(capi.MhhCrossJob(t.data_ptr(), p["kind"], p["index"], g.kstart, g.kend, float(p["offset"]), out))
            elif p["op"] == "lngrad":
                lngrad.append(capi.MhhCrossJob(t.data_ptr(), p["kind"], p["index"], g.kstart, g.kend, 0., out))
            elif p["op"] == "path":
                capi.check(lib.mhh_cross_path(hp.G, t.data_ptr(), hp.rhoref.data_ptr(), out, hp.stream), lib)
            else:
                capi.check(lib.mhh_cross_height_threshold(hp.G, t.data_ptr(), 0., 1 if p["op"] == "base" else 0, out, hp.stream), lib)
        if gather:
            capi.check(lib.mhh_cross_gather(hp.G, (capi.MhhCrossJob*len(gather))(*gather), len(gather), hp.stream), lib)
        if lngrad:
            capi.check(lib.mhh_cross_lngrad(hp.G, self.order, (capi.MhhCrossJob*len(lngrad))(*lngrad), len(lngrad), hp.stream), lib)
        self.host.copy_(self.staging, non_blocking=True)
        self._made = {}

    def sample(self, iotime):
        """One sample: the files name.xy.KKKKK.NNNNNNN, name.xz.JJJJJ.NNNNNNN, name.yz.IIIII.NNNNNNN and name.xy.NNNNNNN of every
        listed variable under `path`. An existing file is an error (the reference opens with "wbx"). Returns the files written by
        this rank (on a slab: the shared ones are named by every rank)."""
        hp, g = self.hp, self.hp.grid
        names = self.filenames(iotime)
        there = [fn for fn in names if os.path.exists(fn)]
        # every rank has looked before any file is made, and all of them refuse together (the reduction is the meeting point)
        if hp.master.max(float(len(there))) > 0:
            raise FileExistsError("%s exists: a cross-section file is created exclusively (\"wbx\", src/field3d_io.cxx:780)"
                                  % (there[0] if there else "a file of this sample on another rank"))
        self.enqueue()
        hp.sync()
        host = self.host.numpy()
        size = g.np_dtype.itemsize
        if hp.npy > 1:
            if hp.rank == 0:
                for p, fn in zip(self.pieces, names):
                    if p["sect"] != "xz":
                        rows, cols = p["shape"]
                        fieldio.prepare_slice_file(fn, rows*cols*hp.npy*size)      # (jtot, itot) or (kmax, jtot)
            hp.master.barrier()
        for p, fn in zip(self.pieces, names):
            plane = host[p["pos"]:p["pos"] + p["shape"][0]*p["shape"][1]].reshape(p["shape"])
            if p["sect"] == "xz":
                fieldio.save_xz_slice(fn, plane, g)
            elif p["sect"] == "yz":
                fieldio.save_yz_slice(fn, plane, g, rank=hp.rank, npy=hp.npy)
            else:
                fieldio.save_xy_slice(fn, plane, g, rank=hp.rank, npy=hp.npy)
        hp.master.barrier()
        return names
