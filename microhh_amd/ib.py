"""Immersed_boundary on the host side: the driver of csrc/immersed_boundary.h behind HotPath(..., ib=Dem(...)).

Flow over terrain (sw_immersed_boundary=dem, src/immersed_boundary.cxx). Binding restates Immersed_boundary::create (:766-918): the
DEM halos, calc_ghost_cells for u (xh, y, z), v (x, yh, z), w (x, y, zh with dzh) and, where the case has scalars, s; the boundary
values; find_k_dem. All of that runs on the host inside the library (mhh_ib_ghost_cells_host, _k_dem_host, _interp_dem_host). The
lists then become the device tables of mhh_ib_job -- one 32-bit cell offset per (i, j, k), the per-point arrays transposed -- and
the mask fields of the `ib` statistics mask are written once, since the DEM does not change.

A sub-step calls exec_scalars() in front of the RHS and exec_momentum() in front of the pressure solve (src/model.cxx:380, :407):
one launch each, followed by the cyclic fills of the fields it wrote. IB_type::User, the fourth order and the prognostic outflow
boundary of :383 are not built.
"""
import ctypes as C
import os

import numpy as np

from . import capi, fieldio

DIRICHLET, NEUMANN, FLUX = 0, 1, 2
BC = {"dirichlet": DIRICHLET, "neumann": NEUMANN, "flux": FLUX}
INT_LISTS = ("i", "j", "k", "ip_i", "ip_j", "ip_k")
PER_GHOST = ("xb", "yb", "zb", "xi", "yi", "zi", "di", "c_idw_sum")
PER_POINT = ("ip_d", "c_idw")


def sine_dem(itot, jtot, xsize, ysize, zsize, amplitude=0.15):
    """The terrain of the tests and the cost script, in the grid's own coordinates: zsize*(0.25 + A sin(2 pi x/xsize) cos(2 pi y/ysize))."""
    x = (np.arange(itot) + 0.5)*xsize/itot
    y = (np.arange(jtot) + 0.5)*ysize/jtot
    return zsize*(0.25 + amplitude*np.sin(2.*np.pi*x[None, :]/xsize)*np.cos(2.*np.pi*y[:, None]/ysize))


def locations(grid):
    """gd.x, gd.xh, gd.y, gd.yh (src/grid.cxx:248-262): (i-igc)*dx is a product in TF, the sums with 0.5*dx and the rank's offset are
    in double, narrowed last."""
    g, t = grid, grid.np_dtype
    yoff = g.mpicoordy*g.ysize/g.npy
    px = ((np.arange(g.icells) - g.igc).astype(t)*t.type(g.dx)).astype(np.float64)
    py = ((np.arange(g.jcells) - g.jgc).astype(t)*t.type(g.dy)).astype(np.float64)
    return {"x": (0.5*g.dx + px + 0.).astype(t), "xh": (px + 0.).astype(t),
            "y": (0.5*g.dy + py + yoff).astype(t), "yh": (py + yoff).astype(t)}


def mpi_offsets(grid):
    """mpi_offset_x, mpi_offset_y of Immersed_boundary::create (:781-782)."""
    return -grid.mpicoordx*grid.imax + grid.igc, -grid.mpicoordy*grid.jmax + grid.jgc


def ghost_cells(lib, grid, dem, x, y, z, dz, n_idw, bc, offsets=None):
    """calc_ghost_cells (src/immersed_boundary.cxx:334-426) for one location: {name: array} as Ghost_cells<TF> holds them, with
    "nghost". dem is the rank's plane [jcells][icells] with filled halos."""
    g, t = grid, grid.np_dtype
    ox, oy = mpi_offsets(g) if offsets is None else offsets
    arrs = [np.ascontiguousarray(a, dtype=t) for a in (dem, x, y, z, dz)]
    ptrs = [a.ctypes.data for a in arrs]
    n = C.c_int(0)
    capi.check(lib.mhh_ib_ghost_cells_host(g.host_struct(), *ptrs, n_idw, bc, ox, oy, C.byref(n), None), lib)
    ng = n.value
    out = {k: np.zeros(ng, dtype=np.int32) for k in ("i", "j", "k")}
    out.update({k: np.zeros((ng, n_idw), dtype=np.int32) for k in ("ip_i", "ip_j", "ip_k")})
    out.update({k: np.zeros(ng, dtype=t) for k in PER_GHOST})
    out.update({k: np.zeros((ng, n_idw), dtype=t) for k in PER_POINT})
    lists = capi.MhhIbGhostLists()
    for k, a in out.items():
        setattr(lists, k, a.ctypes.data_as(capi.IP) if k in INT_LISTS else a.ctypes.data)
    capi.check(lib.mhh_ib_ghost_cells_host(g.host_struct(), *ptrs, n_idw, bc, ox, oy, C.byref(n), C.byref(lists)), lib)
    out["nghost"] = ng
    return out


def k_dem(lib, grid, dem):
    """find_k_dem (src/immersed_boundary.cxx:516-537): unsigned int [jcells][icells], interior columns."""
    g = grid
    out = np.zeros(g.shape2, dtype=np.uint32)
    dem = np.ascontiguousarray(dem, dtype=g.np_dtype)
    capi.check(lib.mhh_ib_k_dem_host(g.host_struct(), dem.ctypes.data, g.z.ctypes.data, out.ctypes.data), lib)
    return out


def interp_dem(lib, grid, plane, xp, yp, offsets=None, x=None, y=None):
    """interp2_dem (src/immersed_boundary.cxx:65-103) of plane [jcells][icells] at the points (xp, yp). x, y: the coordinate arrays
    the factors are formed with (the reference passes the location's own, xh for u and yh for v); None: gd.x, gd.y."""
    g, t = grid, grid.np_dtype
    ox, oy = mpi_offsets(g) if offsets is None else offsets
    loc = locations(g)
    x, y = (np.ascontiguousarray(loc[n] if a is None else a, dtype=t) for n, a in (("x", x), ("y", y)))
    plane, xp, yp = (np.ascontiguousarray(a, dtype=t) for a in (plane, xp, yp))
    out = np.zeros(xp.size, dtype=t)
    capi.check(lib.mhh_ib_interp_dem_host(g.host_struct(), plane.ctypes.data, x.ctypes.data, y.ctypes.data,
                                          xp.ctypes.data, yp.ctypes.data, xp.size, ox, oy, out.ctypes.data), lib)
    return out


def device_tables(grid, gh):
    """The tables of mhh_ib_job from one location's lists: cell [nghost], ip and c_idw [n_idw][nghost] (transposed), as host arrays.
    Every offset is checked to lie inside a field: the kernel indexes with them."""
    g = grid
    cell = (gh["i"].astype(np.int64) + gh["j"].astype(np.int64)*g.icells + gh["k"].astype(np.int64)*g.ijcells)
    ip = (gh["ip_i"].astype(np.int64) + gh["ip_j"].astype(np.int64)*g.icells + gh["ip_k"].astype(np.int64)*g.ijcells)
    for a in (cell, ip):
        if a.size and (a.min() < 0 or a.max() >= g.ncells):
            raise ValueError("immersed boundary: a cell offset outside the field")
    return {"cell": np.ascontiguousarray(cell, dtype=np.int32), "ip": np.ascontiguousarray(ip.T, dtype=np.int32),
            "c_idw": np.ascontiguousarray(gh["c_idw"].T), "c_idw_sum": np.ascontiguousarray(gh["c_idw_sum"]), "di": np.ascontiguousarray(gh["di"])}


def job(fld, bv, bc, visc, nghost, tab):
    """An mhh_ib_job from addresses: tab holds the device tables' addresses by name."""
    return capi.MhhIbJob(fld, bv, bc, nghost, float(visc), tab["cell"], tab["ip"], tab["c_idw"], tab["c_idw_sum"], tab["di"])


class Dem:
    """Dem(dem, n_idw_points, sbcbot="dirichlet", sbot=(...), sbot_spatial={n: plane}): HotPath(..., ib=Dem(...)).

    dem: the interior DEM plane (jtot, itot) of the whole domain, a host array; sbot: one boundary value per scalar (absent: 0);
    sbot_spatial: per scalar number, a (jtot, itot) plane that is interpolated to the wall points (xb, yb) instead."""

    def __init__(self, dem, n_idw_points, sbcbot="dirichlet", sbot=(), sbot_spatial=None):
        if sbcbot not in BC:
            raise ValueError("IB sbcbot=%s is not a valid choice (options: dirichlet, neumann, flux)" % sbcbot)      # :726
        self.dem_in, self.n_idw, self.sbcbot = dem, int(n_idw_points), BC[sbcbot]
        self.sbot_in, self.spatial_in = tuple(sbot), dict(sbot_spatial or {})

    @classmethod
    def from_file(cls, path, n_idw_points, sbcbot="dirichlet", sbot=(), sbot_spatial=()):
        """dem.0000000 and <scalar>_sbot.0000000 under `path` (:785, :878), read at bind with the grid's size and dtype through
        fieldio.load_xy_slice; sbot_spatial: {scalar number: the scalar's name in the file name}, or numbers (s<n>, th for 0)."""
        names = dict(sbot_spatial) if isinstance(sbot_spatial, dict) else {n: ("th" if n == 0 else "s%d" % n) for n in sbot_spatial}
        self = cls(os.path.join(path, "dem.0000000"), n_idw_points, sbcbot, sbot, {n: os.path.join(path, "%s_sbot.0000000" % name) for n, name in names.items()})
        return self

    # -- bind ------------------------------------------------------------------------------------------------------
    def _plane(self, hp, a):
        """A global interior plane (or the file that holds it) -> this rank's [jcells][icells] device tensor with filled halos."""
        g, torch = hp.grid, hp.torch
        if isinstance(a, str):
            a = fieldio.load_xy_slice(a, g, npy=hp.npy)
        a = np.asarray(a)
        if a.shape != (g.jmax*hp.npy, g.itot):
            raise ValueError("immersed boundary: a plane of shape %s, the domain has (jtot, itot) = (%d, %d)" % (a.shape, g.jmax*hp.npy, g.itot))
        t = torch.zeros(g.shape2, dtype=hp.td)
        t[g.jstart:g.jend, g.istart:g.iend] = torch.from_numpy(np.ascontiguousarray(a[hp.rank*g.jmax:(hp.rank+1)*g.jmax], dtype=g.np_dtype))
        t = t.to(hp.device).contiguous()
        hp._halo2d(t)                   # boundary_cyclic.exec_2d (:800): local wrap on one rank, the communicator's ring on a slab
        return t

    def _halo2d_u32(self, t):
        hp, g = self.hp, self.hp.grid
        if hp.master.mode == "local":
            capi.check(hp.lib.mhh_boundary_cyclic_2d_u32(hp.G, t.data_ptr(), hp.stream), hp.lib)
            return
        torch = hp.torch
        t[:, :g.igc] = t[:, g.iend-g.igc:g.iend].clone(); t[:, g.iend:] = t[:, g.istart:g.istart+g.igc].clone()
        send = torch.cat([t[g.jend-g.jgc:g.jend], t[g.jstart:g.jstart+g.jgc]]).reshape(-1)
        recv = torch.empty_like(send)
        hp.master.ring(send, recv, send.numel() // 2, send.numel() // 2)
        t[:g.jgc], t[g.jend:] = recv.view(2, g.jgc, -1)

    def bind(self, hp):
        self.hp = hp
        g, lib, torch = hp.grid, hp.lib, hp.torch
        if hp.cfg["order"] != 2:
            raise ValueError("immersed boundary: a fourth-order case (%s) is not built" % hp.case)
        if g.igc < 2 or g.jgc < 2:
            raise ValueError("immersed boundary: case %s has ghost cells (%d, %d, %d); at least two horizontal ghost cells are needed "
                             "(src/immersed_boundary.cxx:622)" % (hp.case, g.igc, g.jgc, g.kgc))
        self.dem = self._plane(hp, self.dem_in)
        hp.sync()
        self.dem_h = dem = self.dem.detach().cpu().numpy().copy()
        loc = locations(g)
        n = self.n_idw
        self.ghost = {"u": ghost_cells(lib, g, dem, loc["xh"], loc["y"], g.z, g.dz, n, DIRICHLET),
                      "v": ghost_cells(lib, g, dem, loc["x"], loc["yh"], g.z, g.dz, n, DIRICHLET),
                      "w": ghost_cells(lib, g, dem, loc["x"], loc["y"], g.zh, g.dzh, n, DIRICHLET)}
        if hp.s:
            self.ghost["s"] = ghost_cells(lib, g, dem, loc["x"], loc["y"], g.z, g.dz, n, self.sbcbot)
        # the boundary values: mbot = 0 (:845-851); sbot per scalar, constant or interpolated to (xb, yb) (:869-904)
        for name in ("u", "v", "w"):
            self.ghost[name]["mbot"] = np.zeros(self.ghost[name]["nghost"], dtype=g.np_dtype)
        if hp.s:
            gs = self.ghost["s"]
            gs["sbot"] = []
            for m in range(len(hp.s)):
                if m in self.spatial_in:
                    plane = self._plane(hp, self.spatial_in[m])
                    hp.sync()
                    gs["sbot"].append(interp_dem(lib, g, plane.detach().cpu().numpy(), gs["xb"], gs["yb"]))
                else:
                    gs["sbot"].append(np.full(gs["nghost"], self.sbot_in[m] if m < len(self.sbot_in) else 0., dtype=g.np_dtype))

        def dev(a):
            # (an empty tensor has a null address: one element stands in, and the job's nghost = 0 keeps it unread)
            return torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(1, dtype=a.dtype)).to(hp.device)
        self.tables, self._keep = {}, []
        for name, gh in self.ghost.items():
            self.tables[name] = {k: dev(a) for k, a in device_tables(g, gh).items()}
        addr = {name: {k: t.data_ptr() for k, t in tab.items()} for name, tab in self.tables.items()}
        jobs = []
        for name, fld in (("u", hp.u), ("v", hp.v), ("w", hp.w)):
            bv = dev(self.ghost[name]["mbot"]); self._keep.append(bv)
            jobs.append(job(fld.data_ptr(), bv.data_ptr(), DIRICHLET, hp.cfg["visc"], self.ghost[name]["nghost"], addr[name]))
        self.jobs_m = (capi.MhhIbJob*3)(*jobs)
        jobs = []
        for m, s in enumerate(hp.s):
            bv = dev(self.ghost["s"]["sbot"][m]); self._keep.append(bv)
            jobs.append(job(s.data_ptr(), bv.data_ptr(), self.sbcbot, hp.fields.svisc[m], self.ghost["s"]["nghost"], addr["s"]))
        self.jobs_s = (capi.MhhIbJob*max(len(jobs), 1))(*jobs)
        # calc_mask (:489-512), once: the DEM does not change
        self.mask = torch.zeros(g.shape3, device=hp.device, dtype=hp.td)
        self.maskh = torch.zeros(g.shape3, device=hp.device, dtype=hp.td)
        capi.check(lib.mhh_ib_mask(hp.G, self.dem.data_ptr(), self.mask.data_ptr(), self.maskh.data_ptr(), hp.stream), lib)
        # find_k_dem and its cyclic fill (:909-916)
        self.k_dem = torch.from_numpy(k_dem(lib, g, dem).view(np.int32)).to(hp.device).contiguous()
        self._halo2d_u32(self.k_dem)
        return self

    # -- the two calls of a sub-step ----------------------------------------------------------------------------------
    def set_momentum(self):
        hp = self.hp
        capi.check(hp.lib.mhh_ib_set_ghost_cells(hp.G, self.n_idw, self.jobs_m, 3, hp.stream), hp.lib)

    def set_scalars(self):
        hp = self.hp
        if hp.s:
            capi.check(hp.lib.mhh_ib_set_ghost_cells(hp.G, self.n_idw, self.jobs_s, len(hp.s), hp.stream), hp.lib)

    def exec_momentum(self):
        """Immersed_boundary::exec_momentum (:640-674, .cu:108-137): the ghost cells of u, v, w in one launch, then their cyclic fills."""
        self.set_momentum()
        self.hp.halo([self.hp.u, self.hp.v, self.hp.w])

    def exec_scalars(self):
        """Immersed_boundary::exec_scalars (:677-696, .cu:140-168): every scalar in one launch, then their cyclic fills."""
        if self.hp.s:
            self.set_scalars()
            self.hp.halo(list(self.hp.s))

    def fluxbot(self, n):
        """calc_fluxes (:541-597) of scalar n: a new [jcells][icells] device tensor, interior columns."""
        hp = self.hp
        out = hp.torch.zeros(hp.grid.shape2, device=hp.device, dtype=hp.td)
        capi.check(hp.lib.mhh_ib_fluxbot(hp.G, out.data_ptr(), self.k_dem.data_ptr(), hp.s[n].data_ptr(), hp.fields.svisc[n], hp.stream), hp.lib)
        return out
