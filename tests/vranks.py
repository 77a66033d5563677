"""N slab ranks in ONE process: the C ABI of the slab path (k_slab.hip, the lds_slab_* launchers of k_pres.hip) driven for every
rank in turn, the exchanges done here on the backend's own arrays.

``VRanks`` holds, per rank, a rank grid (``npy=``, ``mpicoordy=``), one ``backends.DevCase`` whose fields are the rank's rows of ONE
global ``common.Case``, a slab pressure plan and a pair of all-to-all buffers. No process is spawned, there is no torch.distributed
and no stream beside the backend's: what this harness checks is the arithmetic and the buffer layouts, on either backend of
tests/backends.py; the real exchanges and their stream ordering stay with the multi-process tests (tests/ranks.py).

* ``ring(fields, rs, rn)``   mhh_boundary_cyclic_n(EDGE_EW) + mhh_halo_pack_rows on every rank, the swap with the two neighbours
                             in Master.ring's buffer layout [northbound | southbound], mhh_halo_unpack_rows.
* ``all_to_all(c)``          recv_r[q-block] = send_q[r-block] inside k-slice c of the two buffers.
* ``pres(form, slim)``       the call order of HotPath.pres (microhh_amd/model.py), every stage on every rank before the next.
* ``gather(name)``           the global interior [ktot][jtot][itot].

Buffers are sized by mhh_halo_buffer_elems and mhh_pres_slab_xbuf_elems only (plus a tail the tests watch).

The module also holds the reference side: the oracle's Pres::exec on a Case, the fp64 twin of an fp32 Case, and the tolerance
rule of DESIGN.md §3 (``e_ref`` / ``bound``).
"""
import ctypes as C
import types

import numpy as np

import backends as B
import common as cm
from common import ptr, dbl
from microhh_amd import capi
from microhh_amd.grid import Grid, METRICS

TAIL = 64                      # elements past the size the library states, which no call may touch
FILL = -123.25                 # what buffers hold before the library writes them
NAMES = ("p", "ut", "vt", "wt")


def make_grid(shape, dtype, order=2, stretched=False, gc=None, npy=1, rank=0):
    itot, jtot, ktot = shape
    if order == 4:
        kw = {} if gc is None else dict(igc=gc[0], jgc=gc[1], kgc=gc[2])
        return cm.grid_4th(itot, jtot, ktot, dtype=dtype, npy=npy, mpicoordy=rank, **kw)       # always moser_z
    return cm.grid_2nd(itot, jtot, ktot, gc=gc or (3, 3, 1), dtype=dtype, stretched=stretched, npy=npy, mpicoordy=rank)


def rows_of(gg, g, a):
    """A copy of the rows of rank grid g (ghost rows included) of an array on the global grid gg."""
    j0 = g.mpicoordy * g.jmax
    return a[:, j0:j0 + g.jcells, :].copy()


class VRanks:
    def __init__(self, be, case, npy, order=2, chunks=1, tail=0, plans=True):
        """case: a common.Case on the GLOBAL grid (npy = 1), u, v, w with their cyclic ghost cells (periodic=True).
        plans=False: grids and fields only (the halo tests)."""
        self.be, self.lib, self.case, self.npy, self.order = be, be.lib, case, npy, order
        gg = self.gg = case.grid
        dtype = gg.np_dtype
        self.grids, self.dev, self.F, self.plans, self.xsend, self.xrecv = [], [], [], [], [], []
        self._halo = {}
        for r in range(npy):
            g = Grid(gg.itot, gg.jtot, gg.ktot, gg.xsize, gg.ysize, gg.zsize, order=gg.order, igc=gg.igc, jgc=gg.jgc, kgc=gg.kgc,
                     z=gg.z[gg.kstart:gg.kend].astype(np.float64), dtype=dtype, npy=npy, mpicoordy=r)
            for n in METRICS:                                  # the global grid's metrics to the bit
                setattr(g, n, getattr(gg, n).copy())
            assert (g.dx, g.dy) == (gg.dx, gg.dy)
            rc = cm.Case(g, nscalars=0)
            for n in ("u", "v", "w", "ut", "vt", "wt", "p"):
                setattr(rc, n, rows_of(gg, g, getattr(case, n)))
            rc.rhoref, rc.rhorefh = case.rhoref.copy(), case.rhorefh.copy()
            d = B.DevCase(be, rc)
            self.grids.append(g); self.dev.append(d); self.F.append(d.fields())
        self.chunks, self.tail = chunks, tail
        self.nxh = gg.itot//2 + 1
        self.nxb = (self.nxh + npy - 1)//npy
        if not plans:
            return
        try:
            for r, g in enumerate(self.grids):
                plan = capi.PLAN()
                B.ok(be, self.lib.mhh_pres_slab_plan_create_order(g.host_struct(), order, ptr(g.dz), ptr(g.dzhi), ptr(g.dzi4), ptr(g.dzhi4),
                                                                  ptr(case.rhoref), ptr(case.rhorefh), C.byref(plan)))
                self.plans.append(plan)
                B.ok(be, self.lib.mhh_pres_slab_set_chunks(plan, chunks))
                assert self.lib.mhh_pres_slab_chunks(plan) == chunks and self.lib.mhh_pres_slab_order(plan) == order
                self.xelems = int(self.lib.mhh_pres_slab_xbuf_elems(plan))          # complex elements
                for bufs in (self.xsend, self.xrecv):
                    bufs.append(be.arr(np.full(2*self.xelems + tail, FILL, dtype)))
        except Exception:
            self.close()
            raise
        assert self.xelems == npy * gg.ktot * self.grids[0].jmax * self.nxb

    def close(self):
        for p in self.plans:
            self.lib.mhh_pres_slab_plan_destroy(p)
        self.plans = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.be.sync()
        self.close()

    # -- fields -------------------------------------------------------------------------------------------------------
    def f(self, name):
        """[the array of rank 0, of rank 1, ...] of a DevCase field."""
        return [getattr(d, name) for d in self.dev]

    def gather(self, name):
        parts = [self.be.host(a)[g.interior] for a, g in zip(self.f(name), self.grids)]
        return np.concatenate(parts, axis=1)

    def has_lds(self):
        v = {self.lib.mhh_pres_slab_has_lds(p) for p in self.plans}
        assert len(v) == 1, v
        return v.pop() == 1

    def _ptrs(self, arrays):
        return (C.c_void_p * len(arrays))(*[self.be.ptr(a).value for a in arrays])

    # -- north-south halos --------------------------------------------------------------------------------------------
    def halo_buffers(self, nf):
        """(send, recv) of every rank for nf fields: 2 x mhh_halo_buffer_elems elements ([northbound | southbound]) + TAIL."""
        if nf not in self._halo:
            g = self.grids[0]
            n = int(self.lib.mhh_halo_buffer_elems(g.host_struct(), nf))
            assert n == nf * g.kcells * g.jgc * g.icells
            self._halo[nf] = [[self.be.arr(np.full(2*n + TAIL, FILL, g.np_dtype)) for _ in range(self.npy)] for _ in range(2)]
        return self._halo[nf]

    def ring(self, fields, rs=None, rn=None, ns_calls=False):
        """fields[n][r]: field n of rank r. rs rows travel south, rn north (default: jgc each). ns_calls: through
        mhh_halo_pack_ns / mhh_halo_unpack_ns (the full exchange only)."""
        be, lib, g = self.be, self.lib, self.grids[0]
        nf, npy = len(fields), self.npy
        full = rs is None and rn is None
        rs = g.jgc if rs is None else rs
        rn = g.jgc if rn is None else rn
        assert 0 <= rs <= g.jgc and 0 <= rn <= g.jgc and rs + rn > 0 and (full or not ns_calls)
        per = nf * g.kcells * g.icells
        nn, ns = rn * per, rs * per
        send, recv = self.halo_buffers(nf)
        esz = g.np_dtype.itemsize
        for r in range(npy):
            arr = self._ptrs([f[r] for f in fields])
            B.ok(be, lib.mhh_boundary_cyclic_n(self.dev[r].G, arr, nf, cm.EDGE_EW, be.stream))
            s0 = be.ptr(send[r]).value
            if ns_calls:
                B.ok(be, lib.mhh_halo_pack_ns(self.dev[r].G, arr, nf, s0 + nn*esz, s0, be.stream))
            else:
                B.ok(be, lib.mhh_halo_pack_rows(self.dev[r].G, arr, nf, rs, rn, s0 + nn*esz, s0, be.stream))
        for r in range(npy):                       # Master.ring: my northbound part is the first part of my north neighbour
            south, north = (r - 1) % npy, (r + 1) % npy
            recv[r][:nn] = send[south][:nn]
            recv[r][nn:nn+ns] = send[north][nn:nn+ns]
        for r in range(npy):
            arr = self._ptrs([f[r] for f in fields])
            r0 = be.ptr(recv[r]).value
            if ns_calls:
                B.ok(be, lib.mhh_halo_unpack_ns(self.dev[r].G, arr, nf, r0, r0 + nn*esz, be.stream))
            else:
                B.ok(be, lib.mhh_halo_unpack_rows(self.dev[r].G, arr, nf, rs, rn, r0, r0 + nn*esz, be.stream))
        return nn, ns

    # -- the x <-> y transposes ---------------------------------------------------------------------------------------
    def all_to_all(self, c):
        """Transpose::exec_xy / exec_yx of k-slice c: one equal-split all-to-all of elements [c*seg, (c+1)*seg)."""
        seg = 2*self.xelems // self.chunks             # real numbers
        blk = seg // self.npy
        assert seg * self.chunks == 2*self.xelems and blk * self.npy == seg
        for r in range(self.npy):
            for q in range(self.npy):
                self.xrecv[r][c*seg + q*blk: c*seg + (q+1)*blk] = self.xsend[q][c*seg + r*blk: c*seg + (r+1)*blk]

    def xbuf_host(self, bufs, r):
        """An all-to-all buffer of rank r as complex numbers [slice][peer][k in slice][a][b] -- (a, b) = (jl, kxl) in the staged
        form, (kxl, jl) with the transforms in LDS -- and its tail."""
        h = self.be.host(bufs[r])
        body, tail = h[:2*self.xelems], h[2*self.xelems:]
        z = body[0::2] + 1j*body[1::2]
        return z, tail

    # -- Pres::exec ---------------------------------------------------------------------------------------------------
    def pres(self, dt, form="staged", slim=False, after_x_in=None, before_x_out=None):
        """HotPath.pres for every rank. form "staged": rocFFT transforms, pack and unpack kernels; "lds": the x and y transforms in
        LDS (pres_2, slim halos). slim: the one-row halos of vt and p. The two hooks run with every rank's send buffer written by
        the forward x stage, and just before the inverse x stage reads the receive buffers."""
        lib, be, n, order, R = self.lib, self.be, self.chunks, self.order, range(self.npy)
        P, G, F = self.plans, [d.G for d in self.dev], [C.byref(f) for f in self.F]
        lds_x = form == "lds"
        assert form in ("staged", "lds") and (not lds_x or (order == 2 and slim)) and (order == 2 or not slim)
        if slim or order == 4: self.ring([self.f("vt")], *((2, 1) if order == 4 else (1, 0)))
        else:                  self.ring([self.f("vt")])
        xs, xr = [be.ptr(a) for a in self.xsend], [be.ptr(a) for a in self.xrecv]
        st = be.stream
        if lds_x:
            assert self.has_lds()
            x_in = lambda r, c: lib.mhh_pres_slab_lds_fwd(P[r], G[r], F[r], dt, xs[r], c, st)            # noqa: E731
            y_in = lambda r, c: lib.mhh_pres_slab_lds_fwd_y(P[r], G[r], xr[r], c, st)                    # noqa: E731
            y_out = lambda r, c: lib.mhh_pres_slab_lds_bwd_y(P[r], G[r], xs[r], c, st)                   # noqa: E731
            x_out = lambda r, c: lib.mhh_pres_slab_lds_bwd(P[r], G[r], xr[r], F[r], c, st)               # noqa: E731
        else:
            packed = [lib.mhh_pres_slab_packed(p) for p in P]
            for r in R:
                B.ok(be, lib.mhh_pres_input_packed(G[r], order, F[r], dt, packed[r], st))
            x_in = lambda r, c: lib.mhh_pres_fwd_x_pack_chunk(P[r], G[r], packed[r], xs[r], c, st)       # noqa: E731
            y_in = lambda r, c: lib.mhh_pres_fwd_y_chunk(P[r], G[r], xr[r], c, st)                       # noqa: E731
            y_out = lambda r, c: lib.mhh_pres_bwd_y_chunk(P[r], G[r], xs[r], c, st)                      # noqa: E731
            x_out = lambda r, c: lib.mhh_pres_bwd_x_chunk(P[r], G[r], xr[r], c, st)                      # noqa: E731
        for c in range(n):
            for r in R:
                B.ok(be, x_in(r, c))
        if after_x_in:
            after_x_in(self)
        for c in range(n):
            self.all_to_all(c)
        for c in range(n):
            for r in R:
                B.ok(be, y_in(r, c))
        for r in R:
            B.ok(be, lib.mhh_pres_solve_y(P[r], G[r], st))
        for c in range(n):
            for r in R:
                B.ok(be, y_out(r, c))
            self.all_to_all(c)
        if before_x_out:
            before_x_out(self)
        for c in range(n):
            for r in R:
                B.ok(be, x_out(r, c))
        if order == 2 and slim:
            if not lds_x:
                for r in R:
                    B.ok(be, lib.mhh_pres_unpack_output_slab(P[r], G[r], F[r], st))
            self.ring([self.f("p")], 0, 1)
            for r in R:
                B.ok(be, lib.mhh_pres_output_south_row(G[r], F[r], st))
        else:
            for r in R:
                B.ok(be, lib.mhh_pres_unpack_slab(P[r], G[r], F[r], st))
            if order == 4: self.ring([self.f("p")], 1, 2)
            else:          self.ring([self.f("p")])
            for r in R:
                B.ok(be, lib.mhh_pres_output_order(G[r], order, F[r], st))
        be.sync()


# ---- the reference side -----------------------------------------------------------------------------------------------------
def global_case(shape, dtype, order=2, stretched=False, rho="one", gc=None, seed=666):
    g = make_grid(shape, dtype, order, stretched, gc)
    return cm.Case(g, seed=seed, nscalars=0, rho=rho, periodic=True)


def twin64(case):
    """The fp64 twin of a Case: the same numbers (metrics, dx, dy, rhoref, fields) widened, so that the oracle evaluates the
    SAME operator on the SAME inputs in double precision."""
    g = case.grid
    G = Grid(g.itot, g.jtot, g.ktot, g.xsize, g.ysize, g.zsize, order=g.order, igc=g.igc, jgc=g.jgc, kgc=g.kgc,
             z=g.z[g.kstart:g.kend].astype(np.float64), dtype=np.float64)
    for n in METRICS:
        setattr(G, n, getattr(g, n).astype(np.float64))
    G.dx, G.dy = g.dx, g.dy
    t = types.SimpleNamespace(grid=G)
    for n in ("u", "v", "w", "ut", "vt", "wt", "p", "rhoref", "rhorefh"):
        setattr(t, n, getattr(case, n).astype(np.float64))
    return t


def oracle_input(case, order, dt):
    """orc_pres_input: the packed right-hand side [ktot][jtot][itot] (the tendencies' ghost cells are filled on copies)."""
    g = case.grid
    pk = np.zeros((g.ktot, g.jtot, g.itot), g.np_dtype)
    t = [case.ut.copy(), case.vt.copy(), case.wt.copy()]
    cm.oracle().orc_pres_input(g.host_struct(), order, ptr(pk), ptr(case.u), ptr(case.v), ptr(case.w), *[ptr(x) for x in t],
                               ptr(case.rhoref), ptr(case.rhorefh), dbl(dt))
    return pk


def oracle_exec(case, order, dt):
    """orc_pres_exec on copies: {p, ut, vt, wt} on the global interior."""
    g = case.grid
    p = np.zeros(g.shape3, g.np_dtype); pk = np.zeros((g.ktot, g.jtot, g.itot), g.np_dtype)
    t = [case.ut.copy(), case.vt.copy(), case.wt.copy()]
    cm.oracle().orc_pres_exec(g.host_struct(), order, ptr(p), ptr(pk), ptr(case.u), ptr(case.v), ptr(case.w), *[ptr(x) for x in t],
                              ptr(case.rhoref), ptr(case.rhorefh), dbl(dt))
    return {n: a[g.interior].copy() for n, a in zip(NAMES, [p] + t)}


def errors(got, want, g):
    """max |got - want| per field on the scales of tests/test_pres_ref.py::test_library_slab_pressure: p by max |p|, a tendency by
    the larger of its own maximum and max |p| / min(dx, dy)."""
    pscale = float(np.abs(want["p"]).max())
    out = {}
    for n in NAMES:
        scale = pscale if n == "p" else max(float(np.abs(want[n]).max()), pscale/float(min(g.dx, g.dy)))
        out[n] = float(np.abs(got[n].astype(np.float64) - want[n].astype(np.float64)).max()) / scale
    return out


CEILING = {np.dtype(np.float64): 1e-11, np.dtype(np.float32): 2e-4}      # the project's pressure tolerance: never looser than this
FACTOR32, FACTOR64 = 4., 8.


class Reference:
    """Truth and yardstick of one (shape, order, grid kind): the fp32 Case, its fp64 twin, the oracle on both.
    e_ref[field] = error of the fp32 oracle against the fp64 oracle on the same inputs."""

    def __init__(self, shape, order, stretched, rho, dt, gc=None):
        self.c32 = global_case(shape, np.float32, order, stretched, rho, gc)
        self.c64 = global_case(shape, np.float64, order, stretched, rho, gc)
        self.truth32 = oracle_exec(twin64(self.c32), order, dt)
        self.want64 = oracle_exec(self.c64, order, dt)
        self.e_ref = errors(oracle_exec(self.c32, order, dt), self.truth32, self.c32.grid)

    def case(self, dtype):
        return self.c32 if np.dtype(dtype) == np.float32 else self.c64

    def want(self, dtype):
        """What a library result of this dtype is compared with."""
        return self.truth32 if np.dtype(dtype) == np.float32 else self.want64

    def bound(self, dtype, field):
        """fp32: 4 e_ref against the fp64 truth (library and oracle are two fp32 evaluations of one operator, each within a small
        multiple of the other's noise). fp64: there is no higher precision; rounding noise scales with the unit roundoff
        (2^-53 / 2^-24 = 2^-29), twice that because both sides are noisy: 8 e_ref 2^-29. Neither looser than the project's tolerance."""
        d = np.dtype(dtype)
        b = FACTOR32 * self.e_ref[field] if d == np.float32 else FACTOR64 * self.e_ref[field] * 2.**-29
        return min(b, CEILING[d])
