"""HotPath(..., ib=Dem(...)): one step() against the same sequence issued by hand on a HotPath without ib (the two IB calls and
their cyclic fills made through the entry points at the reference's two places, src/model.cxx:380 and :407), also with surface=
and forcing=; the captured step (GPU); the `ib` statistics mask; the <scalar>fluxbot_ib cross-section; the bind-time refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import backends as B
import ib_ref as R
from microhh_amd import capi, fieldio, ib
from microhh_amd.cross import Cross
from microhh_amd.ib import Dem
from microhh_amd.stats import PLUS, Stats

BACKENDS = [pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)]
GRID = (16, 8, 16)
N_IDW = 5
SBOT = 0.1
FIELDS = ("u", "v", "w", "th", "ut", "vt", "wt", "tht", "p", "evisc")


def dem_plane(amplitude=0.15):
    from microhh_amd.model import CASES
    return ib.sine_dem(GRID[0], GRID[1], *CASES["drycblles"]["size"], amplitude)


def _dem(sbcbot="flux", **kw):
    return Dem(dem_plane(), N_IDW, sbcbot=sbcbot, sbot=(SBOT,), **kw)


def _hotpath(backend, case="drycblles", grid=GRID, **kw):
    from microhh_amd.model import HotPath
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    return HotPath(case, *grid, dt=0.37, **kw)


def _surface():
    from microhh_amd.surface import Surface
    return Surface(mbcbot="noslip", ubot=0., vbot=0., sbcbot="flux", sbot=SBOT, z0m=0.1, z0h=0.1, thref_kstart=300., threfh_kstart=300.)


def _forcing():
    from microhh_amd.forcing import Forcing
    return Forcing(swlspres="uflux", uflux=0.11, utrans=0.07)


def fields(hp):
    hp.sync()
    ts = (hp.u, hp.v, hp.w, hp.s[0], hp.ut, hp.vt, hp.wt, hp.st[0], hp.p, hp.evisc)
    return {n: t.detach().cpu().numpy().copy() for n, t in zip(FIELDS, ts)}


def same(a, b):
    for n in FIELDS:
        assert np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)), n


class ByHand:
    """The immersed boundary of a HotPath WITHOUT ib=: the set-up and the tables through the module's functions, the two calls and
    their cyclic fills through the entry points."""

    def __init__(self, hp, sbcbot):
        self.hp, g, lib, torch = hp, hp.grid, hp.lib, hp.torch
        dem = R.with_halos(g, dem_plane())
        c = ib.locations(g)
        ax = {"u": (c["xh"], c["y"], g.z, g.dz), "v": (c["x"], c["yh"], g.z, g.dz), "w": (c["x"], c["y"], g.zh, g.dzh), "s": (c["x"], c["y"], g.z, g.dz)}
        self.keep, self.jobs = [], {}
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hp.device)                              # noqa: E731
        for name, fld, bc, bv in (("u", hp.u, 0, 0.), ("v", hp.v, 0, 0.), ("w", hp.w, 0, 0.), ("s", hp.s[0], R.BCS[sbcbot], SBOT)):
            gh = ib.ghost_cells(lib, g, dem, *ax[name], N_IDW, bc)
            tab = {k: dev(a) for k, a in ib.device_tables(g, gh).items()}
            dbv = dev(np.full(gh["nghost"], bv, dtype=g.np_dtype))
            self.keep += [tab, dbv]
            self.jobs[name] = ib.job(fld.data_ptr(), dbv.data_ptr(), bc, hp.cfg["visc"], gh["nghost"], {k: t.data_ptr() for k, t in tab.items()})

    def _set(self, names, flds):
        hp = self.hp
        jobs = (capi.MhhIbJob*len(names))(*[self.jobs[n] for n in names])
        capi.check(hp.lib.mhh_ib_set_ghost_cells(hp.G, N_IDW, jobs, len(names), hp.stream), hp.lib)
        ptrs = (C.c_void_p*len(flds))(*[t.data_ptr() for t in flds])
        capi.check(hp.lib.mhh_boundary_cyclic_n(hp.G, ptrs, len(flds), 2, hp.stream), hp.lib)

    def scalars(self):
        self._set(["s"], [self.hp.s[0]])

    def momentum(self):
        self._set(["u", "v", "w"], [self.hp.u, self.hp.v, self.hp.w])


def by_hand_step(hp, bh):
    """Model::exec (src/model.cxx:346-411) on a HotPath without ib=, the two IB calls at :380 and :407."""
    hp.cyclic_prognostic(); hp.exec_viscosity()
    if hp.surface is not None:
        hp.surface_layer()
    bh.scalars()
    hp.rhs()
    if hp.forcing is not None:
        hp.forcing_means(); hp.buffer_force()
    bh.momentum()
    hp.pres()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("extra", ["plain", "surface", "forcing"])
@pytest.mark.parametrize("sbcbot", ["flux", "dirichlet"])
def test_step_is_the_sequence_by_hand(backend, extra, sbcbot):
    kw = {"surface": _surface} if extra == "surface" else {"forcing": _forcing} if extra == "forcing" else {}
    a = _hotpath(backend, ib=_dem(sbcbot), **{k: f() for k, f in kw.items()})
    b = _hotpath(backend, **{k: f() for k, f in kw.items()})
    c = _hotpath(backend, **{k: f() for k, f in kw.items()})
    assert set(a.ib.ghost) == {"u", "v", "w", "s"} and a.ib.ghost["w"]["nghost"] > 256
    bh = ByHand(b, sbcbot)
    for _ in range(2):               # the second step reads what the first one left in the ghost cells
        a.step(); by_hand_step(b, bh); c.step()
        a.pres_rk(3, 0, 0.5); b.pres_rk(3, 0, 0.5); c.pres_rk(3, 0, 0.5)
    fa, fb, fc = fields(a), fields(b), fields(c)
    same(fa, fb)
    assert not np.array_equal(fa["th"], fc["th"]) and not np.array_equal(fa["ut"], fc["ut"])        # and the terrain is felt
    for hp in (a, b, c):
        hp.close()


@pytest.mark.gpu
def test_the_captured_step_is_the_step():
    a, b = _hotpath("hip", ib=_dem()), _hotpath("hip", ib=_dem())
    graph = a.capture_step()                 # runs one eager step first
    graph.replay()
    b.step(); b.step()
    a.sync()
    same(fields(a), fields(b))
    a.close(); b.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_ib_mask_is_mask_thres_by_hand(backend):
    a = _hotpath(backend, ib=_dem(), stats=Stats(masks=("default", "ib")))
    b = _hotpath(backend, ib=_dem(), stats=Stats(masks=("default", "mine")))
    b.stats.mask_thres("mine", b.ib.mask, b.ib.maskh, None, 0.5, PLUS)
    a.step(); b.step()
    ra, rb = a.stats.sample(), b.stats.sample()
    assert set(ra) == {"default", "ib"}
    for k, v in ra["ib"].items():
        assert np.array_equal(np.asarray(v).view(np.uint8), np.asarray(rb["mine"][k]).view(np.uint8)), k
    g = a.grid
    assert not np.array_equal(ra["ib"]["nmask"], ra["default"]["nmask"])
    assert not np.array_equal(ra["ib"]["s0"][g.kstart:g.kend], ra["default"]["s0"][g.kstart:g.kend])
    # the mask fields are calc_mask: 1 above the DEM of the column
    dem = R.with_halos(g, dem_plane())
    want = (g.z[:, None, None] > dem[None]).astype(g.np_dtype)
    assert np.array_equal(a.ib.mask.cpu().numpy()[g.interior], want[g.interior])
    # without ib= the name stays a mask of the caller's
    c = _hotpath(backend, stats=Stats(masks=("default", "ib")))
    c.stats.mask_thres("ib", c.w, c.w)
    c.step(); c.stats.sample()
    for hp in (a, b, c):
        hp.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fluxbot_ib_file_is_calc_fluxes(backend, dtype, tmp_path):
    """The bytes of thfluxbot_ib are calc_fluxes of the reference (the shim, or tests/golden/ib_ref.npz) on the same th: the steep
    terrain (A = 0.22) on the case's own domain, th set to the field the reference result was made from."""
    tmp = str(tmp_path)
    hp = _hotpath(backend, dtype=dtype, ib=Dem(R.hotpath_dem(), N_IDW, sbcbot="flux", sbot=(SBOT,)), cross=Cross(["th", "thfluxbot_ib"], xy=[100.], path=tmp))
    g = hp.grid
    assert (g.itot, g.jtot, g.ktot) == R.HOTPATH_GRID and g.shape3 == R.hotpath_th().shape
    hp.s[0].copy_(hp.torch.from_numpy(np.ascontiguousarray(R.hotpath_th(), dtype=g.np_dtype)).to(hp.device))
    hp.cross.sample(1800)
    fn = os.path.join(tmp, "thfluxbot_ib.xy.0001800")
    assert os.path.getsize(fn) == g.itot*g.jtot*g.np_dtype.itemsize
    got = fieldio.load_xy_slice(fn, g)
    kd = hp.ib.k_dem.cpu().numpy().view(np.uint32)
    c = kd[g.jstart:g.jend, g.istart:g.iend].astype(int)
    assert (np.diff(c, axis=1) != 0).any() and (np.diff(c, axis=0) != 0).any()          # the side loops run
    assert np.array_equal(kd, R.with_halos(g, c, dtype=np.uint32))
    want = R.GOLD.ref("hotpath/%s/flux" % R.tag(dtype))
    assert got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    hp.close()


def test_bind_time_refusals(tmp_path):
    from microhh_amd.model import CASES
    with pytest.raises(ValueError, match="fourth-order case"):
        _hotpath("emul", case="moser600", grid=(16, 12, 12), ib=Dem(np.zeros((12, 16)), N_IDW))
    with pytest.raises(ValueError, match="at least two horizontal ghost cells"):
        _hotpath("emul", case="taylorgreen", ib=Dem(ib.sine_dem(GRID[0], GRID[1], *CASES["taylorgreen"]["size"]), N_IDW))
    with pytest.raises(ValueError, match="field thfluxbot_ib in .* is illegal"):
        _hotpath("emul", cross=Cross(["th", "thfluxbot_ib"], xy=[100.], path=str(tmp_path)))
    with pytest.raises(ValueError, match="sbcbot=ustar is not a valid choice"):
        Dem(dem_plane(), N_IDW, sbcbot="ustar")
    with pytest.raises(ValueError, match="a plane of shape"):
        _hotpath("emul", ib=Dem(np.zeros((4, 4)), N_IDW))


def test_from_file_and_spatial_sbot(tmp_path):
    """Dem.from_file reads dem.0000000 and th_sbot.0000000; the boundary values are the plane interpolated to (xb, yb)."""
    tmp = str(tmp_path)
    plane = 290. + np.arange(GRID[0]*GRID[1], dtype=np.float64).reshape(GRID[1], GRID[0])
    dem_plane().astype(np.float64).tofile(os.path.join(tmp, "dem.0000000"))
    plane.tofile(os.path.join(tmp, "th_sbot.0000000"))
    a = _hotpath("emul", ib=Dem.from_file(tmp, N_IDW, sbcbot="dirichlet", sbot_spatial=(0,)))
    b = _hotpath("emul", ib=Dem(dem_plane(), N_IDW, sbcbot="dirichlet", sbot_spatial={0: plane}))
    gs = a.ib.ghost["s"]
    assert np.array_equal(gs["sbot"][0], b.ib.ghost["s"]["sbot"][0]) and gs["sbot"][0].min() >= 290. and np.ptp(gs["sbot"][0]) > 10.
    for k in R.LISTS:
        assert np.array_equal(gs[k], b.ib.ghost["s"][k])
    if R.have_reference():
        g = a.grid
        assert np.array_equal(gs["sbot"][0], R.ref_interp(g, R.with_halos(g, plane), gs["xb"], gs["yb"]))
    a.close(); b.close()
