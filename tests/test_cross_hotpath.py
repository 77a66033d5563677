"""HotPath(..., cross=Cross(...)): the files of a sample under the reference's names, each of exactly the right size and equal to
the NumPy slice of hp's host copies; exclusive creation; an illegal name refused at bind; sampling changes no state. On the
emulation, with one case on the GPU."""
import os

import numpy as np
import pytest

import backends as B
import cross_ref as R
from microhh_amd import fieldio
from microhh_amd.cross import Cross, indices

BACKENDS = [pytest.param("emul"), pytest.param("hip", marks=pytest.mark.gpu)]
EMUL = [pytest.param("emul")]
UTRANS, VTRANS = 3., -1.5
XY, XZ, YZ = 0, 1, 2
IOTIME = 1800


def _hotpath(backend, case, grid, cross, dtype=np.float64, **kw):
    from microhh_amd.model import CASES, HotPath
    from microhh_amd.surface import Surface
    from microhh_amd.thermo import Moist
    if backend == "emul":
        kw.update(device="cpu", lib=B.get("emul").lib)
    if case == "bomex":
        kw["thermo"] = Moist(CASES["bomex"]["pbot"])
    if case != "moser600":
        kw["surface"] = Surface()
    return HotPath(case, *grid, dt=2., dtype=dtype, cross=cross, **kw)


def host(t):
    return t.detach().cpu().numpy().copy()


def sections(hp, cr, loc):
    """[(section, global index, job kind, array index)] of a variable at location loc (s | u | v | w) for the plain section; the
    full lists for everything else (loc "s"): Cross::cross_simple (src/cross.cxx:564-636), restated."""
    g = hp.grid
    kxy, kxyh = indices(hp.lib, g, XY, cr.xy)
    jxz, jxzh = indices(hp.lib, g, XZ, cr.xz)
    ixz, ixzh = indices(hp.lib, g, YZ, cr.yz)
    out = [("xz", j, XZ, j + g.jgc) for j in (jxzh if loc == "v" else jxz)]
    out += [("yz", i, YZ, i % g.imax + g.igc) for i in (ixzh if loc == "u" else ixz)]
    out += [("xy", k, XY, k + g.kgc) for k in (kxyh if loc == "w" else kxy)]
    return out


def check_files(hp, cr, tmp, expect):
    """expect: {name: (host array, loc, offset, "simple" | "plane")}: every file there, no other, the right size, the right bytes."""
    g = hp.grid
    names = set()
    for name, (a, loc, off, op) in expect.items():
        if op == "plane":
            fn = fieldio.cross_filename(tmp, name, "xy", None, IOTIME)
            assert os.path.basename(fn) == "%s.xy.%07d" % (name, IOTIME)
            assert os.path.getsize(fn) == g.jtot*g.itot*g.np_dtype.itemsize
            assert np.array_equal(fieldio.load_xy_slice(fn, g).view(np.uint8), np.ascontiguousarray(R.numpy_plane(g, a, R.PLANE, 0, 0, 0, off)).view(np.uint8)), name
            names.add(fn)
            continue
        for sect, gi, kind, idx in sections(hp, cr, loc):
            fn = os.path.join(tmp, "%s.%s.%05d.%07d" % (name, sect, gi, IOTIME))
            want = np.ascontiguousarray(R.numpy_plane(g, a, kind, idx, g.kstart, g.kend, off))
            assert os.path.getsize(fn) == want.size*g.np_dtype.itemsize, fn
            got = {"xy": fieldio.load_xy_slice, "xz": fieldio.load_xz_slice, "yz": fieldio.load_yz_slice}[sect](fn, g)
            if op == "simple":
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), fn
            else:                                                # lngrad: `a` is the reference's lngrad field, held within the bound
                assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= R.lngrad_bound(g, want)), fn
            names.add(fn)
    assert {os.path.join(tmp, f) for f in os.listdir(tmp)} == names


@pytest.mark.parametrize("backend", BACKENDS)
def test_drycblles_files(backend, tmp_path):
    tmp = str(tmp_path)
    grid = (32, 8, 16)
    cr = Cross(["u", "v", "w", "th", "thfluxbot", "ufluxbot", "thpath", "ustar", "obuk", "ubot", "thbot", "b", "evisc"],
               xy=[0., 610., 1200.], xz=[0., 1700., 3200.], yz=[0., 1650., 3200.], path=tmp, utrans=UTRANS, vtrans=VTRANS)
    hp = _hotpath(backend, "drycblles", grid, cr)
    g = hp.grid
    hp.step()
    before = {n: host(t) for n, t in (("u", hp.u), ("v", hp.v), ("w", hp.w), ("th", hp.s[0]), ("ut", hp.ut), ("vt", hp.vt), ("wt", hp.wt), ("tht", hp.st[0]))}
    written = hp.cross.sample(IOTIME)
    assert len(written) == len(set(written)) == len(os.listdir(tmp))
    after = {n: host(t) for n, t in (("u", hp.u), ("v", hp.v), ("w", hp.w), ("th", hp.s[0]), ("ut", hp.ut), ("vt", hp.vt), ("wt", hp.wt), ("tht", hp.st[0]))}
    for n in before:                                             # fields and tendencies: the same bits before and after a sample
        assert np.array_equal(before[n].view(np.uint8), after[n].view(np.uint8)), n
    th = after["th"]
    b = (9.81/host(hp.thref)[:, None, None]*(th - host(hp.thref)[:, None, None])).astype(g.np_dtype)      # calc_buoyancy (src/thermo_dry.cxx:51-63)
    rho, t = host(hp.rhoref), g.np_dtype.type
    path = np.zeros(g.shape2, dtype=g.np_dtype)
    for k in range(g.kstart, g.kend):                            # calc_cross_path (src/cross.cxx:170-197)
        path = path + (t(rho[k])*th[k])*t(g.dz[k])
    sf = hp.surface
    # the leftover offset of fluxbot: evisc, a diagnostic field, is the last plain section, so it is none (src/fields.cxx:1241-1245)
    expect = {"u": (after["u"], "u", UTRANS, "simple"), "v": (after["v"], "v", VTRANS, "simple"), "w": (after["w"], "w", 0., "simple"),
              "th": (th, "s", 0., "simple"), "b": (b, "s", 0., "simple"), "evisc": (host(hp.evisc), "s", 0., "simple"),
              "thfluxbot": (host(sf.sfluxbot[0]), "s", 0., "plane"), "ufluxbot": (host(hp.surf["u_fluxbot"]), "s", 0., "plane"),
              "thpath": (path, "s", 0., "plane"), "ustar": (host(sf.ustar), "s", 0., "plane"), "obuk": (host(sf.obuk), "s", 0., "plane"),
              "ubot": (host(sf.ubot_t), "s", UTRANS, "plane"), "thbot": (host(sf.sbot[0]), "s", 0., "plane")}
    check_files(hp, cr, tmp, expect)
    # the half-level lists were used: v has the row jtot (the north ghost row), u the column itot (column 0), w the level ktot
    assert os.path.exists(os.path.join(tmp, "v.xz.%05d.%07d" % (g.jtot, IOTIME))) and os.path.exists(os.path.join(tmp, "w.xy.%05d.%07d" % (g.ktot, IOTIME)))
    assert os.path.exists(os.path.join(tmp, "u.yz.%05d.%07d" % (g.itot, IOTIME)))
    with pytest.raises(FileExistsError):                         # "wbx": a second sample at the same iotime
        hp.cross.sample(IOTIME)
    hp.close()


@pytest.mark.parametrize("backend", EMUL)
def test_leftover_offset_of_fluxbot(backend, tmp_path):
    """fluxbot and fluxtop take the offset the last plain section left: v's, where v is the last listed prognostic field by name."""
    tmp = str(tmp_path)
    cr = Cross(["v", "u", "thfluxbot", "thfluxtop"], xy=[100.], path=tmp, utrans=UTRANS, vtrans=VTRANS)
    hp = _hotpath(backend, "drycblles", (16, 8, 8), cr)
    hp.step()
    hp.cross.sample(IOTIME)
    g = hp.grid
    for name, a in (("thfluxbot", hp.surface.sfluxbot[0]), ("thfluxtop", hp.surf["s_fluxtop"])):
        got = fieldio.load_xy_slice(fieldio.cross_filename(tmp, name, "xy", None, IOTIME), g)
        assert np.array_equal(got, host(a)[g.jstart:g.jend, g.istart:g.iend] + VTRANS)
    hp.close()


@pytest.mark.parametrize("backend", EMUL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_bomex_files(backend, dtype, tmp_path):
    tmp = str(tmp_path)
    cr = Cross(["ql", "qlpath", "qlbase", "qltop", "b", "qt", "qlqipath"], xy=[700., 1500.], xz=[3200.], yz=[3200.], path=tmp)
    hp = _hotpath(backend, "bomex", (32, 8, 32), cr, dtype=dtype)
    g = hp.grid
    hp.step()
    hp.cross.sample(IOTIME)
    ql, qi, b = host(hp.thermo.field("ql")), host(hp.thermo.field("qi")), host(hp.thermo.field("b"))
    assert (ql[g.interior] > 0).any()
    rho, t = host(hp.rhoref), g.np_dtype.type
    path, pathqi = np.zeros(g.shape2, dtype=g.np_dtype), np.zeros(g.shape2, dtype=g.np_dtype)
    for k in range(g.kstart, g.kend):
        path = path + (t(rho[k])*ql[k])*t(g.dz[k])
        pathqi = pathqi + (t(rho[k])*(ql[k] + qi[k]))*t(g.dz[k])
    cloudy = ql[g.kstart:g.kend] > 0                              # calc_cross_height_threshold (src/cross.cxx:200-250), threshold 0
    z = g.z[g.kstart:g.kend][:, None, None]
    fill = t(-1e-9)
    base = np.where(cloudy.any(axis=0), np.where(cloudy, z, np.inf).min(axis=0), fill).astype(g.np_dtype)
    top = np.where(cloudy.any(axis=0), np.where(cloudy, z, -np.inf).max(axis=0), fill).astype(g.np_dtype)
    assert (base != fill).any() and (base == fill).any() and (top[base != fill] >= base[base != fill]).all()
    expect = {"ql": (ql, "s", 0., "simple"), "b": (b, "s", 0., "simple"), "qt": (host(hp.s[1]), "s", 0., "simple"),
              "qlpath": (path, "s", 0., "plane"), "qlqipath": (pathqi, "s", 0., "plane"), "qlbase": (base, "s", 0., "plane"), "qltop": (top, "s", 0., "plane")}
    check_files(hp, cr, tmp, expect)
    hp.close()


@pytest.mark.parametrize("backend", EMUL)
def test_an_illegal_name_is_refused_at_bind(backend, tmp_path):
    for case, grid, bad in (("drycblles", (16, 8, 8), "ql"), ("drycblles", (16, 8, 8), "qsatpath"), ("drycblles", (16, 8, 8), "ulngrad"),
                            ("drycblles", (16, 8, 8), "lflx"), ("bomex", (16, 8, 8), "rr_bot"), ("bomex", (16, 8, 8), "w500hpa")):
        with pytest.raises(ValueError, match="field %s in .* is illegal" % bad):
            _hotpath(backend, case, grid, Cross(["u", bad], xy=[0.], path=str(tmp_path)))
    with pytest.raises(ValueError, match="Empty cross-section list"):
        Cross([])
    from microhh_amd import capi
    with pytest.raises(capi.MhhError, match=r"in \[cross\]\[xy\] is outside domain"):
        _hotpath(backend, "drycblles", (16, 8, 8), Cross(["u"], xy=[5000.], path=str(tmp_path)))


@pytest.mark.parametrize("backend", EMUL)
def test_sampling_between_steps_changes_nothing(backend, tmp_path):
    """step(); sample(); step() equals step(); step() bit for bit, with the steps integrating (pres_rk) so that the fields move."""
    def run(sample):
        cr = Cross(["u", "w", "th", "thlngrad", "thpath", "b", "blngrad"], xy=[300.], xz=[3200.], yz=[100.], path=str(tmp_path))
        hp = _hotpath(backend, "drycblles", (16, 8, 8), cr)
        for n in range(2):
            hp.step()
            hp.pres_rk(3, n, 0.5)
            if sample and n == 0:
                hp.cross.sample(IOTIME)
        out = [host(x) for x in (hp.u, hp.v, hp.w, hp.s[0], hp.ut, hp.vt, hp.wt, hp.st[0], hp.p, hp.evisc)]
        hp.close()
        return out
    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert len(os.listdir(str(tmp_path))) > 0


@pytest.mark.parametrize("backend", EMUL)
def test_moser600_lngrad_against_the_reference(backend, tmp_path):
    """Order 4: u and ulngrad write; ulngrad matches calc_lngrad_4th of the reference on hp's host copy of u within the bound of
    tests/test_cross_kernels.py (where the reference tree is absent: the files exist with the right sizes and finite values)."""
    tmp = str(tmp_path)
    cr = Cross(["u", "ulngrad"], xy=[0.3, 1.], xz=[1.], yz=[2.], path=tmp)
    hp = _hotpath(backend, "moser600", (16, 12, 12), cr)
    g = hp.grid
    hp.cyclic_prognostic()
    hp.cross.sample(IOTIME)
    u = host(hp.u)
    if R.have_reference():
        expect = {"u": (u, "u", 0., "simple"), "ulngrad": (R.ref_lngrad(g, u), "s", 0., "lngrad")}
        check_files(hp, cr, tmp, expect)
    else:
        expect = {"u": (u, "u", 0., "simple")}
        for f in os.listdir(tmp):
            if f.startswith("ulngrad"):
                a = np.fromfile(os.path.join(tmp, f), dtype=g.np_dtype)
                assert a.size in (g.imax*g.jmax, g.imax*g.kmax, g.jmax*g.kmax) and np.all(np.isfinite(a))
                os.remove(os.path.join(tmp, f))
        check_files(hp, cr, tmp, expect)
    hp.close()
