"""Pin the oracle: bit-for-bit equality with the reference's own kernels (oracle/_ref, built from the
reference sources in place with identical flags -O2 -ffp-contract=off) on seeded random fields, for
every stencil kernel of SURVEY.md §8a that the reference TU exposes without Grid/FFTW.

Where oracle/_ref is absent (a checkout without the reference) the oracle's outputs are held against
tests/golden/ref_digests.json instead: the SHA-256 of every reference output array and the exact value of every
reference scalar below, on the same inputs. The stretched grids of both ways are built from the z profiles stored
in that file (moser_z's last bits follow the host's numpy). Recorded where the reference library exists, with
the whole module:  MHH_RECORD_REF_DIGESTS=1 python -m pytest tests/test_oracle_vs_ref.py"""
import hashlib
import json
import os

import numpy as np
import pytest

import common as cm
from common import ptr, dbl

REF = cm.ref()
DIGESTS = os.path.join(cm.ROOT, "tests", "golden", "ref_digests.json")
RECORD = {"z": {}, "out": {}} if os.environ.get("MHH_RECORD_REF_DIGESTS") == "1" else None
if RECORD is not None and REF is None:
    raise RuntimeError("recording tests/golden/ref_digests.json needs the reference library (oracle/_ref)")
GOLD = None
if RECORD is None:
    with open(DIGESTS) as _f:
        GOLD = json.load(_f)

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    if RECORD is not None:
        with open(DIGESTS, "w") as f:
            json.dump(RECORD, f, indent=0, sort_keys=True)
            f.write("\n")


def _z(ktot, zsize):
    key = "%d/%r" % (ktot, zsize)
    if RECORD is not None:
        RECORD["z"][key] = cm.moser_z(ktot, zsize).tolist()
        return np.array(RECORD["z"][key])
    return np.array(GOLD["z"][key])


def _digest(a):
    a = np.ascontiguousarray(a)
    return "%s %s %s" % (a.dtype.str, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest())


def same_as_ref(key, got, run_ref):
    """`got`: the oracle's output (array or scalar); `run_ref()`: the reference's own on the same inputs. Returns (equal, detail):
    bit-for-bit against the reference library where it exists, against its recorded output where not."""
    key = "/".join(map(str, key))
    scalar = np.ndim(got) == 0
    if REF is None:
        want = GOLD["out"][key]
        return (float(got).hex() if scalar else _digest(got)) == want, ("recorded reference output", key)
    want = run_ref()
    if RECORD is not None:
        RECORD["out"][key] = float(want).hex() if scalar else _digest(want)
    if scalar:
        return got == want, (key, got, want)
    return np.array_equal(got, want), (key, cm.ulp_diff(got, want))


def _shape(g):
    return "x".join(map(str, g.shape3))


def grids2(dtype):
    return [cm.grid_2nd(*gs[:3], gc=gs[3:], dtype=dtype, z=_z(gs[2], 1200.)) for gs in cm.SMALL_GRIDS_2] + \
           [cm.grid_2nd(12, 1, 8, gc=(3, 3, 1), dtype=dtype, z=_z(8, 1200.))]          # 2-D run (jtot == 1)


def grids4(dtype):
    return [cm.grid_4th(16, 12, 12, dtype=dtype, z=_z(12, 2.)), cm.grid_4th(10, 8, 8, dtype=dtype, z=_z(8, 2.)),
            cm.grid_4th(12, 1, 8, dtype=dtype, z=_z(8, 2.))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme,refname", [(cm.ADVEC_2, "ref_advec_2"), (cm.ADVEC_2I5, "ref_advec_2i5"), (cm.ADVEC_2I4, "ref_advec_2i4"), (cm.ADVEC_2I62, "ref_advec_2i62"), (cm.ADVEC_2I53, "ref_advec_2i53"), (cm.ADVEC_4, "ref_advec_4"), (cm.ADVEC_4M, "ref_advec_4m")])
def test_advec_bitwise(scheme, refname, dtype):
    O = cm.oracle()
    for g in (grids4(dtype) if scheme in (cm.ADVEC_4, cm.ADVEC_4M) else grids2(dtype)):
        if scheme == cm.ADVEC_2I5 and g.ktot < 6:
            continue
        if scheme in (cm.ADVEC_2I4, cm.ADVEC_2I53) and (g.igc < 2 or g.jgc < 2 or g.ktot < 4):
            continue
        c = cm.Case(g)
        G = g.host_struct()
        key = ("advec", refname, g.np_dtype.name, _shape(g))
        for comp, (oname, tname) in enumerate([("orc_advec_u", "ut"), ("orc_advec_v", "vt"), ("orc_advec_w", "wt")]):
            t_o, t_r = c.copy_of(tname), c.copy_of(tname)
            getattr(O, oname)(G, scheme, ptr(t_o), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))

            def run_ref():
                getattr(REF, refname)(G, comp, ptr(t_r), None, ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))
                return t_r
            ok, why = same_as_ref(key + (tname,), t_o, run_ref)
            assert ok, why
            assert not np.array_equal(t_o, getattr(c, tname))
        t_o, t_r = c.st[0].copy(), c.st[0].copy()
        O.orc_advec_s(G, scheme, ptr(t_o), ptr(c.s[0]), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))

        def run_ref_s():
            getattr(REF, refname)(G, 3, ptr(t_r), ptr(c.s[0]), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.rhoref), ptr(c.rhorefh))
            return t_r
        ok, why = same_as_ref(key + ("st",), t_o, run_ref_s)
        assert ok, why
        cfl_o = O.orc_advec_cfl(G, scheme, ptr(c.u), ptr(c.v), ptr(c.w), dbl(0.37))
        ok, why = same_as_ref(key + ("cfl",), cfl_o, lambda: getattr(REF, refname + "_cfl")(G, ptr(c.u), ptr(c.v), ptr(c.w), dbl(0.37)))
        assert ok and cfl_o > 0, why


@pytest.mark.parametrize("dtype", DTYPES)
def test_advec_s_lim_bitwise(dtype):
    """Koren flux limiter (include/advec_monotonic.h:10-180) against the reference's own template."""
    O = cm.oracle()
    for g in grids2(dtype) + [cm.grid_2nd(12, 8, 8, gc=(3, 3, 2), dtype=dtype, z=_z(8, 1200.))]:
        if g.ktot < 6:
            continue
        c = cm.Case(g)
        G = g.host_struct()
        u, v, w, s = cm.limiter_inputs(c, dtype)
        t_o, t_r = c.st[0].copy(), c.st[0].copy()
        O.orc_advec_s_lim(G, ptr(t_o), ptr(s), ptr(u), ptr(v), ptr(w), ptr(c.rhoref), ptr(c.rhorefh))

        def run_ref():
            REF.ref_advec_s_lim(G, ptr(t_r), ptr(s), ptr(u), ptr(v), ptr(w), ptr(c.rhoref), ptr(c.rhorefh))
            return t_r
        ok, why = same_as_ref(("advec_s_lim", g.np_dtype.name, _shape(g)), t_o, run_ref)
        assert ok, why
        assert not np.array_equal(t_o, c.st[0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [2, 4])
def test_diff_bitwise(order, dtype):
    O = cm.oracle()
    for g in (grids4(dtype) if order == 4 else grids2(dtype)):
        c = cm.Case(g)
        G = g.host_struct()
        for is_w, fld, tname in [(0, c.u, "ut"), (1, c.w, "wt"), (0, c.s[0], "vt")]:
            t_o, t_r = c.copy_of(tname), c.copy_of(tname)
            (O.orc_diff_w if is_w else O.orc_diff_c)(G, order, ptr(t_o), ptr(fld), dbl(1.3e-2))

            def run_ref():
                getattr(REF, "ref_diff_%d" % order)(G, is_w, ptr(t_r), ptr(fld), dbl(1.3e-2))
                return t_r
            ok, why = same_as_ref(("diff", order, g.np_dtype.name, _shape(g), tname), t_o, run_ref)
            assert ok, why
            assert not np.array_equal(t_o, getattr(c, tname))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sm", [0, 1])
def test_smag2_bitwise(sm, dtype):
    O = cm.oracle()
    for g in grids2(dtype):
        if g.jtot == 1:
            continue
        c = cm.Case(g)
        G = g.host_struct()
        key = ("smag2", sm, g.np_dtype.name, _shape(g))
        s_o = np.zeros(g.shape3, dtype=dtype); s_r = np.zeros(g.shape3, dtype=dtype)
        O.orc_smag2_strain2(G, sm, ptr(s_o), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.dudz), ptr(c.dvdz))

        def run_ref_strain2():
            REF.ref_smag2_strain2(G, sm, ptr(s_r), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.dudz), ptr(c.dvdz))
            return s_r
        ok, why = same_as_ref(key + ("strain2",), s_o, run_ref_strain2)
        assert ok and s_o[g.interior].min() > 0, why
        for comp, (oname, tname, fb, ft) in enumerate([("orc_smag2_diff_u", "ut", c.u_fluxbot, c.u_fluxtop),
                                                       ("orc_smag2_diff_v", "vt", c.v_fluxbot, c.v_fluxtop)]):
            t_o, t_r = c.copy_of(tname), c.copy_of(tname)
            getattr(O, oname)(G, sm, ptr(t_o), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(fb), ptr(ft), ptr(c.rhoref), ptr(c.rhorefh), dbl(1e-5))

            def run_ref_uv():
                REF.ref_smag2_diff_uvw(G, comp, sm, ptr(t_r), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(fb), ptr(ft), ptr(c.rhoref), ptr(c.rhorefh), dbl(1e-5))
                return t_r
            ok, why = same_as_ref(key + (tname,), t_o, run_ref_uv)
            assert ok, (oname, sm, why)
        t_o, t_r = c.copy_of("wt"), c.copy_of("wt")
        O.orc_smag2_diff_w(G, ptr(t_o), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), ptr(c.rhoref), ptr(c.rhorefh), dbl(1e-5))

        def run_ref_w():
            REF.ref_smag2_diff_uvw(G, 2, sm, ptr(t_r), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.evisc), None, None, ptr(c.rhoref), ptr(c.rhorefh), dbl(1e-5))
            return t_r
        ok, why = same_as_ref(key + ("wt",), t_o, run_ref_w)
        assert ok, why
        t_o, t_r = c.st[0].copy(), c.st[0].copy()
        O.orc_smag2_diff_c(G, sm, ptr(t_o), ptr(c.s[0]), ptr(c.evisc), ptr(c.s_fluxbot), ptr(c.s_fluxtop), ptr(c.rhoref), ptr(c.rhorefh), dbl(1./3.), dbl(1e-5))

        def run_ref_c():
            REF.ref_smag2_diff_c(G, sm, ptr(t_r), ptr(c.s[0]), ptr(c.evisc), ptr(c.s_fluxbot), ptr(c.s_fluxtop), ptr(c.rhoref), ptr(c.rhorefh), dbl(1./3.), dbl(1e-5))
            return t_r
        ok, why = same_as_ref(key + ("st",), t_o, run_ref_c)
        assert ok, why
        for tPr in (1./3., 1.7):
            ok, why = same_as_ref(key + ("dnmul", repr(tPr)), O.orc_smag2_dnmul(G, ptr(c.evisc), dbl(tPr)),
                                  lambda: REF.ref_smag2_dnmul(G, ptr(c.evisc), dbl(tPr)))
            assert ok, why
