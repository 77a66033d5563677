"""Stats on a slab (npy > 1): every rank sums its own rows, the double sums and the counts go through Master.sum_ between the sums
kernels and the finish kernels. 2 ranks on the emulation (gloo) at 16 x 32 x 10 against the single-rank sample of the same global
fields: counts, areas, frac and cover equal; profiles within the bound of stats_ref.bound(), to which a moment adds what the
difference of the two MEANS does to its terms, p * mean|x|^(p-1) * |mean_slab - mean_single| (the bound is for sums of the same
terms; the means of the two runs are themselves only within it). path is the sum of the ranks' own calc_path loops -- the
reference's loop runs per rank -- and is held against the reference's loop run on each slab where the reference tree exists."""
import ctypes as C

import numpy as np

import backends as B
import common as cm
import stats_ref as SR
from microhh_amd import stats as S
from microhh_amd.grid import Grid
from microhh_amd.model import CASES, HotPath, synthetic_global
from ranks import run_ranks

GRID = (16, 32, 10)
MASKS = ("default", "wplus", "warm")
THRES = 300.2          # of scalar 0 (300 + 0.003 z +- 0.05 on 1200 m): the upper part of the domain is `warm`
COVER = 301.5


def _make(lib, **kw):
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib, global_init=synthetic_global("drycblles", *GRID), stats=S.Stats(masks=MASKS), **kw)
    hp.stats.mask_thres("warm", hp.s[0], hp.s[0], threshold=THRES)
    hp.stats.add("th", hp.s[0], 0, ("mean", "frac", "path", "cover"), threshold=COVER)
    hp.cyclic_prognostic()
    return hp


def _flat(r):
    return {"%s/%s" % (m, k): np.asarray(v) for m, rm in r.items() for k, v in rm.items()}


def _worker(rank, world, out):
    hp = _make(B.get("emul").lib, npy=world, rank=rank)
    out.update(_flat(hp.stats.sample()))
    out["mfield"], _ = hp.stats.sampler.host_words()
    out["th"] = hp.s[0].numpy().copy()
    out["rho"] = hp.rhoref.numpy().copy()
    hp.close()


def test_two_ranks_against_one():
    hp = _make(B.get("emul").lib)
    ref = _flat(hp.stats.sample())
    g = hp.grid
    mf, _ = hp.stats.sampler.host_words()
    h = {"w": hp.w.numpy(), "u": hp.u.numpy(), "v": hp.v.numpy(), "s0": hp.s[0].numpy(), "p": hp.p.numpy(), "evisc": hp.evisc.numpy(), "th": hp.s[0].numpy()}
    parts = run_ranks(_worker, 2, backend="gloo", tag="slab-gloo", args=())
    ks, ke = g.kstart, g.kend + 1
    checked = 0
    for p in parts:
        assert set(p) - {"mfield", "th", "rho"} == set(ref)
    a, b = parts
    for key in ref:                                    # every rank holds the same finished values
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for m, mask in enumerate(MASKS):
        for name in ("nmask", "nmaskh", "area", "areah", "th_frac", "th_cover"):
            assert np.array_equal(a["%s/%s" % (mask, name)], ref["%s/%s" % (mask, name)]), (mask, name)
        for var, loc, off in (("w", 1, 0.), ("u", 0, 0.), ("v", 0, 0.), ("s0", 0, 0.), ("p", 0, 0.), ("evisc", 0, 0.), ("th", 0, 0.)):
            for op in ("mean", "2", "3", "4", "grad"):
                key = "%s/%s" % (mask, S.prof_name(var, op))
                if key not in ref:
                    continue
                half = (1 - loc) if op == "grad" else loc
                flag, nmk = SR.flags(m)[half], ref["%s/%s" % (mask, "nmaskh" if half else "nmask")]
                mean = ref["%s/%s" % (mask, var)]
                tol = SR.bound(g, ref[key][ks:ke], SR.term_scale(h, g, var, op, off, mean, mf, flag, nmk)[ks:ke])
                if op in ("2", "3", "4"):
                    dmean = np.abs(a["%s/%s" % (mask, var)][ks:ke] - mean[ks:ke])
                    lower = SR.term_scale(h, g, var, str(int(op) - 1), off, mean, mf, flag, nmk)[ks:ke]
                    tol = tol + int(op)*lower*dmean
                live = nmk[ks:ke] > 0
                diff = np.abs(a[key][ks:ke] - ref[key][ks:ke])
                assert np.array_equal(a[key] == S.fill_value(g.np_dtype), ref[key] == S.fill_value(g.np_dtype)), key
                assert np.all(diff[live] <= tol[live]), (key, float((diff[live]/tol[live]).max()))
                checked += 1
    assert checked >= 3*20
    # path: the sum over the ranks of what each rank's own loop adds, over the sum of their column counts
    fl = [SR.flags(m)[0] for m in range(len(MASKS))]
    inner = g.interior
    for m, mask in enumerate(MASKS):
        mk = (mf[inner] & fl[m]) != 0
        t = np.abs(h["th"][inner]*hp.rhoref.numpy()[g.kstart:g.kend, None, None]*g.dz[g.kstart:g.kend, None, None])[mk]
        ncol = int(mk.any(axis=0).sum())
        tol = t.size*2.**-53*t.sum()/ncol
        got = float(a["%s/th_path" % mask])
        assert abs(got - float(ref["%s/th_path" % mask])) <= tol, mask
        if SR.have_reference():
            lib = SR.shim()
            first, count = 0., 0.
            for rank, p in enumerate(parts):
                gr = Grid(GRID[0], GRID[1], GRID[2], *CASES["drycblles"]["size"], order=2, igc=g.igc, jgc=g.jgc, kgc=g.kgc, npy=2, mpicoordy=rank)
                d = SR.dims_of(gr)
                col = np.zeros(4)
                nm = np.ones(gr.kcells, dtype=np.int32)
                lib.ref_stats_columns(0, C.byref(d), cm.ptr(col), cm.ptr(p["th"]), cm.ptr(gr.dz), cm.ptr(p["rho"]), 0., COVER, cm.ptr(p["mfield"]), int(fl[m]), cm.ptr(nm))
                first += col[3]; count += col[2]
            assert count == ncol and abs(got - first/count) <= tol, mask
    hp.close()
