"""The mask machinery of csrc/stats.h against the reference's own calc_mask_thres, calc_nmask and calc_area (src/stats.cxx, behind
tests/cpp/ref_stats_shim.cpp, or tests/golden/stats_ref.npz): the words over ALL cells after initialize_masks, after every threshold
and after finalize_masks, the counts and the areas -- bit for bit on every backend."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import stats_ref as SR
from backends import be  # noqa: F401
from microhh_amd import capi
from microhh_amd import stats as S

CASES = SR.all_cases()
IDS = ["%s-gc%d%d%d" % ((SR.case_of(s, k).key,) + gc) for s, gc, k in CASES]


def test_golden_file_matches_the_seeded_inputs():
    """Recording (MHH_RECORD_STATS_GOLDEN=1) happens here; the file's digests are those of the inputs this host draws."""
    SR.record_if_asked()
    z = SR.golden()
    assert z is not None, "tests/golden/stats_ref.npz is missing"
    for shape, gc, kind in CASES:
        c = SR.case_of(shape, kind)
        assert str(z["digest/%s" % c.key]) == c.digest(), c.key
    if SR.have_reference() and not SR.RECORD:          # and what it holds is what the reference gives here
        rec = SR.computed()
        assert sorted(rec) == sorted(z.files)
        for k in rec:
            assert np.array_equal(rec[k], z[k], equal_nan=(rec[k].dtype.kind == "f")), k


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
@pytest.mark.parametrize("shape,gc,kind", CASES, ids=IDS)
def test_words_counts_and_areas_bit_for_bit(be, shape, gc, kind, dtype):  # noqa: F811
    dev = SR.Dev(be, shape, gc, dtype, kind)
    g = dev.g
    stages = []
    dev.masks(stages)
    r = lambda name: SR.ref(shape, gc, dtype, kind, name, be)      # noqa: E731
    flagmax = sum(int(f) for n in range(len(SR.MASKS)) for f in SR.flags(n))
    assert np.all(stages[0][0] == flagmax) and np.all(stages[0][1] == flagmax)           # ghosts included
    for n in (1, 2):
        assert np.array_equal(stages[n][0], r("mfield%d" % n)), "mfield after threshold %d" % n
        assert np.array_equal(stages[n][1], r("mfield_bot%d" % n)), "mfield_bot after threshold %d" % n
    mf, mb = dev.s.host_words()
    assert np.array_equal(mf, r("mfield")) and np.array_equal(mb, r("mfield_bot"))
    nmask = dev.s.nmask.cpu().numpy()
    assert np.array_equal(nmask, r("nmask"))
    assert np.array_equal(dev.s.nmask_bot.cpu().numpy(), r("nmask_bot"))
    for name in ("area", "areah"):
        got, want = getattr(dev.s, name).cpu().numpy(), r(name)
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    # the fixture is what it claims to be
    ks, ke = g.kstart, g.kend
    if kind == "seeded":
        sp, tl = SR.MASKS.index("sparse"), SR.MASKS.index("topless")
        assert nmask[sp].min() > 0 and abs(nmask[sp, 0, ks:ke].sum()/(g.itot*g.jtot*g.ktot) - 1./3.) < 0.1
        assert nmask[tl, 0, ke-1] == 0 and nmask[tl, 1, ke-1] == 0 and r("area")[tl, ke-1] == 0
    assert np.all(nmask[0] == g.itot*g.jtot) and np.all(r("area")[0, ks:ke] == 1)


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=SR.tag)
def test_nan_clears_nothing_and_min_complements_plus(be, dtype):  # noqa: F811
    """NaN <= t and NaN > t are both false: a NaN never clears a bit, in either mode. Elsewhere Min keeps what Plus clears."""
    shape, gc = SR.SHAPES[1], (1, 1, 1)
    dev = SR.Dev(be, shape, gc, dtype)
    g = dev.g
    h = {k: v.copy() for k, v in dev.h.items()}
    nan3 = np.zeros(g.shape3, dtype=bool); nan3[:, g.jstart+1, g.istart+2] = True; nan3[g.kstart+2, g.jstart:g.jend, g.istart+4] = True
    for k in ("sparse", "sparseh"):
        h[k][nan3] = np.nan
    h["sparse_bot"][g.jstart+1, g.istart+2] = np.nan
    d = {k: dev.tensor(h[k]) for k in ("sparse", "sparseh", "sparse_bot")}
    words = {}
    for mode in (S.PLUS, S.MIN):
        dev.s.initialize_masks()
        dev.s.set_mask_thres("sparse", d["sparse"], d["sparseh"], d["sparse_bot"], 0., mode)
        be.sync()
        words[mode] = dev.s.host_words()
    fl, flh = SR.flags(SR.MASKS.index("sparse"))
    inner = (slice(None), slice(g.jstart, g.jend), slice(g.istart, g.iend))
    both = int(fl) | int(flh)
    p3, m3 = words[S.PLUS][0][inner] & both, words[S.MIN][0][inner] & both
    # a column of NaN keeps both flags on every level in both modes, ghost levels included
    assert np.all(p3[:, 1, 2] == both) and np.all(m3[:, 1, 2] == both)
    nan_src = nan3[inner]
    clean = ~nan_src.any(axis=0)                         # columns without a NaN: the two modes are complements on every level
    assert np.all((p3 ^ m3)[:, clean] == both)
    pb, mb = words[S.PLUS][1][inner[1:]] & int(fl), words[S.MIN][1][inner[1:]] & int(fl)
    assert pb[1, 2] == int(fl) and mb[1, 2] == int(fl)
    assert np.all((pb ^ mb)[clean] == int(fl))
    other = 63 & ~both                                   # and no other mask's bit moved
    assert np.all(words[S.PLUS][0] & other == other) and np.all(words[S.MIN][0] & other == other)


def test_refusals_name_their_reason(be):  # noqa: F811
    dev = SR.Dev(be, SR.SHAPES[1], (1, 1, 1), np.float64)
    s, lib = dev.s, be.lib
    with pytest.raises(ValueError, match="Invalid mask name"):
        s.set_mask_thres("nosuch", dev.d["a"], dev.d["a"])
    with pytest.raises(capi.MhhError, match="Invalid mask type"):
        s.set_mask_thres("sparse", dev.d["a"], dev.d["a"], mode=2)
    with pytest.raises(capi.MhhError, match="MHH_STATS_MAX_MASKS"):
        capi.check(lib.mhh_stats_mask_init(dev.G, s.mfield.data_ptr(), s.mfield_bot.data_ptr(), 9, be.stream), lib)
    with pytest.raises(capi.MhhError, match="unknown operation"):
        s.sums([(dev.d["a"], 0, 99, 0., 0., None)])
    with pytest.raises(capi.MhhError, match="needs the finished mean"):
        s.sums([(dev.d["a"], 0, S.MOMENT2, 0., 0., None)])
    with pytest.raises(ValueError, match="second-order"):
        from microhh_amd.grid import Grid
        g4 = Grid(16, 8, 8, 1., 1., 1., order=4)
        S.Sampler(lib, g4, g4.host_struct(), dev.torch, dev.device)
    for name in ("qlcore", "bplus", "bmin"):
        with pytest.raises(ValueError, match="is not built"):
            S.Stats(masks=("default", name))
    with pytest.raises(ValueError, match="a flux needs flux="):
        S.Stats().add("a", dev.d["a"], 0, ("mean", "w"))
    with pytest.raises(ValueError, match="unknown operation"):
        S.Stats().add("a", dev.d["a"], 0, ("mean", "median"))
    assert C.sizeof(capi.MhhStatsJob) == 120
