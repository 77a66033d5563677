"""The summation order of the level reductions (csrc/level_reduce.h), restated in NumPy and compared bit for bit.

A block owns one level and a chunk of ROWS rows. Thread (ty, tx) of its BY x BX threads adds the cells j = j0 + ty step BY,
i = istart + tx step BX of the chunk, in that order, into a double. The 256 accumulators of the block are then added either in a
binary tree (the horizontal means, mhh_field_mean_profile and mhh_field_mean_sum) or as sixteen runs of sixteen consecutive thread
ids followed by the sixteen runs (the masked sums, mhh_stats_sums and mhh_budget_2_*_sums). The chunks of a level are added in
index order. The other tests of these entry points allow any order within the summation bound; this one allows one.

Cases are the smallest at which each piece can go wrong: 130 columns give threads 0 and 1 three cells of a row and the others two,
37 rows give two chunks of which the second holds 5 rows (ty = 0 takes two of them), 260 levels make the finish kernel of
mhh_field_mean_sum add twice in a thread, 1, 2, 3 and 5 masks take the four accumulator widths, at 3 and 5 with mask slots that do
not exist, and the gradient's q*dzhi is the one product that is added, so it pins "no contraction". Ghost cells in i and j hold 1e30.
It is the fp64 cases that tell one order from another: a few thousand fp32 values add exactly in double, in any order, and what the
fp32 cases pin is where a value is rounded to fp32 (the product with dz, the difference of the gradient, the quotient of a mean).

The chunks of a level are dealt to the blocks by level_tiling / level_tile (strips of sr chunks, units round-robin over the 8 XCDs).
SHAPE has 2 chunks; MORE (means_common.LEVEL_SHAPES) has 8, 9, 16, 17, 25 and 32 of them on 6 columns: sr = 1, 2, 3 and 4, whole and
cut last strips, a last round of units with idle slots -- the tilings of jtot = 256, 512 and 1024. A chunk decoded twice, not at all
or with the wrong rows changes a level's sum.

Runs on the ``emul`` backend and on the ``hip`` backend (marked gpu)."""
import numpy as np
import pytest

from backends import be  # noqa: F401
from common import DTYPES, same_bits as same
from means_common import grid, fields, profiles, sums, LEVEL_SHAPES
from microhh_amd import stats as S

BX, BY, ROWS = 64, 4, 32
SHAPE = (130, 37, 4)
TALL = (2, 1, 260)
MORE = [s for s in LEVEL_SHAPES if s != SHAPE]
MORE_IDS = ["%dx%dx%d" % s for s in MORE]
THRESHOLDS = (0.2, 0.4, 0.6, 0.8)


# ---- the order ------------------------------------------------------------------------------------------------------------------
def thread_acc(t):
    """t[..., rows, imax], the terms of one chunk -> acc[..., BY*BX] by thread id tx + ty*BX."""
    acc = np.zeros(t.shape[:-2] + (BY, BX))
    for r0 in range(0, t.shape[-2], BY):
        for c0 in range(0, t.shape[-1], BX):
            blk = t[..., r0:r0+BY, c0:c0+BX]
            acc[..., :blk.shape[-2], :blk.shape[-1]] += blk
    return acc.reshape(t.shape[:-2] + (BY*BX,))


def tree(a):
    """The binary tree over the last axis: a[t] += a[t+s] for s = n/2, n/4, .. 1."""
    a = a.copy()
    s = a.shape[-1] // 2
    while s:
        a[..., :s] += a[..., s:2*s]
        s //= 2
    return a[..., 0]


def runs16(a):
    """Sixteen runs of sixteen consecutive thread ids, each added in order from zero, then the sixteen runs in order."""
    r = a.reshape(a.shape[:-1] + (16, 16))
    run = np.zeros(r.shape[:-1])
    for c in range(16):
        run = run + r[..., c]
    out = np.zeros(run.shape[:-1])
    for c in range(16):
        out = out + run[..., c]
    return out


def level_sums(t, block):
    """t[..., jmax, imax] -> [...]: the chunks of ROWS rows, each reduced by `block`, added in index order from zero."""
    tmp = np.zeros(t.shape[:-2])
    for j0 in range(0, t.shape[-2], ROWS):
        tmp = tmp + block(thread_acc(t[..., j0:j0+ROWS, :]))
    return tmp


def interior(g, a):
    return a[:, g.jstart:g.jend, g.istart:g.iend]


# ---- the horizontal means -------------------------------------------------------------------------------------------------------
def test_the_chunk_rows_are_the_one_constant(be):
    assert int(be.lib.mhh_field_mean_chunk_rows()) == ROWS and int(be.lib.mhh_stats_chunk_rows()) == ROWS


def mean_profile_is_the_tree_order(be, dtype, shape):
    g = grid(shape, dtype)
    host = fields(g, 2)
    got = profiles(be, g, be.grid(g), [be.arr(a) for a in host])
    n = float(g.itot * g.jtot)
    for f in range(2):
        tmp = level_sums(interior(g, host[f]).astype(np.float64), tree)        # every level of kcells
        assert same(got[f], (tmp / n).astype(dtype)), f


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_profile_is_the_tree_order(be, dtype):
    mean_profile_is_the_tree_order(be, dtype, SHAPE)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MORE, ids=MORE_IDS)
def test_mean_profile_is_the_tree_order_over_many_chunks(be, dtype, shape):
    mean_profile_is_the_tree_order(be, dtype, shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPE, TALL] + MORE)
def test_mean_sum_is_the_tree_order_and_the_finish_kernels(be, dtype, shape):
    g = grid(shape, dtype)
    host = fields(g, 2)
    got = sums(be, g, be.grid(g), [be.arr(a) for a in host])
    want = np.zeros(2)
    for f in range(2):
        x = interior(g, host[f])[g.kstart:g.kend] * g.dz[g.kstart:g.kend, None, None]       # the product in TF
        assert x.dtype == g.np_dtype
        lev = level_sums(x.astype(np.float64), tree)
        acc = np.zeros(256)
        for k in range(g.kmax):                                    # thread t: the levels t, t+256, ... in order
            acc[k % 256] += lev[k]
        want[f] = tree(acc)
    assert same(got, want)


# ---- the masked sums ------------------------------------------------------------------------------------------------------------
class Masked:
    """u, v, w and two mask fields on a backend, a Sampler whose masks are final, the mask words on the host."""

    def __init__(self, be, dtype, nm, shape=SHAPE):
        import torch
        self.be, self.torch = be, torch
        self.g = g = grid(shape, dtype)
        self.G = be.grid(g)
        self.device = torch.device("cpu") if be.name == "emul" else be.dev
        self.h = dict(zip(("u", "v", "w", "m", "mh"), fields(g, 5, seed=11)))
        self.h["mh"] = self.h["mh"] - self.h["mh"].dtype.type(0.45)          # signed like "m"; full and half flags differ
        self.d = {k: torch.from_numpy(a.copy()).to(self.device) for k, a in self.h.items()}
        masks = ("default", "t1", "t2", "t3", "t4")[:nm]
        self.s = s = S.Sampler(be.lib, g, self.G, torch, self.device, masks, stream=lambda: be.stream)
        s.initialize_masks()
        for name, thr in zip(masks[1:], THRESHOLDS):
            s.set_mask_thres(name, self.d["m"], self.d["mh"], None, thr - 0.5, S.PLUS)      # "m" is signed, mean near zero
        s.finalize_masks()
        be.sync()
        self.words = interior(g, s.host_words()[0])
        self.nm = nm

    def bit(self, half):
        """[nmasks][kcells][jmax][imax] of 0. and 1.: in_mask<double> under flag (half 0) or flagh (half 1)."""
        return np.stack([((self.words >> (2*n + half)) & 1).astype(np.float64) for n in range(self.nm)])

    def mean_sums(self, var, half):
        """The restated MEAN sums [nmasks][kcells] over ALL levels."""
        return level_sums(self.bit(half) * interior(self.g, self.h[var]).astype(np.float64), runs16)


_masked = {}


def masked(be, dtype, nm, shape=SHAPE):
    key = (be.name, np.dtype(dtype).name, nm, shape)
    if key not in _masked:
        _masked[key] = Masked(be, dtype, nm, shape)
    return _masked[key]


def inside(g, a, k0, k1):
    """a[..., kcells] with zero outside k0 .. k1-1: what a sums call leaves outside a job's levels."""
    out = np.zeros_like(a)
    out[..., k0:k1] = a[..., k0:k1]
    return out


def stats_sums_are_the_16x16_order(be, dtype, nm, shape):
    m = masked(be, dtype, nm, shape)
    g, d = m.g, m.d
    jobs = [(d["u"], 0, S.MEAN, 0., 0., None), (d["u"], 0, S.GRAD, 0., 0., None), (d["v"], 0, S.MEAN, 0., 0., None),
            (d["w"], 1, S.MEAN, 0., 0., None), (d["u"], 0, S.COUNT, 0., 0., None), (d["u"], 1, S.COUNT, 0., 0., None)]
    _, got = m.s.sums(jobs)
    be.sync()
    got = got.cpu().numpy()
    ks, ke = g.kstart, g.kend
    want = np.zeros_like(got)
    want[0] = inside(g, m.mean_sums("u", 0), ks, ke+1)
    # calc_grad_2nd: in_mask * TF(fld[k] - fld[k-1]) * dzhi[k] under the flag of the OTHER level, the products left to right
    u = interior(g, m.h["u"])
    du = np.zeros(u.shape)
    du[1:] = (u[1:] - u[:-1]).astype(np.float64)
    assert (u[1:] - u[:-1]).dtype == g.np_dtype
    q = m.bit(1) * du
    want[1] = inside(g, level_sums(q * g.dzhi.astype(np.float64)[None, :, None, None], runs16), ks, ke+1)
    want[2] = inside(g, m.mean_sums("v", 0), ks, ke+1)
    want[3] = inside(g, m.mean_sums("w", 1), ks, ke+1)
    want[4] = level_sums(m.bit(0), runs16)                         # calc_nmask: every level of kcells
    want[5] = level_sums(m.bit(1), runs16)
    for n, name in enumerate(("mean u", "grad u", "mean v", "mean w", "count", "counth")):
        assert same(got[n], want[n]), name
    if nm > 1:                                                     # the masks are what they claim to be: nested and not empty
        cnt = want[4][:, ks:ke].sum(axis=1)
        assert np.all(cnt[1:] < cnt[:-1]) and cnt[-1] > 0 and not same(want[4], want[5])


@pytest.mark.parametrize("nm", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_sums_are_the_16x16_order(be, dtype, nm):
    stats_sums_are_the_16x16_order(be, dtype, nm, SHAPE)


@pytest.mark.parametrize("nm", [2, 5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MORE, ids=MORE_IDS)
def test_stats_sums_are_the_16x16_order_over_many_chunks(be, dtype, nm, shape):
    stats_sums_are_the_16x16_order(be, dtype, nm, shape)


def budget_model_sums_are_the_16x16_order_and_the_stats_means(be, dtype, nm, shape):
    m = masked(be, dtype, nm, shape)
    g, d, t = m.g, m.d, m.torch
    got = t.zeros((3, nm, g.kcells), device=m.device, dtype=t.float64)
    scratch = t.zeros((int(be.lib.mhh_budget_2_scratch_elems(m.G, nm)),), device=m.device, dtype=t.float64)
    S.capi.check(be.lib.mhh_budget_2_model_sums(m.G, m.s.mfield.data_ptr(), nm, d["u"].data_ptr(), d["v"].data_ptr(), d["w"].data_ptr(),
                                                got.data_ptr(), scratch.data_ptr(), be.stream), be.lib)
    _, stats = m.s.sums([(d["u"], 0, S.MEAN, 0., 0., None), (d["v"], 0, S.MEAN, 0., 0., None), (d["w"], 1, S.MEAN, 0., 0., None)])
    be.sync()
    got, stats = got.cpu().numpy(), stats.cpu().numpy()
    for n, (var, half) in enumerate((("u", 0), ("v", 0), ("w", 1))):
        assert same(got[n], m.mean_sums(var, half)), var           # calc_mask_mean_profile: every level of kcells
    assert same(got[:, :, g.kstart:g.kend+1], stats[:, :, g.kstart:g.kend+1])


@pytest.mark.parametrize("nm", [1, 2, 3, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_budget_model_sums_are_the_16x16_order_and_the_stats_means(be, dtype, nm):
    budget_model_sums_are_the_16x16_order_and_the_stats_means(be, dtype, nm, SHAPE)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MORE, ids=MORE_IDS)
def test_budget_model_sums_are_the_16x16_order_over_many_chunks(be, dtype, shape):
    budget_model_sums_are_the_16x16_order_and_the_stats_means(be, dtype, 2, shape)
