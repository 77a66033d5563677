"""Field3d_operators on the device (src/field3d_operators.cxx:45-66,132-155): mhh_field_mean_profile and mhh_field_mean_sum.

The reference accumulates in double in loop order; the kernels add the same doubles in another, fixed order. Any summation order
of n doubles is within gamma*sum|x| of the exact sum, gamma = (n-1)u/(1-(n-1)u), u = 2^-53, so the comparison is against
math.fsum with exactly that bound plus one ulp of the result type for the quotient's rounding and the cast: nothing to tune.
Ghost cells in i and j hold 1e30 (a kernel that reads them cannot pass); ghost levels in k hold ordinary values and ARE summed
by the profile, as the reference loops over all of kcells.

Runs on the ``emul`` backend and on the ``hip`` backend (marked gpu)."""
import math

import numpy as np
import pytest

from backends import be  # noqa: F401
from common import DTYPES, same_bits as same
from means_common import SHAPES, grid, fields, gamma, ulp, ptrs, scratch, profiles, sums, profile_bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mean_profile_within_the_summation_bound(be, dtype, shape):
    g = grid(shape, dtype)
    G = be.grid(g)
    host = fields(g, 2)
    dev = [be.arr(a) for a in host]
    got = profiles(be, g, G, dev)
    N = g.itot * g.jtot
    for n in range(2):
        assert got[n].dtype == g.np_dtype
        for k in range(g.kcells):
            ref, bound = profile_bound(host[n][k, g.jstart:g.jend, g.istart:g.iend], N, dtype)
            assert abs(float(got[n][k]) - ref) <= bound, (shape, n, k, float(got[n][k]), ref, bound)
    assert same(be.host(dev[0]), host[0])                       # inputs untouched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mean_sum_within_the_summation_bound(be, dtype, shape):
    g = grid(shape, dtype)
    G = be.grid(g)
    host = fields(g, 2)
    dev = [be.arr(a) for a in host]
    got = sums(be, g, G, dev)
    for n in range(2):
        # x = fl_TF(fld*dz), the product formed in TF as the reference's expression does
        x = host[n][g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend] * g.dz[g.kstart:g.kend, None, None]
        assert x.dtype == g.np_dtype
        xs = [float(v) for v in x.ravel()]
        ref = math.fsum(xs)
        bound = gamma(len(xs)) * math.fsum(abs(v) for v in xs) + ulp(ref, dtype)
        assert abs(float(got[n]) - ref) <= bound, (shape, n, float(got[n]), ref, bound)


def test_a_level_is_split_over_chunks_and_the_last_chunk_is_partial(be):
    """(130, 37, 6): from the scratch size, a level takes two chunks of rows, and the second holds 5 of its 32 rows."""
    g = grid((130, 37, 6), np.float64)
    G = be.grid(g)
    rows = int(be.lib.mhh_field_mean_chunk_rows())
    nchunks = int(be.lib.mhh_field_mean_scratch_elems(G, 1)) // g.kcells
    assert nchunks >= 2 and nchunks == -(-g.jmax // rows)
    assert g.jmax % rows != 0
    assert int(be.lib.mhh_field_mean_scratch_elems(G, 11)) == 11 * g.kcells * nchunks


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_the_same_bits_batched_and_field_by_field(be, dtype):
    g = grid((130, 37, 6), dtype)
    G = be.grid(g)
    host = fields(g, 11)
    dev = [be.arr(a) for a in host]
    p1, p2 = profiles(be, g, G, dev), profiles(be, g, G, dev)
    s1, s2 = sums(be, g, G, dev), sums(be, g, G, dev)
    assert all(same(a, b) for a, b in zip(p1, p2)) and same(s1, s2)
    w1 = scratch(be, g, G, 1)
    for n in range(11):                                          # 11 single-field launches: the same bits as the batch, twice
        for _ in range(2):
            assert same(profiles(be, g, G, [dev[n]], w1)[0], p1[n]), n
            assert same(sums(be, g, G, [dev[n]], w1), s1[n:n+1]), n


def test_refusals(be):
    g = grid((17, 9, 8), np.float64)
    G = be.grid(g)
    dev = [be.arr(a) for a in fields(g, 1)]
    work = scratch(be, g, G, 1)
    out = [be.zeros(g.kcells, np.float64)]
    assert be.lib.mhh_field_mean_profile(G, ptrs(be, dev), 12, ptrs(be, out), be.ptr(work), be.stream) == 1
    assert be.lib.mhh_field_mean_profile(G, ptrs(be, dev), 0, ptrs(be, out), be.ptr(work), be.stream) == 1
    assert be.lib.mhh_field_mean_sum(G, ptrs(be, dev), 1, None, be.ptr(work), be.stream) == 1
    assert not be.host(out[0]).any()
