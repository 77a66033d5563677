"""Shared plumbing of the horizontal-mean tests (tests/test_field_means.py, tests/test_pres_ref.py): the fields, the calls of
mhh_field_mean_profile / mhh_field_mean_sum and the summation bound."""
import ctypes as C
import math

import numpy as np

import backends as B
import common as cm

SHAPES = [(70, 9, 10), (20, 1, 12), (130, 37, 6)]
# The shapes of tests/test_reduction_order.py, by the level tiling (level_reduce.h) of their chunks of 32 rows; the classes are
# asserted from the headers by tests/test_launch_geometry.py::test_matrix_reaches_every_geometry_class:
LEVEL_SHAPES = [(130, 37, 4),     # 2 chunks: sr 1, several k-segments (the class of jtot = 64 and 128)
                (6, 260, 5),      # 9 chunks: sr 1, 9 strips, a last round of units with idle slots
                (6, 250, 3),      # 8 chunks: sr 1, 8 strips (the class of jtot = 256)
                (6, 484, 3),      # 16 chunks: sr 2, 8 strips (the class of jtot = 512)
                (6, 520, 3),      # 17 chunks: sr 2, the last strip cut
                (6, 780, 2),      # 25 chunks: sr 3, the last strip cut
                (6, 1000, 2)]     # 32 chunks: sr 4, 8 strips (the class of jtot = 1024)
U = 2.0**-53


def grid(shape, dtype):
    return cm.grid_2nd(*shape, gc=(2, 2, 1), dtype=dtype)


def fields(g, nf, seed=5):
    """nf fields: even ones U[0,1), odd ones signed with a mean near zero; 1e30 in the i and j ghost cells."""
    rs = np.random.RandomState(seed)
    out = []
    for n in range(nf):
        a = np.full(g.shape3, 1e30, dtype=g.np_dtype)
        x = rs.random_sample((g.kcells, g.jmax, g.imax))
        if n % 2:
            x = x - 0.5
        a[:, g.jstart:g.jend, g.istart:g.iend] = x.astype(g.np_dtype)
        out.append(a)
    return out


def gamma(n):
    return (n - 1) * U / (1 - (n - 1) * U)


def ulp(x, dtype):
    return float(np.spacing(np.abs(dtype(x)))) if x != 0 else float(np.finfo(dtype).tiny)


def ptrs(be, arrays):
    return (C.c_void_p * len(arrays))(*[be.ptr(a).value for a in arrays])


def scratch(be, g, G, nf):
    n = int(be.lib.mhh_field_mean_scratch_elems(G, nf))
    assert n == nf * g.kcells * -(-g.jmax // int(be.lib.mhh_field_mean_chunk_rows()))
    return be.zeros(n, np.float64)


def profiles(be, g, G, dev, work=None):
    nf = len(dev)
    work = scratch(be, g, G, nf) if work is None else work
    out = [be.zeros(g.kcells, g.np_dtype) for _ in range(nf)]
    B.ok(be, be.lib.mhh_field_mean_profile(G, ptrs(be, dev), nf, ptrs(be, out), be.ptr(work), be.stream))
    return [be.host(o) for o in out]


def sums(be, g, G, dev, work=None):
    nf = len(dev)
    work = scratch(be, g, G, nf) if work is None else work
    out = be.zeros(nf, np.float64)
    B.ok(be, be.lib.mhh_field_mean_sum(G, ptrs(be, dev), nf, be.ptr(out), be.ptr(work), be.stream))
    return be.host(out)


def profile_bound(x, N, dtype):
    """(fsum/N, bound) of one level's interior cells x."""
    xs = [float(v) for v in x.ravel()]
    ref = math.fsum(xs) / N
    return ref, gamma(len(xs)) * math.fsum(abs(v) for v in xs) / N + ulp(ref, dtype)
