"""Buffer and Force through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_force.cpp runs Buffer::exec and
Force::exec (the sponge with fixed profiles, geostrophic wind + Coriolis, large-scale sources) on (17, 9, 8) from inputs this test
writes, and gives the bits of the same calls made through the Python binding. Built here with hipcc into a temporary directory."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import backends as B
import common as cm
import hostprog
from common import same_bits as same
from microhh_amd import capi, forcing

NAMES = ["u", "v", "w", "s0", "s1"]


def test_force_host_program_compiles():
    """not gpu: the program and the host classes it drives build against the library."""
    hostprog.compile("host_force")


@pytest.mark.gpu
def test_cpp_host_buffer_and_force_give_the_bits_of_the_python_calls():
    be = B.get("hip")
    g = cm.grid_2nd(17, 9, 8, gc=(1, 1, 1))
    c = cm.Case(g, nscalars=2, periodic=True)
    rs = np.random.RandomState(9)
    profs = [rs.random_sample(g.kcells) - 0.3 for _ in range(9)]        # abuf u v w s0 s1, ug, vg, ls_u, ls_s1
    k = g.kstart + (2 * g.kmax) // 3
    zstart, sigma, beta, fc, utrans, vtrans = 0.5 * (float(g.zh[k]) + float(g.z[k])), 2., 2.3, 1.39e-4, 0.13, -0.21
    # the Python calls
    d = B.DevCase(be, c); f = d.fields()
    keep = [be.arr(p) for p in profs]
    sg, sgh = (be.arr(t) for t in forcing.sigma_tables(be.lib, g, zstart, sigma, beta))
    b = capi.MhhBufferParams(); b.swbuffer = 1
    b.bufferkstart, b.bufferkstarth = forcing.buffer_kstart(g, zstart)
    b.sigma, b.sigmah = be.ptr(sg).value, be.ptr(sgh).value
    b.abuf_u, b.abuf_v, b.abuf_w = (be.ptr(t).value for t in keep[:3])
    b.abuf_s[0], b.abuf_s[1] = be.ptr(keep[3]).value, be.ptr(keep[4]).value
    p = capi.MhhForceParams(); p.swlspres, p.order, p.fc, p.utrans, p.vtrans = 3, 2, fc, utrans, vtrans
    p.ug, p.vg = be.ptr(keep[5]).value, be.ptr(keep[6]).value
    p.swls = 1; p.ls_u = be.ptr(keep[7]).value; p.ls_s[1] = be.ptr(keep[8]).value
    B.ok(be, be.lib.mhh_buffer_exec(d.G, C.byref(f), C.byref(b), be.stream))
    B.ok(be, be.lib.mhh_force_exec(d.G, C.byref(f), C.byref(p), be.stream))
    want = [be.host(x) for x in (d.ut, d.vt, d.wt, d.st[0], d.st[1])]
    assert not same(want[0], c.ut) and not same(want[2], c.wt)
    # the C++ program on the same inputs
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi, c.u, c.v, c.w, c.s[0], c.s[1], c.ut, c.vt, c.wt, c.st[0], c.st[1]] + profs)
        out = hostprog.run(hostprog.compile("host_force"), fin, fout, "17", "9", "8",
                           *[repr(float(x)) for x in (g.xsize, g.ysize, g.zsize, zstart, sigma, beta, fc, utrans, vtrans)])
        assert "bufferkstart %d bufferkstarth %d" % (b.bufferkstart, b.bufferkstarth) in out
        got = hostprog.read_doubles(fout).reshape((5,) + tuple(g.shape3))
    for n, a, w in zip(NAMES, got, want):
        assert same(a, w), (n, cm.ulp_diff(a, w))
