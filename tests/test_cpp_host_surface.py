"""Boundary_surface through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_surface.cpp runs init_surface,
set_values, init_solver and two exec calls -- the fused call, and the slab sequence with the local wrap as its exchange, which must
agree -- on (17, 9, 8) from inputs this test writes, and gives the bits of the same calls made through the Python binding. Built
here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import backends as B
import common as cm
import hostprog
import surface_ref as S
from common import same_bits as same

NAMES = ["dutot", "ustar", "obuk", "ufluxbot", "vfluxbot", "ugradbot", "vgradbot", "sbot0", "sgradbot0", "dudz", "dvdz", "dbdz", "nobuk"]


def test_surface_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_surface")


@pytest.mark.gpu
def test_cpp_host_surface_layer_gives_the_bits_of_the_python_calls():
    be = B.get("hip")
    case = S.SurfCase("flux", S.SHAPES[1], np.float64)
    g, inp = case.g, case.inputs()
    inp["sfluxbot0"][:] = 0.07                                     # set_bc fills a uniform flux
    d = S.DevSurf(be, case, inp, case.state())
    d.fused(); d.fused()
    want = d.outputs()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [be.host(d.a[k]) for k in ("u", "v", "s0")])
        hostprog.run(hostprog.compile("host_surface"), fin, fout, g.itot, g.jtot, g.ktot,
                     *[repr(float(x)) for x in (S.zsl_of(g), S.UBOT, S.VBOT, 0.07, S.Z0M, S.THREF, S.THREFH)])
        got = hostprog.read_doubles(fout).reshape((len(NAMES),) + tuple(g.shape2))
    core = (slice(g.jstart, g.jend), slice(g.istart, g.iend))
    for n, a in zip(NAMES, got):
        w = want[n].astype(np.float64)
        sel = core if n in ("dudz", "dvdz", "dbdz") else slice(None)             # written on the interior only
        assert same(np.ascontiguousarray(a[sel]), np.ascontiguousarray(w[sel])), (n, cm.ulp_diff(a[sel], w[sel]))
