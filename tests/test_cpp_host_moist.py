"""Thermo_moist through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_moist.cpp runs create_basestate, the means,
exec (the base state on the device and the buoyancy tendency) and get_thermo_field("ql") on 32 x 8 x 24 from inputs this test writes,
and gives the bits of the same calls made through the Python driver (HotPath with thermo=Moist). Built here with hipcc into a
temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import common as cm
import hostprog
from common import same_bits as same

GRID = (32, 8, 24)
PBOT = 101500.


def test_moist_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_moist")


@pytest.mark.gpu
def test_cpp_host_thermo_moist_gives_the_bits_of_the_python_driver():
    from microhh_amd import thermo
    from microhh_amd.model import HotPath
    hp = HotPath("bomex", *GRID, dt=0.37, thermo=thermo.Moist(PBOT))
    g, th = hp.grid, hp.thermo
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)          # noqa: E731
    thl0, qt0 = thermo.bomex_profiles(g.z[g.kstart:g.kend])
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, (host(hp.s[0]), host(hp.s[1]), host(hp.wt), thl0, qt0, g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi))
        th.means(); hp.thermo_moist()
        ql = th.field("ql")
        th.check()
        want = [host(hp.wt), host(ql)] + [host(th.tab[n]) for n in thermo.BASE_STATE]
        hp.close()
        hostprog.run(hostprog.compile("host_moist"), fin, fout, *GRID, repr(PBOT))
        got = hostprog.read_doubles(fout)
    n3 = int(np.prod(g.shape3))
    parts = [got[:n3].reshape(g.shape3), got[n3:2*n3].reshape(g.shape3)] + [got[2*n3 + k*g.kcells:2*n3 + (k+1)*g.kcells] for k in range(8)]
    assert float(want[1].max()) > 0
    for name, a, w in zip(["wt", "ql"] + list(thermo.BASE_STATE), parts, want):
        assert same(np.ascontiguousarray(a), np.ascontiguousarray(w)), (name, cm.ulp_diff(a, w))
