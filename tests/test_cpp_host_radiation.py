"""Radiation_gcss through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_radiation.cpp runs exec and
get_radiation_field on 64 x 8 x 32 from inputs this test writes, and gives the bits of the same calls made through the Python driver
(HotPath("dycoms", ..., radiation=Gcss(...))). Built here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import common as cm
import hostprog
from common import same_bits as same

GRID = (64, 8, 32)
DAY = 160.5


def test_radiation_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_radiation")


@pytest.mark.gpu
def test_cpp_host_radiation_gives_the_bits_of_the_python_driver():
    from microhh_amd.model import CASES, HotPath
    from microhh_amd.radiation import Gcss, dycoms_profiles
    from microhh_amd.thermo import Moist
    c = CASES["dycoms"]
    thl0, qt0 = dycoms_profiles((np.arange(GRID[2]) + 0.5)*c["size"][2]/GRID[2])
    hp = HotPath("dycoms", *GRID, dt=2., nscalars=2, thermo=Moist(c["pbot"], thl0=thl0, qt0=qt0),
                 radiation=Gcss(c["xka"], c["fr0"], c["fr1"], c["div"], c["lat"], c["lon"], DAY))
    g, th, rad = hp.grid, hp.thermo, hp.radiation
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)          # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [host(hp.s[0]), host(hp.s[1]), host(hp.st[0]), host(th.tab["pref"]), host(th.tab["exnref"]), host(hp.rhoref)] +
                               [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi])
        before = host(hp.st[0])
        rad.exec()
        f = rad.fields()
        th.check()
        want = [host(hp.st[0]), host(f["lflx"]), host(f["sflx"])]
        mu = rad.mu
        hp.close()
        hostprog.run(hostprog.compile("host_radiation"), fin, fout, *GRID, *[repr(c[k]) for k in ("xka", "fr0", "fr1", "div", "lat", "lon")], repr(DAY))
        got = hostprog.read_doubles(fout)
    n3 = int(np.prod(g.shape3))
    assert got.size == 3*n3 + 1 and not same(want[0], before) and float(want[2].max()) > 100.
    for k, (name, w) in enumerate(zip(["thlt", "lflx", "sflx"], want)):
        a = got[k*n3:(k+1)*n3].reshape(g.shape3)
        assert same(np.ascontiguousarray(a), np.ascontiguousarray(w)), (name, cm.ulp_diff(a, w))
    assert got[-1] == mu
