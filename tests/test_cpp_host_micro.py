"""Microphys_2mom_warm and Limiter through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_micro.cpp runs exec,
Limiter::exec and get_time_limit on 64 x 8 x 32 from inputs this test writes, and gives the bits of the same calls made through the
Python driver (HotPath("rico", ..., micro=Warm2mom)). Built here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import common as cm
import hostprog
from common import same_bits as same

GRID = (64, 8, 32)
PBOT, NC0, DT, SUBDT, IDT = 101540., 70.e6, 6., 2., 6000000000


def test_micro_host_program_compiles():
    """not gpu: the program and the host classes it drives build against the library."""
    hostprog.compile("host_micro")


@pytest.mark.gpu
def test_cpp_host_microphysics_gives_the_bits_of_the_python_driver():
    from microhh_amd.microphys import Warm2mom
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    hp = HotPath("rico", *GRID, dt=SUBDT, thermo=Moist(PBOT), micro=Warm2mom(NC0, dt=DT))
    g, th, mi = hp.grid, hp.thermo, hp.micro
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)          # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [host(t) for t in hp.s] + [host(t) for t in hp.st] + [host(th.tab["pref"]), host(th.tab["exnref"]), host(hp.rhoref)] +
                               [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi])
        mi.exec(); mi.limit()
        limit = mi.time_limit(IDT, DT)
        th.check()
        want = [host(hp.s[2]), host(hp.s[3])] + [host(t) for t in hp.st] + [host(mi.rain_rate())]
        hp.close()
        hostprog.run(hostprog.compile("host_micro"), fin, fout, *GRID, repr(NC0), repr(DT), repr(SUBDT), IDT)
        got = hostprog.read_doubles(fout)
    n3, n2 = int(np.prod(g.shape3)), int(np.prod(g.shape2))
    parts = [got[k*n3:(k+1)*n3].reshape(g.shape3) for k in range(6)] + [got[6*n3:6*n3+n2].reshape(g.shape2)]
    assert float(want[6].max()) > 0 and got.size == 6*n3 + n2 + 1
    for name, a, w in zip(["qr", "nr", "thlt", "qtt", "qrt", "nrt", "rr_bot"], parts, want):
        assert same(np.ascontiguousarray(a), np.ascontiguousarray(w)), (name, cm.ulp_diff(a, w))
    assert int(got[-1]) == limit
