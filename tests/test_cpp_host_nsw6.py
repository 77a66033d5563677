"""Microphys_nsw6 and Limiter through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_nsw6.cpp runs exec, Limiter::exec
and get_time_limit on 64 x 8 x 32 from inputs this test writes, and gives the bits of the same calls made through the Python driver
(HotPath("rcemip", ..., micro=Nsw6)). Built here with hipcc into a temporary directory."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
from common import same_bits as same

CPP = os.path.join(cm.ROOT, "tests", "cpp")
LIBDIR = os.path.join(cm.ROOT, "microhh_amd")
GRID = (64, 8, 32)
PBOT, NC0, DT, SUBDT, IDT = 101480., 100.e6, 6., 2., 6000000000


def _compile(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", out, os.path.join(CPP, "host_nsw6.cpp"),
                    "-L" + LIBDIR, "-lmhh_hip", "-Wl,-rpath," + LIBDIR], check=True)


def test_nsw6_host_program_compiles():
    """not gpu: the program and the host classes it drives build against the library."""
    with tempfile.TemporaryDirectory() as tmp:
        _compile(os.path.join(tmp, "host_nsw6"))


@pytest.mark.gpu
def test_cpp_host_nsw6_gives_the_bits_of_the_python_driver():
    from microhh_amd.microphys import Nsw6
    from microhh_amd.model import HotPath
    from microhh_amd.thermo import Moist
    hp = HotPath("rcemip", *GRID, dt=SUBDT, thermo=Moist(PBOT), micro=Nsw6(NC0, dt=DT))
    g, th, mi = hp.grid, hp.thermo, hp.micro
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)          # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("host_nsw6", "in.bin", "out.bin"))
        _compile(exe)
        with open(fin, "wb") as fh:
            for a in ([host(t) for t in hp.s] + [host(t) for t in hp.st] + [host(th.tab["pref"]), host(th.tab["exnref"]), host(hp.rhoref)] +
                      [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi]):
                np.ascontiguousarray(a, dtype=np.float64).tofile(fh)
        mi.exec(); mi.limit()
        limit = mi.time_limit(IDT, DT)
        th.check()
        want = [host(t) for t in hp.st] + [host(mi.rain_rate()), host(mi.snow_rate()), host(mi.graupel_rate())]
        hp.close()
        r = subprocess.run([exe, fin, fout, *[str(n) for n in GRID], repr(NC0), repr(DT), repr(SUBDT), str(IDT)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "host_nsw6 ok" in r.stdout, r.stdout + r.stderr
        got = np.fromfile(fout, dtype=np.float64)
    n3, n2 = int(np.prod(g.shape3)), int(np.prod(g.shape2))
    parts = [got[k*n3:(k+1)*n3].reshape(g.shape3) for k in range(5)] + [got[5*n3 + k*n2:5*n3 + (k+1)*n2].reshape(g.shape2) for k in range(3)]
    assert max(float(w.max()) for w in want[5:]) > 0 and got.size == 5*n3 + 3*n2 + 1
    for name, a, w in zip(["thlt", "qtt", "qrt", "qst", "qgt", "rr_bot", "rs_bot", "rg_bot"], parts, want):
        assert same(np.ascontiguousarray(a), np.ascontiguousarray(w)), (name, cm.ulp_diff(a, w))
    assert int(got[-1]) == limit
