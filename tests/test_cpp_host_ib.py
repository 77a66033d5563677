"""The immersed boundary through the C++ host layer (Immersed_boundary<TF> of microhh_amd/host/mhh_host.h): tests/cpp/host_ib.cpp
runs create, prepare_device, exec_scalars, exec_momentum, get_mask and the wall flux on 16 x 8 x 16 from inputs this test writes, and
its fields, its mask (and so the mask's profile) and its flux plane are the ones the Python driver (microhh_amd.ib.Dem behind a
HotPath) leaves from the same inputs, byte for byte. Built here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import hostprog

GRID = (16, 8, 16)
N_IDW, SBOT = 5, 0.1


def test_ib_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_ib")


@pytest.mark.gpu
@pytest.mark.parametrize("sbcbot", ["flux", "dirichlet"])
def test_cpp_host_ib_leaves_the_fields_of_the_python_driver(sbcbot):
    from microhh_amd import ib
    from microhh_amd.model import CASES, HotPath
    dem = ib.sine_dem(GRID[0], GRID[1], *CASES["drycblles"]["size"], 0.22)          # the steep terrain: the side loops of the flux run
    hp = HotPath("drycblles", *GRID, ib=ib.Dem(dem, N_IDW, sbcbot=sbcbot, sbot=(SBOT,)))
    g = hp.grid
    host = lambda t: t.detach().cpu().numpy().copy()      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, (host(hp.u), host(hp.v), host(hp.w), host(hp.s[0]), hp.ib.dem_h, g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi))
        hostprog.run(hostprog.compile("host_ib"), fin, fout, *GRID, N_IDW, ib.BC[sbcbot], repr(SBOT), repr(hp.cfg["visc"]))
        got = hostprog.read_doubles(fout)
    before = host(hp.s[0])
    hp.ib.exec_scalars(); hp.ib.exec_momentum()
    flux = hp.ib.fluxbot(0)
    hp.sync()
    assert not np.array_equal(before, host(hp.s[0]))
    n3, n2 = g.ncells, g.ijcells
    want = [host(hp.u), host(hp.v), host(hp.w), host(hp.s[0]), host(hp.ib.mask), host(hp.ib.maskh)]
    for n, a in enumerate(want):
        assert np.array_equal(got[n*n3:(n+1)*n3].view(np.uint8), a.reshape(-1).view(np.uint8)), n
    mask = got[4*n3:5*n3].reshape(g.shape3)
    assert np.array_equal(mask.sum(axis=(1, 2)), host(hp.ib.mask).sum(axis=(1, 2))) and 0 < mask[g.interior].mean() < 1       # the mask's profile
    interior = (slice(g.jstart, g.jend), slice(g.istart, g.iend))
    assert np.array_equal(got[6*n3:6*n3+n2].reshape(g.shape2)[interior].view(np.uint8), np.ascontiguousarray(host(flux)[interior]).view(np.uint8))
    assert [int(x) for x in got[6*n3+n2:]] == [hp.ib.ghost[n]["nghost"] for n in ("u", "v", "w", "s")]
    hp.close()
