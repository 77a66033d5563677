"""Cross through the C++ host layer (Cross_sampler<TF> of microhh_amd/host/mhh_host.h): tests/cpp/host_cross.cpp writes the sections
of u, w, th, thlngrad and the planes thpath, thfluxbot, thbase, thtop on 32 x 8 x 16 from inputs this test writes, and its files are
the ones the Python driver (microhh_amd.cross.Cross behind a HotPath) writes from the same fields, byte for byte. Built here with
hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import hostprog

GRID = (32, 8, 16)
IOTIME, UTRANS, THRESHOLD = 3600, 2.5, 301.9125      # the threshold: the mean of th on level 8, so that the base varies over the columns
LOC = dict(xy=[0., 610., 1200.], xz=[0., 1700., 3200.], yz=[1650., 3200.])


def test_cross_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_cross")


@pytest.mark.gpu
def test_cpp_host_cross_writes_the_files_of_the_python_driver():
    import torch
    from microhh_amd import capi, fieldio
    from microhh_amd.cross import Cross
    from microhh_amd.model import HotPath
    with tempfile.TemporaryDirectory() as tmp:
        pydir, cppdir = os.path.join(tmp, "py"), os.path.join(tmp, "cpp")
        os.mkdir(pydir); os.mkdir(cppdir)
        hp = HotPath("drycblles", *GRID, cross=Cross(["u", "w", "th", "thlngrad", "thpath", "thfluxbot"], path=pydir, utrans=UTRANS, **LOC))
        g, lib = hp.grid, capi.lib()
        hp.cross.sample(IOTIME)
        for name, up in (("thbase", 1), ("thtop", 0)):             # the threshold heights of th: the entry point, then the writer
            out = torch.zeros((g.jmax, g.imax), device=hp.device, dtype=hp.td)
            capi.check(lib.mhh_cross_height_threshold(hp.G, hp.s[0].data_ptr(), THRESHOLD, up, out.data_ptr(), hp.stream), lib)
            hp.sync()
            fieldio.save_xy_slice(fieldio.cross_filename(pydir, name, "xy", None, IOTIME), out.cpu().numpy(), g)
        base = fieldio.load_xy_slice(fieldio.cross_filename(pydir, "thbase", "xy", None, IOTIME), g)
        assert (base > 0).any() and len(np.unique(base)) > 1
        fin = os.path.join(tmp, "in.bin")
        host = lambda t: t.detach().cpu().numpy()      # noqa: E731
        hostprog.write_doubles(fin, (host(hp.u), host(hp.w), host(hp.s[0]), host(hp.surf["s_fluxbot"]), host(hp.rhoref), g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi))
        hostprog.run(hostprog.compile("host_cross"), fin, cppdir, *GRID, IOTIME, repr(UTRANS), repr(THRESHOLD))
        hp.close()
        want = sorted(os.listdir(pydir))
        assert sorted(os.listdir(cppdir)) == want and len(want) == 4*8 + 4
        for f in want:
            assert open(os.path.join(cppdir, f), "rb").read() == open(os.path.join(pydir, f), "rb").read(), f
