"""Source and Decay through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_source.cpp runs Decay::exec, two Source
objects (the sources without a profile; the profile sources, as the reference's one switch has it), an update of every plain source
and a second exec on the 24 x 20 x 16 grid of tests/source_ref.py, and gives the bits of the same calls made through the Python
binding. Built here with hipcc into a temporary directory."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import backends as B
import common as cm
import hostprog
import source_ref as R
from common import same_bits as same
from microhh_amd import capi
from microhh_amd.source import Handle


def test_source_host_program_compiles():
    """not gpu: the program and the host classes it drives build against the library."""
    hostprog.compile("host_source")


def _row(s):
    p = s.get("profile_index")
    return [s["scalar"], float(bool(s.get("swvmr", False))), -1 if p is None else p] + [s.get(k, 0.) for k in
            ("x0", "y0", "z0", "sigma_x", "sigma_y", "sigma_z", "line_x", "line_y", "line_z")] + [s.get("strength", 1.)]


@pytest.mark.gpu
def test_cpp_host_source_and_decay_give_the_bits_of_the_python_calls():
    be = B.get("hip")
    case = R.CASES[0]
    g, inp = R.grid_of(case), R.inputs(case)
    src = R.sources_of(case[0])
    plain = [s for s in src if s.get("profile_index") is None]
    prof = [s for s in src if s.get("profile_index") is not None]
    profiles, rho = R.profiles_of(g), R.rhoref_of(g)
    s0 = [inp.field("s", n) for n in range(3)]
    st0 = [inp.field("st0", n) for n in range(3)]
    # the Python calls
    st, s = [be.arr(a) for a in st0], [be.arr(a) for a in s0]
    f = capi.MhhFields(); f.nscalars = 3
    for n in range(3):
        f.s[n], f.st[n] = be.ptr(s[n]).value, be.ptr(st[n]).value
    p = capi.MhhDecayParams()
    p.exponential[0], p.timescale[0], p.exponential[1], p.timescale[1] = 1, 600., 1, 2.5
    G = be.grid(g)
    B.ok(be, be.lib.mhh_decay_exec(G, C.byref(f), C.byref(p), R.DT_SUB, be.stream))
    ha = Handle(be.lib, g, plain, None, rho, be.stream)
    hb = Handle(be.lib, g, prof, profiles, rho, be.stream)
    ha.exec(G, f, be.stream); hb.exec(G, f, be.stream)
    ha.update(None, x0=[q["x0"] + 137. for q in plain], y0=[q["y0"] for q in plain], z0=[q["z0"] for q in plain],
              strength=[2.*q["strength"] for q in plain], stream=be.stream)
    ha.exec(G, f, be.stream)
    be.sync()
    want = [be.host(a) for a in st]
    norms = [ha.norm(n) for n in range(ha.n)]
    ha.close(); hb.close()
    assert not any(same(a, b) for a, b in zip(want, st0))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi] + s0 + st0 + [rho, profiles] + [np.array(_row(q)) for q in plain + prof])
        hostprog.run(hostprog.compile("host_source"), fin, fout, *case[0], *[repr(float(x)) for x in (g.xsize, g.ysize, g.zsize)],
                     len(plain), len(prof), repr(R.DT_SUB))
        out = hostprog.read_doubles(fout)
    n3 = int(np.prod(g.shape3))
    got = out[:3*n3].reshape((3,) + tuple(g.shape3))
    for n in range(3):
        assert same(got[n], want[n]), (n, cm.ulp_diff(got[n], want[n]))
    assert same(out[3*n3:], np.array(norms))
