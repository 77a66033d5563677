"""Boundary_outflow through the C++ host layer (microhh_amd/host/mhh_host.h): tests/cpp/host_outflow.cpp runs the member of the
reference's signature, Boundary_outflow::exec(data, inflow_prof), and the head of Model::exec -- the cyclic fills, exec_all of two
open scalars (src/model.cxx:347), advec->exec -- on a 24 x 20 x 16 grid, and gives the bits of the same calls made through the Python
binding. Built here with hipcc into a temporary directory."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import backends as B
import common as cm
import hostprog
import outflow_ref as R
from common import same_bits as same
from microhh_amd import capi
from microhh_amd.grid import ADVEC_2I5

SHAPE = (24, 20, 16)


def test_outflow_host_program_compiles():
    """not gpu: the program and the host classes it drives build against the library."""
    hostprog.compile("host_outflow")


@pytest.mark.gpu
def test_cpp_boundary_outflow_gives_the_bits_of_the_python_calls():
    be = B.get("hip")
    g = cm.grid_2nd(*SHAPE, gc=(3, 3, 1))
    rs = np.random.RandomState(31)
    host = {n: np.ascontiguousarray(rs.random_sample(g.shape3)*2. - 0.5) for n in ("u", "v", "w", "s0", "s1", "s2")}
    rho, rhoh = 1.2 - 0.01*np.arange(g.kcells), 1.205 - 0.01*np.arange(g.kcells)
    p1, p2 = rs.random_sample(g.ktot), rs.random_sample(g.ktot) + 1.
    # the Python calls
    G = be.grid(g)
    dev = {n: be.arr(a) for n, a in host.items()}
    tend = {n: be.zeros(g.shape3, np.float64) for n in host}
    t1, t2 = be.arr(R.table_of(g, p1)), be.arr(R.table_of(g, p2))
    copy = be.arr(host["s0"])
    rc, _ = R.lib_exec(be, g, [copy], [t1], (R.IN, R.OUT, R.OUT, R.IN), R.ALL)
    assert rc == 0
    every = [dev[n] for n in ("u", "v", "w", "s0", "s1", "s2")]
    B.ok(be, be.lib.mhh_boundary_cyclic_n(G, (C.c_void_p * 6)(*[be.ptr(a).value for a in every]), 6, cm.EDGE_BOTH, be.stream))
    rc, launches = R.lib_exec(be, g, [dev["s1"], dev["s2"]], [t1, t2], R.JAENSCHWALDE, R.ALL)
    assert rc == 0 and launches == 2
    f = capi.MhhFields(); f.nscalars = 3
    for n in ("u", "v", "w"):
        setattr(f, n, be.ptr(dev[n]).value); setattr(f, n + "t", be.ptr(tend[n]).value)
    for n in range(3):
        f.s[n], f.st[n] = be.ptr(dev["s%d" % n]).value, be.ptr(tend["s%d" % n]).value
    rho_d, rhoh_d = be.arr(rho), be.arr(rhoh)
    f.rhoref, f.rhorefh = be.ptr(rho_d).value, be.ptr(rhoh_d).value
    B.ok(be, be.lib.mhh_advec_exec(G, ADVEC_2I5, C.byref(f), be.stream))
    be.sync()
    want = [be.host(copy)] + [be.host(dev["s%d" % n]) for n in range(3)] + [be.host(tend["s%d" % n]) for n in range(3)]
    assert not same(want[0], host["s0"]) and not same(want[2], want[1]) and np.abs(want[5]).max() > 0
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi] + [host[n] for n in ("u", "v", "w", "s0", "s1", "s2")] + [rho, rhoh, p1, p2])
        hostprog.run(hostprog.compile("host_outflow"), fin, fout, *SHAPE, *[repr(float(x)) for x in (g.xsize, g.ysize, g.zsize)])
        out = hostprog.read_doubles(fout)
    got = out.reshape((7,) + tuple(g.shape3))
    for n, nm in enumerate(("exec(s0)", "s0", "s1", "s2", "st0", "st1", "st2")):
        assert same(got[n], want[n]), (nm, cm.ulp_diff(got[n], want[n]))


# ---- both calls of Model::exec, with an immersed boundary; plain and through Substep_slab on a one-rank RCCL communicator ----------
IB_GRID = (16, 16, 16)
N_IDW, SBOT = 5, 0.1


def test_outflow_ib_host_program_compiles():
    """not gpu: Substep_slab::set_outflow / cyclic_outflow and the sequence with Immersed_boundary build against the library."""
    hostprog.compile("host_outflow_ib", libs=("rccl",))


@pytest.mark.gpu
@pytest.mark.parametrize("slab", [0, 1], ids=["plain", "substep-slab-rccl"])
def test_cpp_model_sequence_with_ib_makes_both_outflow_calls(slab):
    from microhh_amd import ib
    from microhh_amd.model import CASES, HotPath
    from microhh_amd.outflow import Outflow
    g = cm.grid_2nd(*IB_GRID)
    prof = 300. + 0.05*np.arange(g.ktot) + 0.2*np.cos(np.arange(g.ktot))
    dem = ib.sine_dem(IB_GRID[0], IB_GRID[1], *CASES["drycblles"]["size"], 0.22)
    hp = HotPath("drycblles", *IB_GRID, ib=ib.Dem(dem, N_IDW, sbcbot="flux", sbot=(SBOT,)), outflow=Outflow({0: prof}))
    g = hp.grid
    host = lambda t: t.detach().cpu().numpy().copy()      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, (host(hp.u), host(hp.v), host(hp.w), host(hp.s[0]), hp.ib.dem_h, g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi, prof))
        hostprog.run(hostprog.compile("host_outflow_ib", libs=("rccl",)), fin, fout, *IB_GRID, N_IDW, repr(SBOT), repr(hp.cfg["visc"]), slab)
        got = hostprog.read_doubles(fout).reshape((2,) + tuple(g.shape3))
    # the Python driver: the four calls of step() in front of the RHS (src/model.cxx:346-347, :380-383)
    hp.cyclic_prognostic(); hp.outflow_bcs(); hp.sync()
    first = host(hp.s[0])
    hp.ib.exec_scalars(); hp.sync()
    between = host(hp.s[0])
    hp.outflow_bcs(); hp.sync()
    second = host(hp.s[0])
    hp.close()
    assert same(got[0], first), cm.ulp_diff(got[0], first)
    assert same(got[1], second), cm.ulp_diff(got[1], second)
    assert not same(second, between) and not same(second, first)          # the second call does something: without it th differs
