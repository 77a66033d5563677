"""Budget_2 through the C++ host layer (Budget_2_sampler<TF> of microhh_amd/host/mhh_host.h): tests/cpp/host_budget.cpp runs the
masks of a Stats_sampler and exec_stats with every group on 32 x 8 x 16 from inputs this test writes, and gives the bits of the same
calls made through the Python driver (microhh_amd.budget.Budget2Sampler). Built here with hipcc into a temporary directory."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import common as cm
import stats_ref as R
from microhh_amd import budget as BU
from microhh_amd import stats as S
from microhh_amd.grid import DIFF_SMAG2, Grid

CPP = os.path.join(cm.ROOT, "tests", "cpp")
LIBDIR = os.path.join(cm.ROOT, "microhh_amd")
GRID = (32, 8, 16)
UTRANS, VTRANS, FC = 1.5, -0.5, 1.e-4
MASKS = ("default", "wpos", "wneg")
ALL = 0x7ff


def _compile(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", out, os.path.join(CPP, "host_budget.cpp"),
                    "-L" + LIBDIR, "-lmhh_hip", "-Wl,-rpath," + LIBDIR], check=True)


def test_budget_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    with tempfile.TemporaryDirectory() as tmp:
        _compile(os.path.join(tmp, "host_budget"))


@pytest.mark.gpu
def test_cpp_host_budget_gives_the_bits_of_the_python_driver():
    import torch
    from microhh_amd import capi
    g = Grid(*GRID, 3200., 3200., 1200., order=2, igc=3, jgc=3, kgc=1)
    rs = np.random.RandomState(47)
    f3 = {n: R.cyclic(rs.random_sample(g.shape3) - 0.5, g) for n in ("u", "v", "w", "p", "b")}
    f3["evisc"] = R.cyclic(0.05 + rs.random_sample(g.shape3), g)
    f2 = {n: rs.random_sample(g.shape2) - 0.5 for n in ("u_fluxbot", "v_fluxbot")}
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in {**f3, **f2}.items()}
    sm = S.Sampler(capi.lib(), g, g.device_struct(dev), torch, dev, MASKS, stream=lambda: None)
    sm.initialize_masks()
    sm.set_mask_thres("wpos", d["w"], d["w"], None, 0., S.PLUS)
    sm.set_mask_thres("wneg", d["w"], d["w"], None, 0., S.MIN)
    sm.finalize_masks()
    bs = BU.Budget2Sampler(sm)
    model, means = bs.model_profiles(d["u"], d["v"], d["w"]), bs.mean_profiles(d["b"], d["p"])
    want = bs.profiles(bs.desc(ALL, d, model, means, utrans=UTRANS, vtrans=VTRANS, fc=FC, diff_scheme=DIFF_SMAG2))
    torch.cuda.synchronize()
    want, model = want.cpu().numpy(), model.cpu().numpy()
    names = bs.names(ALL)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("host_budget", "in.bin", "out.bin"))
        _compile(exe)
        with open(fin, "wb") as fh:
            for x in [f3[n] for n in ("u", "v", "w", "p", "evisc", "b")] + [f2["u_fluxbot"], f2["v_fluxbot"], g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi]:
                np.ascontiguousarray(x, dtype=np.float64).tofile(fh)
        r = subprocess.run([exe, fin, fout, *[str(n) for n in GRID], repr(UTRANS), repr(VTRANS), repr(FC)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "host_budget ok" in r.stdout, r.stdout + r.stderr
        got = np.fromfile(fout, dtype=np.float64)
    kc = g.kcells
    per = (3 + len(names))*kc
    assert got.size == len(MASKS)*per and len(names) == 43
    for m, mask in enumerate(MASKS):
        o = got[m*per:(m + 1)*per]
        for i in range(3):
            assert np.array_equal(o[i*kc:(i + 1)*kc], model[i, m]), (mask, i)
        for n, (name, _) in enumerate(names):
            assert np.array_equal(o[(3 + n)*kc:(4 + n)*kc], want[n, m], equal_nan=True), (mask, name)
    assert np.abs(want).max() > 0
