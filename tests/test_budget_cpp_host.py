"""Budget_2 through the C++ host layer (Budget_2_sampler<TF> of microhh_amd/host/mhh_host.h): tests/cpp/host_budget.cpp runs the
masks of a Stats_sampler and exec_stats with every group on 32 x 8 x 16 from inputs this test writes, and gives the bits of the same
calls made through the Python driver (microhh_amd.budget.Budget2Sampler). Built here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import hostprog
import stats_ref as R
from microhh_amd import budget as BU
from microhh_amd import stats as S
from microhh_amd.grid import DIFF_SMAG2, Grid

GRID = (32, 8, 16)
UTRANS, VTRANS, FC = 1.5, -0.5, 1.e-4
MASKS = ("default", "wpos", "wneg")
ALL = 0x7ff


def test_budget_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_budget")


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
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, [f3[n] for n in ("u", "v", "w", "p", "evisc", "b")] + [f2["u_fluxbot"], f2["v_fluxbot"], g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi])
        hostprog.run(hostprog.compile("host_budget"), fin, fout, *GRID, repr(UTRANS), repr(VTRANS), repr(FC))
        got = hostprog.read_doubles(fout)
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
