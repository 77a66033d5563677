"""Stats through the C++ host layer (Stats_sampler<TF> of microhh_amd/host/mhh_host.h): tests/cpp/host_stats.cpp runs the masks,
calc_stats, calc_tend and calc_stats_2d on 32 x 8 x 16 from inputs this test writes, and gives the bits of the same calls made
through the Python driver (microhh_amd.stats.Sampler). Built here with hipcc into a temporary directory."""
import os
import tempfile

import numpy as np
import pytest

import hostprog
from microhh_amd import stats as S
from microhh_amd.grid import Grid

GRID = (32, 8, 16)
THRESHOLD, OFFSET = 2.e-4, 1.5
MASKS = ("default", "wpos", "wneg")
PROFS = ("area", "areah", "u", "u_2", "u_3", "u_4", "u_grad", "w", "w_2", "w_grad", "q", "q_frac", "w_adv", "u_w", "u_diff", "u_flux")


def test_stats_host_program_compiles():
    """not gpu: the program and the host class it drives build against the library."""
    hostprog.compile("host_stats")


@pytest.mark.gpu
def test_cpp_host_stats_gives_the_bits_of_the_python_driver():
    import torch
    from microhh_amd import capi
    g = Grid(*GRID, 3200., 3200., 1200., order=2, igc=3, jgc=3, kgc=1)
    rs = np.random.RandomState(31)
    u, w = rs.random_sample(g.shape3) - 0.4, rs.random_sample(g.shape3) - 0.5
    q = np.where(rs.random_sample(g.shape3) < 0.3, 1.e-3*rs.random_sample(g.shape3), 0.)
    bot, rho = 290. + rs.random_sample(g.shape2), 1.1 - 0.01*np.arange(g.kcells)
    ev, fbot, ftop = 0.05 + rs.random_sample(g.shape3), rs.random_sample(g.shape2) - 0.5, rs.random_sample(g.shape2) - 0.5
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(u=u, w=w, q=q, bot=bot, rho=rho, ev=ev, fbot=fbot, ftop=ftop).items()}
    sm = S.Sampler(capi.lib(), g, g.device_struct(dev), torch, dev, MASKS, stream=lambda: None)
    sm.initialize_masks()
    sm.set_mask_thres("wpos", d["w"], d["w"], None, 0., S.PLUS)
    sm.set_mask_thres("wneg", d["w"], d["w"], None, 0., S.MIN)
    sm.finalize_masks()
    a = sm.profiles([(d["u"], 0, S.MEAN, OFFSET, 0., None), (d["w"], 1, S.MEAN, 0., 0., None), (d["q"], 0, S.MEAN, 0., THRESHOLD, None),
                     (d["bot"], 0, S.MEAN2D, OFFSET, 0., None), (d["w"], 1, S.MEAN, 0., 0., None)])
    b = sm.profiles([(d["u"], 0, op, OFFSET, 0., a[0] if op != S.GRAD else None) for op in (S.MOMENT2, S.MOMENT3, S.MOMENT4, S.GRAD)] +
                    [(d["w"], 1, S.MOMENT2, 0., 0., a[1]), (d["w"], 1, S.GRAD, 0., 0., None), (d["q"], 0, S.FRAC, 0., THRESHOLD, None)])
    fx = dict(kind=1, w=d["w"], wmean=a[1], evisc=d["ev"], flux_bot=d["fbot"], flux_top=d["ftop"], visc=1.e-5, tPr=1./3., limit=0, surface_model=1)
    c = sm.profiles([(d["u"], 0, S.FLUX_W, OFFSET, 0., a[0], dict(fx, scheme=25)), (d["u"], 0, S.FLUX_DIFF, OFFSET, 0., a[0], dict(fx, scheme=22)),
                     (d["u"], 0, S.FLUX_SUM, OFFSET, 0., a[0], dict(a=0, b=1))])
    col = sm.columns(d["q"], 0, 0., THRESHOLD, d["rho"]).cpu().numpy()
    torch.cuda.synchronize()
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    nmask, nbot = sm.nmask.cpu().numpy(), sm.nmask_bot.cpu().numpy()
    want = {"area": sm.area.cpu().numpy(), "areah": sm.areah.cpu().numpy(), "u": a[0], "u_2": b[0], "u_3": b[1], "u_4": b[2], "u_grad": b[3],
            "w": a[1], "w_2": b[4], "w_grad": b[5], "q": a[2], "q_frac": b[6], "w_adv": a[4], "u_w": c[0], "u_diff": c[1], "u_flux": c[2]}
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        hostprog.write_doubles(fin, (u, w, q, ev, bot, fbot, ftop, rho, g.z, g.zh, g.dz, g.dzh, g.dzi, g.dzhi))
        hostprog.run(hostprog.compile("host_stats"), fin, fout, *GRID, repr(THRESHOLD), repr(OFFSET))
        got = hostprog.read_doubles(fout)
    kc = g.kcells
    per = (2 + len(PROFS))*kc + 4
    assert got.size == len(MASKS)*per
    for m, mask in enumerate(MASKS):
        o = got[m*per:(m + 1)*per]
        assert np.array_equal(o[:kc], nmask[m, 0]) and np.array_equal(o[kc:2*kc], nmask[m, 1]), mask
        for n, name in enumerate(PROFS):
            assert np.array_equal(o[(2 + n)*kc:(3 + n)*kc], want[name][m]), (mask, name)
        tail = o[(2 + len(PROFS))*kc:]
        assert tail[0] == col[m, 0] and tail[1] == col[m, 1] and tail[2] == a[3, m, 0] and tail[3] == nbot[m], mask
    assert 0 < nmask[1, 0, g.kstart] < GRID[0]*GRID[1] and col[0, 0] > 0.
