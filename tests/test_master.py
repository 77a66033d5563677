"""microhh_amd.master.Master alone -- no grid, no library, a few hundred elements per buffer: every element of every rank's receive
buffer against rank arithmetic, in each of its three modes. local: in this process. direct: gloo on CPU tensors with 2, 3 and 4
ranks (3 = the smallest ring whose north and south neighbours differ with an odd rank count) and, on the GPU, RCCL on a one-rank
communicator. host_staged: two ranks sharing the GPU over gloo. Then HotPath._halo2d, which rides on Master.ring, against the
periodic image of a global array."""
import numpy as np
import pytest
import torch

import backends as B
from microhh_amd.master import Master
from ranks import run_ranks

RING_CASES = [(6, 6), (6, 0), (0, 6), (5, 3)]     # (nn, ns): (., 0) leaves messages out, two ranks send the whole buffer at once
TAIL, SENTINEL = 4, -1.                           # elements beyond nn + ns, in send and recv alike: nobody may write there
SEG = 7                                           # elements per peer of the all-to-all
# jtot = 24: 12 or 8 rows per rank, jmax >= jgc = 3; three ranks need an itot that divides by three as well (Grid: itot % npy == 0)
HALO_GRID = {2: (16, 24, 4), 3: (24, 24, 4)}


def _enc(rank, part, n):
    """n values that say who sent them (rank), as which part (ring: 0 northbound, 1 southbound; all-to-all: the peer) and where."""
    return rank * 1e4 + part * 1e3 + np.arange(n, dtype=np.float64)


def _summand(rank):
    return (rank + 1.) * np.arange(1., 6.)        # whole numbers: their sum is exact in any order


def _exercise(m, out):
    dev, host = m.device, (lambda t: t.cpu().numpy().copy())
    for nn, ns in RING_CASES:
        send = np.full(nn + ns + TAIL, SENTINEL)
        send[:nn], send[nn:nn+ns] = _enc(m.rank, 0, nn), _enc(m.rank, 1, ns)
        send = torch.from_numpy(send).to(dev)
        recv = torch.full_like(send, SENTINEL)
        m.ring(send, recv, nn, ns)
        out["ring_%d_%d" % (nn, ns)] = host(recv)
    send = torch.from_numpy(np.concatenate([_enc(m.rank, peer, SEG) for peer in range(m.npy)])).to(dev)
    recv = torch.full_like(send, SENTINEL)
    m.all_to_all(send, recv)
    out["all_to_all"] = host(recv)
    out["max"] = np.array(m.max(float(np.sin(m.rank + 1.))))
    s = m.sum_(torch.from_numpy(_summand(m.rank)).to(dev))
    assert s.device == torch.empty(0, device=dev).device
    out["sum"] = host(s)
    m.barrier()
    out["barrier_returned"] = np.array(1)


def _check(parts):
    world = len(parts)
    for r, p in enumerate(parts):
        for nn, ns in RING_CASES:
            want = np.concatenate([_enc((r - 1) % world, 0, nn), _enc((r + 1) % world, 1, ns), np.full(TAIL, SENTINEL)])
            assert np.array_equal(p["ring_%d_%d" % (nn, ns)], want), (world, r, nn, ns)
        assert np.array_equal(p["all_to_all"], np.concatenate([_enc(peer, r, SEG) for peer in range(world)])), (world, r)
        assert float(p["max"]) == np.max([float(np.sin(q + 1.)) for q in range(world)])
        assert np.array_equal(p["sum"], np.sum([_summand(q) for q in range(world)], axis=0))
        assert int(p["barrier_returned"]) == 1


def _worker(rank, world, out, device, force_comm, mode):
    if device != "cpu":
        torch.cuda.set_device(0)
    m = Master(world, rank, None, torch.device(device), force_comm)
    assert m.mode == mode and (m.south, m.north) == ((rank - 1) % world, (rank + 1) % world) and m.ranks == list(range(world))
    assert m.side_stream() is None or device != "cpu"
    _exercise(m, out)


def test_local_mode_is_copies():
    m = Master(1, 0, None, torch.device("cpu"), False)
    assert m.mode == "local" and m.side_stream() is None
    out = {}
    _exercise(m, out)
    _check([out])


@pytest.mark.parametrize("world", [2, 3, 4])
def test_direct_mode_over_gloo_on_cpu_tensors(world):
    _check(run_ranks(_worker, world, backend="gloo", tag="master", args=("cpu", False, "direct")))


@pytest.mark.gpu
def test_host_staged_mode_two_ranks_share_the_gpu():
    _check(run_ranks(_worker, 2, backend="gloo", tag="master", args=("cuda:0", False, "host_staged")))


@pytest.mark.gpu
def test_direct_mode_over_rccl_to_self():
    _check(run_ranks(_worker, 1, backend="nccl", tag="master", args=("cuda:0", True, "direct")))


@pytest.mark.gpu
def test_side_stream_and_slice_events_are_made_once_per_shape():
    m = Master(1, 0, None, torch.device("cuda:0"), False)
    side = m.side_stream()
    assert side is m.side_stream() and isinstance(side[0], torch.cuda.Stream) and len(side[1]) == 2
    ev = m.slice_events(4)
    assert ev is m.slice_events(4) and [len(e) for e in ev] == [4] * 4
    assert [len(e) for e in m.slice_events(2)] == [2] * 4


def _halo2d_worker(rank, world, out):
    from microhh_amd.model import HotPath
    hp = HotPath("drycblles", *HALO_GRID[world], device="cpu", lib=B.get("emul").lib, npy=world, rank=rank)
    g = hp.grid
    t = torch.zeros(g.shape2, dtype=hp.td)
    t[g.jstart:g.jend, g.istart:g.iend] = torch.from_numpy(_global2d(world)[rank*g.jmax:(rank+1)*g.jmax])
    hp._halo2d(t)
    out["t"], out["gc"] = t.numpy().copy(), np.array([g.jgc, g.igc])
    hp.close()


def _global2d(world):
    itot, jtot, _ = HALO_GRID[world]
    return 100. * np.arange(jtot)[:, None] + np.arange(itot)[None, :]


@pytest.mark.parametrize("world", [2, 3])
def test_halo2d_gives_the_periodic_image_of_the_global_array(world):
    """Every ghost row (and, with the east-west wrap, every ghost column) of every rank's array."""
    itot, jtot, _ = HALO_GRID[world]
    a, jmax = _global2d(world), jtot // world
    for r, p in enumerate(run_ranks(_halo2d_worker, world, backend="gloo", tag="master")):
        jgc, igc = p["gc"]
        jj, ii = np.arange(-jgc, jmax + jgc) + r * jmax, np.arange(-igc, itot + igc)
        assert np.array_equal(p["t"], a[np.ix_(jj % jtot, ii % itot)]), (world, r)
