"""Several scalars on the slab path: the overlapped sub-step (interior rows while the halos travel, then the edge strips) with
scalars beyond th, which the row-wise calls run in the scalar pass of the marching kernel. Compared with the single-rank run on
the same global fields: RHS tendencies (every st included) and evisc bit-exact, pressure-corrected tendencies to 1e-10.

* emulated: world 2 over gloo, kernels = the library's own sources on the CPU (tests/emul);
* on the GPU (marked gpu): 2 rank processes sharing the one card, messages over gloo through host copies."""
import numpy as np
import pytest

import backends as B
from ranks import run_ranks

GRID = (16, 32, 10)
GRID_GPU = (128, 64, 32)


def _interior(hp, t):
    g = hp.grid
    return t[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()


def _run(hp, out, overlapped=False):
    if overlapped:
        assert hp.can_overlap
        hp.halo_visc_rhs()
    else:
        hp.cyclic_prognostic()
        hp.exec_viscosity()
        hp.rhs()
    out["evisc"] = _interior(hp, hp.evisc)
    for n in ("ut", "vt", "wt"):
        out["rhs_" + n] = _interior(hp, getattr(hp, n))
    for m, t in enumerate(hp.st):
        out["rhs_st%d" % m] = _interior(hp, t)
    hp.pres()
    for n in ("ut", "vt", "wt", "p"):
        out[n] = _interior(hp, getattr(hp, n))


def _compare(parts, ref, nsc):
    for key in ["evisc", "rhs_ut", "rhs_vt", "rhs_wt"] + ["rhs_st%d" % m for m in range(nsc)]:
        got = np.concatenate([p[key] for p in parts], axis=1)
        assert np.array_equal(got, ref[key]), key
    for key in ("ut", "vt", "wt", "p"):
        got = np.concatenate([p[key] for p in parts], axis=1)
        scale = np.abs(ref[key]).max()
        assert np.abs(got - ref[key]).max() <= 1e-10 * scale, (key, np.abs(got - ref[key]).max() / scale)


def _emul_worker(rank, world, out, nsc):
    from microhh_amd.model import HotPath, synthetic_global
    lib = B.get("emul").lib
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib, npy=world, rank=rank, nscalars=nsc,
                 global_init=synthetic_global("drycblles", *GRID, nscalars=nsc), overlap=True)
    assert len(hp.s) == nsc and hp.can_overlap
    _run(hp, out, overlapped=True)
    hp.close()


def test_overlapped_slab_with_three_scalars_matches_single_rank_emulated():
    from microhh_amd.model import HotPath, synthetic_global
    nsc, world = 3, 2
    lib = B.get("emul").lib
    ref = {}
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib, nscalars=nsc, global_init=synthetic_global("drycblles", *GRID, nscalars=nsc))
    assert len(hp.s) == nsc
    _run(hp, ref)
    hp.close()
    _compare(run_ranks(_emul_worker, world, backend="gloo", tag="slab-scalars-emul", args=(nsc,)), ref, nsc)


def test_hotpath_scalar_count():
    """nscalars=None keeps the case's count; the synthetic scalars beyond th follow th's recipe."""
    from microhh_amd.model import CASES, HotPath, synthetic_global
    lib = B.get("emul").lib
    gi = synthetic_global("drycblles", *GRID, nscalars=4)
    assert all(("s%d" % m) in gi for m in range(4)) and "s4" not in gi
    assert "s1" not in synthetic_global("drycblles", *GRID)
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib)
    assert len(hp.s) == CASES["drycblles"]["nscalars"]
    hp.close()
    hp = HotPath("drycblles", *GRID, device="cpu", lib=lib, nscalars=2, force_slab=True, overlap=True)
    assert len(hp.s) == len(hp.st) == 2 and hp.fields.nscalars == 2 and hp.can_overlap
    hp.close()
    with pytest.raises(ValueError):
        HotPath("drycblles", *GRID, device="cpu", lib=lib, nscalars=9)


def _gpu_worker(rank, world, out, nsc):
    import torch
    from microhh_amd.model import HotPath, synthetic_global
    torch.cuda.set_device(0)
    hp = HotPath("drycblles", *GRID_GPU, device="cuda:0", npy=world, rank=rank, nscalars=nsc,
                 global_init=synthetic_global("drycblles", *GRID_GPU, nscalars=nsc), overlap=True)
    assert hp._host_staged and hp.can_overlap
    _run(hp, out, overlapped=True)
    hp.close()


@pytest.mark.gpu
def test_overlapped_slab_with_two_scalars_on_one_gpu_matches_single_rank():
    from microhh_amd.model import HotPath, synthetic_global
    nsc, world = 2, 2
    ref = {}
    hp = HotPath("drycblles", *GRID_GPU, device="cuda:0", nscalars=nsc, global_init=synthetic_global("drycblles", *GRID_GPU, nscalars=nsc))
    _run(hp, ref)
    hp.close()
    _compare(run_ranks(_gpu_worker, world, backend="gloo", tag="slab-scalars-gpu", args=(nsc,)), ref, nsc)
