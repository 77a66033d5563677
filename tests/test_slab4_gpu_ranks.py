"""The 4th-order cases (moser600: advec_4 + diff_4 + pres_4) on the N > 1 path with the real HIP kernels. 2 and 4 ranks share the one
GPU of the test box (one process per rank; messages over gloo through host copies), one rank runs the exchanges through RCCL itself,
the full BASELINE size runs the slab code path on one rank, and the C++ slab driver runs Pres_4 on a one-rank RCCL communicator.
Every run is compared with the single-GPU path on the same fields: RHS tendencies bit-exact, p and the pressure-corrected tendencies
to 1e-10 (fp64) / 2e-4 (fp32)."""
import os
import tempfile

import numpy as np
import pytest

import hostprog
from ranks import run_ranks

pytestmark = pytest.mark.gpu
CASE = "moser600"
GRID = (128, 64, 32)


def _interior(hp, t):
    g = hp.grid
    return t[g.kstart:g.kend, g.jstart:g.jend, g.istart:g.iend].cpu().numpy().copy()


def _run(hp, out):
    hp.cyclic_prognostic()
    hp.exec_viscosity()
    hp.rhs()
    for n in ("ut", "vt", "wt"):
        out["rhs_" + n] = _interior(hp, getattr(hp, n))
    hp.pres()
    for n in ("ut", "vt", "wt", "p"):
        out[n] = _interior(hp, getattr(hp, n))
    out["div"] = np.array(hp.divergence())
    out["cfl"] = np.array(hp.cfl(0.5))


def _single(dtype=np.float64, **kw):
    from microhh_amd.model import HotPath, synthetic_global
    out = {}
    hp = HotPath(CASE, *GRID, device="cuda:0", dtype=dtype, global_init=synthetic_global(CASE, *GRID, dtype=dtype), **kw)
    _run(hp, out)
    hp.close()
    return out


def _compare(got, ref, tol, exact_div=True):
    for key in ("rhs_ut", "rhs_vt", "rhs_wt"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("ut", "vt", "wt", "p"):
        scale = np.abs(ref[key]).max()
        err = np.abs(got[key].astype(np.float64) - ref[key]).max() / scale
        assert err <= tol, (key, err)
    for cfl, div in zip(np.atleast_1d(got["cfl"]), np.atleast_1d(got["div"])):
        assert float(cfl) == float(ref["cfl"])
        if exact_div:
            assert abs(float(div) - float(ref["div"])) <= 1e-12 * abs(float(ref["div"])) + 1e-18


def _worker(rank, world, out, chunks, dtype):
    import torch
    from microhh_amd.model import HotPath, synthetic_global
    torch.cuda.set_device(0)
    hp = HotPath(CASE, *GRID, device="cuda:0", dtype=dtype, npy=world, rank=rank, global_init=synthetic_global(CASE, *GRID, dtype=dtype), pres_chunks=chunks)
    assert hp._host_staged and hp.pres_chunks == chunks and hp.lib.mhh_pres_slab_order(hp.plan) == 4
    _run(hp, out)
    hp.close()


def _ranks(world, chunks, dtype=np.float64):
    parts = run_ranks(_worker, world, backend="gloo", tag="slab4-gpu", args=(chunks, dtype))       # at most 4 ranks + this process on the GPU
    return {k: (np.concatenate([p[k] for p in parts], axis=1) if parts[0][k].ndim == 3 else np.array([float(p[k]) for p in parts]))
            for k in parts[0]}


@pytest.mark.parametrize("world,chunks", [(2, 1), (4, 1), (4, 4)], ids=["2", "4", "4-sliced"])
def test_pres4_slab_ranks_on_one_gpu_match_single_rank(world, chunks):
    _compare(_ranks(world, chunks), _single(), 1e-10)


def test_pres4_slab_ranks_on_one_gpu_fp32():
    _compare(_ranks(2, 1, np.float32), _single(np.float32), 2e-4)


def _rccl_worker(rank, world, out, chunks):
    from microhh_amd.model import HotPath, synthetic_global
    hp = HotPath(CASE, *GRID, device="cuda:0", npy=1, rank=0, force_slab=True, global_init=synthetic_global(CASE, *GRID), pres_chunks=chunks)
    assert hp.pres_chunks == chunks and hp._force_comm and not hp._host_staged
    _run(hp, out)
    hp.close()


@pytest.mark.parametrize("chunks", [1, 4], ids=["whole-transposes", "sliced-transposes"])
def test_pres4_slab_through_real_rccl_on_one_rank(chunks):
    """The slab code path with its exchanges through RCCL (nccl backend, one-rank communicator, MHH_FORCE_COMM=1): the halos of vt
    (2 rows south, 1 north) and p (1 south, 2 north) as batch_isend_irecv to self, the transposes as all_to_all_single -- whole or in
    four k-slices on the exchange stream. Same bits as the plain slab run on one rank, which matches the single-rank run."""
    plain = _single(force_slab=True, pres_chunks=chunks)
    _compare(plain, _single(), 1e-10)
    got, = run_ranks(_rccl_worker, 1, backend="nccl", tag="slab4-gpu-rccl", env={"MHH_FORCE_COMM": "1"}, args=(chunks,))
    for key in plain:
        assert np.array_equal(got[key], plain[key]), key


def test_pres4_slab_full_size_matches_single_gpu():
    """moser600 at its BASELINE size (512 x 256 x 256, fp64) through the slab code path on one rank against the single-GPU
    HotPath (its pressure step takes the transforms in LDS at this size); the slab result is a projection (bench.py's self-check,
    at the bound tests/test_bench_contract.py holds it to)."""
    import torch
    from microhh_amd.model import HotPath
    shape = (512, 256, 256)
    res = {}
    for slab in (False, True):
        hp = HotPath(CASE, *shape, device="cuda:0", dt=0.5, force_slab=slab)
        if not slab:
            assert hp.lib.mhh_pres_exec_form(hp.plan) == 1
        hp.cyclic_prognostic(); hp.exec_viscosity(); hp.rhs(); hp.pres(); hp.sync()
        g = hp.grid
        it = (slice(g.kstart, g.kend), slice(g.jstart, g.jend), slice(g.istart, g.iend))
        res[slab] = [t[it].clone() for t in (hp.ut, hp.vt, hp.wt, hp.p)]
        if slab:
            d1, d0 = hp.projected_divergence()
            assert d0 > 1e-3 and d1 / d0 < 1e-9, (d1, d0)
        hp.close()
        del hp
        torch.cuda.empty_cache()
    for a, b, n in zip(res[False], res[True], ("ut", "vt", "wt", "p")):
        assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max()), (n, float((a - b).abs().max()) / float(a.abs().max()))


@pytest.mark.parametrize("chunks", [1, 4], ids=["whole-transposes", "sliced-transposes"])
def test_cpp_pres_slab_order4_matches_single_gpu_pres(chunks):
    """Pres_slab<TF>(master, grid, fields, 4) of microhh_amd/host/mhh_host_rccl.h on a one-rank RCCL communicator against
    Pres<TF>(grid, fields, 4) of microhh_amd/host/mhh_host.h on the same fields: p, ut, vt, wt to 1e-10, the same divergence."""
    from microhh_amd.model import HotPath
    exe = hostprog.compile("pres4_slab", libs=("rccl",))
    hp = HotPath(CASE, 64, 32, 32, device="cuda:0", dt=0.5)
    hp.cyclic_prognostic(); hp.rhs(); hp.sync()
    g = hp.grid
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            np.array([g.itot, g.jtot, g.ktot, g.igc, g.jgc, g.kgc, chunks], dtype=np.int32).tofile(f)
            np.array([g.xsize, g.ysize, g.zsize, hp.dt], dtype=np.float64).tofile(f)
            for a in [getattr(g, n) for n in ("z", "zh", "dz", "dzh", "dzi", "dzhi", "dzi4", "dzhi4")] + [hp.rhoref_h, hp.rhorefh_h]:
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
            for t in (hp.u, hp.v, hp.w, hp.ut, hp.vt, hp.wt):
                t.cpu().numpy().astype(np.float64).tofile(f)
        hp.close()
        hostprog.run(exe, fin, fout, timeout=300)
        raw = np.fromfile(fout, dtype=np.float64)
    div1, div2 = raw[:2]
    n3 = g.ncells
    fields = raw[2:].reshape(2, 4, *g.shape3)
    it = (slice(g.kstart, g.kend), slice(g.jstart, g.jend), slice(g.istart, g.iend))
    for m, n in enumerate(("p", "ut", "vt", "wt")):
        a, b = fields[0, m][it], fields[1, m][it]
        assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max(), (n, np.abs(a - b).max() / np.abs(a).max())
    assert div1 == div2 and n3 == fields[0, 0].size
