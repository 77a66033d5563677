"""One rank-spawn harness for the N > 1 tests: fresh child processes on 127.0.0.1, one torch.distributed group, one result
file per rank.

A worker is a module-level ``worker(rank, world, out, *args)``: it runs with the process group up, leaves numpy arrays in the
dict ``out`` and closes what it opened; ``run_ranks`` hands the parent one dict per rank."""
import os
import sys
import tempfile
import zlib

import numpy as np

import common as cm

TESTS = os.path.dirname(os.path.abspath(__file__))

# One base per tag, 29300 ... 30700 as the modules had them; a case of a tag moves up by less than 100 with its world size
# and arguments, the process by its pid: two suites on one host, and two cases in a row, keep apart.
PORT_BASE = {"slab-scalars-emul": 29300, "slab-gloo": 29500, "slab-save": 29600, "slab-gpu": 29700, "slab-scalars-gpu": 29800,
             "slab-gpu-rccl": 29900, "slab4-gloo": 30100, "slab4-gpu": 30300, "slab4-gpu-rccl": 30500, "master": 30700}


def port(tag, world, args):
    return PORT_BASE[tag] + zlib.crc32(repr((world, args)).encode()) % 100 + os.getpid() % 1000


def _child(rank, worker, world, backend, master_port, tmp, env, args):
    for p in (cm.ROOT, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(master_port)
    os.environ.update(env)
    if backend == "nccl":                # RCCL itself on a one-rank communicator (two ranks on one device are refused)
        import torch
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        out = {}
        worker(rank, world, out, *args)
        np.savez(os.path.join(tmp, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


def run_ranks(worker, world, *, backend, tag, env=None, args=()):
    """worker on `world` fresh processes (torch.multiprocessing.spawn: at most four ranks beside the parent on a GPU), each with
    `env` set before the group comes up; returns [out of rank 0, out of rank 1, ...]."""
    import torch.multiprocessing as mp
    assert backend == "gloo" or (backend == "nccl" and world == 1)
    env = {k: str(v) for k, v in (env or {}).items()}
    cm.known_switches(env)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_child, args=(worker, world, backend, port(tag, world, args), tmp, env, tuple(args)), nprocs=world, join=True)
        parts = []
        for r in range(world):
            with np.load(os.path.join(tmp, "rank%d.npz" % r)) as z:
                parts.append({k: z[k] for k in z.files})
    return parts
