"""Cost of Boundary_outflow on one GPU at N^3 (the drycblles layout, gc (3,3,1), fp64 by default): the time of
mhh_boundary_outflow_exec on four open scalars, all four edges (West inflow, the others outflow), and next to it the time of
mhh_boundary_cyclic_n on the same four fields, alternating in one process so that both see the same machine.

    python scripts/outflow_cost.py [--n 512] [--dtype f64] [--rounds 5] [--out profiles/outflow_cost.jsonl]

A time is the median of 20 windows of device events around 10 calls, per call; a round measures the cyclic fill, then the outflow
fill, and the rounds' figures show the run-to-run spread. Also printed: the launches of one outflow call, with one scalar and with
four. One JSON line per figure. Both fills are idempotent on the fields they have filled, so the rounds repeat the same work.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NSC = 4


def median_ms(torch, fn, n=20, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--igc", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from microhh_amd import capi, outflow
    from microhh_amd.grid import Grid, EDGE_BOTH
    from microhh_amd.model import CASES
    assert torch.cuda.is_available(), "this measures the GPU: there is no fallback"
    lib = capi.lib()
    dt = np.float64 if a.dtype == "f64" else np.float32
    td = torch.float64 if a.dtype == "f64" else torch.float32
    n = a.n
    g = Grid(n, n, n, *CASES["drycblles"]["size"], order=2, igc=a.igc, jgc=3, kgc=1, dtype=dt)
    G = g.device_struct("cuda:0")
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    flds = [torch.rand(g.shape3, generator=gen, device="cuda:0", dtype=td) for _ in range(NSC)]
    tabs = [torch.from_numpy(outflow.profile_table(lib, g, np.linspace(0., 1., g.ktot) + m)).to("cuda:0") for m in range(NSC)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fa = (C.c_void_p * NSC)(*[t.data_ptr() for t in flds])
    pa = (C.c_void_p * NSC)(*[t.data_ptr() for t in tabs])
    dirs = (C.c_int * 4)(1, 0, 0, 0)

    def cyclic():
        capi.check(lib.mhh_boundary_cyclic_n(G, fa, NSC, EDGE_BOTH, stream), lib)

    def open_(nf=NSC):
        capi.check(lib.mhh_boundary_outflow_exec(G, 2, fa, nf, pa, dirs, 15, stream), lib)
    rows = []
    open_(1); one = int(lib.mhh_boundary_outflow_last_launches())
    open_(NSC); four = int(lib.mhh_boundary_outflow_last_launches())
    rows.append(dict(name="launches", one_scalar=one, four_scalars=four))
    ghost = 2*g.igc*g.jcells*g.kcells + 2*g.kgc*g.icells*g.kcells
    cyc_ghost = 2*g.igc*g.jcells*g.kcells + 2*g.jgc*g.icells*g.kcells
    for r in range(a.rounds):
        c = median_ms(torch, cyclic)
        o = median_ms(torch, open_)
        rows.append(dict(name="round", round=r, n=n, dtype=a.dtype, igc=g.igc, scalars=NSC, cyclic_n_ms=round(c, 5), outflow_ms=round(o, 5),
                         ghost_cells_written_outflow=NSC*ghost, ghost_cells_written_cyclic=NSC*cyc_ghost))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
