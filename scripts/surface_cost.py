"""Cost of the surface layer: mhh_boundary_surface_exec against its five stage calls, and its share of a step.

    python scripts/surface_cost.py [--grids 256x256x16 512x512x16 1024x1024x16:float32] [--step 256] [--out profiles/surface_cost.jsonl]

Per grid (drycblles: mbcbot = noslip, th with sbcbot = flux, Thermo_dry): the fused call and the staged sequence (five stage calls
and three 2-D cyclic fills), each per call as the median of 20 windows of 50 calls timed with device events, in the steady state -- after a first call has
moved nobuk from 0 -- and the walk lengths seen (table steps per column in the first call and in a later one). The surface layer
works on 2-D arrays, so ktot is kept small for the large column counts. Then one step() of HotPath("drycblles", N, N, N) with and
without surface= in the same process: the yardstick is that run's own step without the surface layer. Every call's return code is
checked. One JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(torch, fn, n=20, warmup=3, reps=1):
    """Median over n windows of `reps` calls each, per call: a window of one 20-microsecond call would time the event pair."""
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


def make(shape, dtype, surface=True):
    from microhh_amd.model import HotPath
    from microhh_amd.surface import Surface
    return HotPath("drycblles", *shape, dtype=dtype, surface=Surface(mbcbot="noslip", sbcbot="flux", sbot=0.1) if surface else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["256x256x16", "512x512x16", "1024x1024x16:float32"])
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for spec in args.grids:
        parts = spec.split(":")
        shape = tuple(int(x) for x in parts[0].split("x"))
        dtype = np.dtype(parts[1] if len(parts) > 1 else "float64").type
        hp = make(shape, dtype)
        sf = hp.surface
        hp.cyclic_prognostic()
        sf.exec(); hp.sync()
        n1 = sf.nobuk.cpu().numpy().astype(np.int64)
        sf.exec(); hp.sync()
        n2 = sf.nobuk.cpu().numpy().astype(np.int64)
        head = dict(shape=list(shape), dtype=np.dtype(dtype).name, columns=shape[0]*shape[1])
        emit(dict(head, name="walk", first_call_max=int(n1.max()), first_call_mean=round(float(n1.mean()), 1), later_call_max=int(np.abs(n2 - n1).max())))
        fused, staged = median_ms(torch, sf.exec, reps=50), median_ms(torch, sf.staged, reps=50)
        emit(dict(head, name="surface", fused_ms=round(fused, 4), staged_ms=round(staged, 4), ratio=round(fused / staged, 3)))
        hp.close(); del hp
        torch.cuda.empty_cache()
    n = args.step
    ms = {}
    for surface in (False, True):
        hp = make((n, n, n), np.float64, surface)
        ms[surface] = median_ms(torch, hp.step)
        if surface:
            ms["surface_alone"] = median_ms(torch, hp.surface_layer, reps=50)
        hp.close(); del hp
        torch.cuda.empty_cache()
    emit(dict(name="step", shape=[n, n, n], dtype="float64", step_ms=round(ms[False], 4), step_with_surface_ms=round(ms[True], 4),
              surface_and_ghost_cells_ms=round(ms["surface_alone"], 4), share_of_step=round((ms[True] - ms[False]) / ms[False], 4)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
