"""Cost of Source and Decay on one GPU at N^3 (drycblles, fp64): the decay pass, the source pass with 1, 64 and 1024
sources, and beside it the same sources issued as one exec per single-source handle, which is the launch pattern of the reference's
GPU path (calc_source_g once per source, src/source.cu).

    python scripts/source_cost.py [--n 256] [--counts 1 64 1024] [--out profiles/source_cost.jsonl]

Every measurement is a child process of this script under its own `timeout`; the script stops at the first child that ends with a
non-zero status. The sources are blobs of sigma = 2.5 cells (a box of about 20 cells across) on four scalars, at seeded places
inside the domain. Each time is the median of 20 windows of device events, per call. One JSON line per measurement; with --step the
share of one drycblles step() of the same size (4 scalars, no other module) is added.
"""
import argparse
import json
import os
import subprocess
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


def sources(n, count, size):
    rs = np.random.RandomState(1234 + count)
    dx, dz = size[0]/n, size[2]/n
    out = []
    for m in range(count):
        c = rs.uniform(0.15, 0.85, 3)
        out.append(dict(scalar=m % NSC, x0=c[0]*size[0], y0=c[1]*size[1], z0=c[2]*size[2], sigma_x=2.5*dx, sigma_y=2.5*dx, sigma_z=2.5*dz,
                        strength=1. + m % 7))
    return out


def child(what, n, count):
    import torch
    from microhh_amd.model import HotPath, CASES
    from microhh_amd.source import Sources, Decay, Handle
    size = CASES["drycblles"]["size"]
    if what == "step":
        hp = HotPath("drycblles", n, n, n, nscalars=NSC)
        row = dict(name="step", n=n, nscalars=NSC, step_ms=round(median_ms(torch, hp.step, reps=1), 4))
    elif what == "decay":
        hp = HotPath("drycblles", n, n, n, nscalars=NSC, decay=Decay({m: 600. for m in range(NSC)}))
        row = dict(name="decay", n=n, scalars=NSC, ms=round(median_ms(torch, hp.decay.exec), 4), bytes_per_cell_per_scalar=24)
    elif what == "one_launch":
        src = sources(n, count, size)
        hp = HotPath("drycblles", n, n, n, nscalars=NSC, source=Sources(src))
        row = dict(name="one_launch", n=n, sources=count, tiles=hp.source.handle.tiles, ms=round(median_ms(torch, hp.source.exec), 4))
    else:           # the reference's launch pattern: one handle, one launch per source
        src = sources(n, count, size)
        hp = HotPath("drycblles", n, n, n, nscalars=NSC)
        hs = [Handle(hp.lib, hp.grid, [s], None, hp.rhoref_h, hp.stream) for s in src]

        def per_source():
            for h in hs:
                h.exec(hp.G, hp.fields, hp.stream)
        row = dict(name="launch_per_source", n=n, sources=count, ms=round(median_ms(torch, per_source, reps=2 if count > 100 else 10), 4))
        for h in hs:
            h.close()
    hp.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, metavar=("WHAT", "COUNT"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.n, int(a.child[1]))
        return
    jobs = ([] if a.no_step else [("step", 0)]) + [("decay", 0)] + [(w, c) for c in a.counts for w in ("one_launch", "launch_per_source")]
    rows = []
    for what, count in jobs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--child", what, str(count)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout); sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps(dict(name=what, sources=count, status=r.returncode, stopped=True)), flush=True)
            sys.exit(r.returncode)
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    step = next((r["step_ms"] for r in rows if r["name"] == "step"), None)
    if step:
        for r in rows:
            if "ms" in r:
                r["share_of_step"] = round(r["ms"] / step, 4)
                print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
