"""Cost of the immersed boundary: its share of a step, the two launches and their cyclic fills, the host set-up.

    python scripts/ib_cost.py [--step 256] [--no-trace] [--out profiles/ib_cost.jsonl]      # on the GPU
    python scripts/ib_cost.py --setup 256 512                                               # host only, one core, no GPU touched

drycblles N^3 with the sine terrain (A = 0.15, n_idw = 5, sbcbot = flux). One step() of HotPath with and without ib= in the same
process, each as the median of 20 windows timed with device events; exec_scalars and exec_momentum (launch plus fills) and the
launches alone, per call over windows of 50. Then, unless --no-trace, a child process of this script under
`rocprofv3 --kernel-trace --stats` that runs the two IB calls alone, so that every cyclic-fill launch of its trace after the
constructor belongs to them; the rows of the kernel statistics are printed as they are. --setup times mhh_ib_ghost_cells_host for
the four locations at N x N columns (ktot = 64), serially. One JSON line per measurement."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N_IDW, AMPLITUDE = 5, 0.15


def median_ms(torch, fn, n=20, warmup=3, reps=1):
    """Median over n windows of `reps` calls each, per call."""
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


def dem_of(n):
    from microhh_amd import ib
    from microhh_amd.model import CASES
    return ib.sine_dem(n, n, *CASES["drycblles"]["size"], AMPLITUDE)


def make(n, with_ib):
    from microhh_amd.ib import Dem
    from microhh_amd.model import HotPath
    return HotPath("drycblles", n, n, n, ib=Dem(dem_of(n), N_IDW, sbcbot="flux", sbot=(0.1,)) if with_ib else None)


def setup_times(sizes, emit):
    from microhh_amd import capi, ib
    from microhh_amd.grid import Grid
    from microhh_amd.model import CASES
    lib = capi.lib()
    for n in sizes:
        g = Grid(n, n, 64, *CASES["drycblles"]["size"], order=2, igc=3, jgc=3, kgc=1)
        dem = np.pad(dem_of(n), 3, mode="wrap")
        c = ib.locations(g)
        row = dict(name="setup", columns=n*n, ktot=64, n_idw=N_IDW)
        total = 0.
        for loc, ax in (("u", (c["xh"], c["y"], g.z, g.dz)), ("v", (c["x"], c["yh"], g.z, g.dz)), ("w", (c["x"], c["y"], g.zh, g.dzh)), ("s", (c["x"], c["y"], g.z, g.dz))):
            t0 = time.perf_counter()
            gh = ib.ghost_cells(lib, g, dem, *ax, N_IDW, 0)
            dt = time.perf_counter() - t0
            total += dt
            row["%s_s" % loc], row["%s_nghost" % loc] = round(dt, 2), gh["nghost"]
        row["total_s"] = round(total, 2)
        emit(row)


def child(n):
    """The two IB calls alone, for the kernel trace."""
    hp = make(n, True)
    for _ in range(50):
        hp.ib.exec_scalars(); hp.ib.exec_momentum()
    hp.sync()
    hp.close()


def trace(n, emit):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child", "--step", str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            emit(dict(name="trace", error=r.stderr[-500:]))
            return
        for fn in glob.glob(os.path.join(tmp, "**", "*kernel_stats*.csv"), recursive=True):
            with open(fn) as fh:
                for row in csv.DictReader(fh):
                    if "ib_" in row.get("Name", "") or "cyclic" in row.get("Name", ""):
                        emit(dict(name="kernel", kernel=row["Name"][:90], calls=int(row["Calls"]), total_ns=int(row["TotalDurationNs"]), average_ns=float(row["AverageNs"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--setup", type=int, nargs="+", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    if args.child:
        child(args.step)
        return
    if args.setup:
        setup_times(args.setup, emit)
    else:
        import torch
        n = args.step
        ms = {}
        for with_ib in (False, True):
            t0 = time.perf_counter()
            hp = make(n, with_ib)
            bind_s = time.perf_counter() - t0
            ms[with_ib] = median_ms(torch, hp.step)
            if with_ib:
                ib = hp.ib
                ms["scalars"], ms["momentum"] = median_ms(torch, ib.exec_scalars, reps=50), median_ms(torch, ib.exec_momentum, reps=50)
                ms["set_s"], ms["set_m"] = median_ms(torch, ib.set_scalars, reps=50), median_ms(torch, ib.set_momentum, reps=50)
                nghost = {k: v["nghost"] for k, v in ib.ghost.items()}
                ms["bind_s"] = bind_s
            hp.close(); del hp
            torch.cuda.empty_cache()
        emit(dict(name="step", shape=[n, n, n], dtype="float64", step_ms=round(ms[False], 4), step_with_ib_ms=round(ms[True], 4),
                  share_of_step=round((ms[True] - ms[False]) / ms[False], 4), exec_scalars_ms=round(ms["scalars"], 4), exec_momentum_ms=round(ms["momentum"], 4),
                  launch_scalars_ms=round(ms["set_s"], 4), launch_momentum_ms=round(ms["set_m"], 4), nghost=nghost, bind_with_ib_s=round(ms["bind_s"], 1)))
        if not args.no_trace:
            trace(n, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
