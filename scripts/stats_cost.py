"""Cost of one statistics sample next to one step of the same HotPath.

    python scripts/stats_cost.py [--configs drycblles256 drycblles512 bomex256] [--out profiles/stats.jsonl]

Per configuration, fp64, in ONE process: after warm-up, `rounds` alternating rounds of (windows of sample(), windows of the device part
of a sample without the read-back, windows of step()), each window timed with device events; the figure is the smallest of the rounds'
medians and the rounds are listed (their spread is the noise). drycblles: the default mask alone and what Stats.bind registers. bomex:
256 x 256 x 128 with thermo=Moist and masks=("default", "ql", "wplus"), plus ql with mean, frac, path and cover; ql, ql_h and w at the
full level are evaluated once per sample (two saturation-adjustment passes and an interpolation) and that is part of the time.

Algorithmic bytes of a sample: every registered variable once per pass it takes part in (pass A if it has a mean, pass B if it has a
moment, frac or gradient, the column pass if it has path or cover, and a flux pass of its own -- the variable, w and evisc -- if it
has fluxes), mfield once per pass (init is a write, every threshold reads
two fields and reads and writes mfield, the count reads it), over the interior cells. The kernels read a variable once per group of up to
four operations of pass B and, for a gradient, the level below as well; the caches may or may not absorb that. One JSON line per
configuration."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBPS = 6.3          # the copy rate DESIGN.md §7 quotes


def windows_ms(torch, fn, n=7, reps=1):
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts))


def algorithmic_bytes(st, g):
    from microhh_amd import stats as S
    ncell, tf = g.imax*g.jmax*g.kmax, g.np_dtype.itemsize
    fields = 0
    passes = {"count": 1, "A": 0, "B": 0, "column": 0, "flux": 0}
    for name, t, loc, ops, off, thr in st.vars:
        a = "mean" in ops
        b = any(op in S.PASS_B for op in ops)
        c = any(op in S.COLUMN for op in ops)
        d = any(op in S.FLUXES for op in ops)             # the flux pass of a variable: the variable, w and evisc, once each
        fields += a + b + c + 3*d
        passes["A"] |= a; passes["B"] |= b; passes["column"] += c; passes["flux"] += d
    mfield = 1 + 2*len(st.thresholds) + passes["count"] + passes["A"] + passes["B"] + passes["column"] + passes["flux"]
    fields += 2*len(st.thresholds)
    return ncell*(fields*tf + mfield*4), fields, mfield


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["drycblles256", "drycblles512", "bomex256"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from microhh_amd import stats as S
    from microhh_amd.model import CASES, HotPath
    from microhh_amd.thermo import Moist
    lines = []
    for cfg in args.configs:
        if cfg.startswith("drycblles"):
            n = int(cfg[len("drycblles"):])
            shape, masks = (n, n, n), ("default",)
            hp = HotPath("drycblles", *shape, stats=S.Stats(masks=masks))
        else:
            shape, masks = (256, 256, 128), ("default", "ql", "wplus")
            hp = HotPath("bomex", *shape, dt=2., thermo=Moist(CASES["bomex"]["pbot"]), stats=S.Stats(masks=masks))
            hp.stats.add("ql", hp.stats.ql, 0, ("mean", "frac", "path", "cover"))
        st = hp.stats
        for _ in range(3):
            hp.step()
        r = st.sample(); st.sample()
        assert np.all(r["default"]["area"][hp.grid.kstart:hp.grid.kend] == 1)
        rounds = {"sample": [], "device": [], "step": []}
        for _ in range(args.rounds):
            rounds["sample"].append(windows_ms(torch, st.sample))
            rounds["device"].append(windows_ms(torch, st.enqueue, reps=3))
            rounds["step"].append(windows_ms(torch, hp.step, reps=3))
        nbytes, nfields, nmf = algorithmic_bytes(st, hp.grid)
        ms = {k: min(v) for k, v in rounds.items()}
        row = dict(name=cfg, shape=list(shape), dtype="float64", masks=list(masks), variables=[v[0] for v in st.vars],
                   sample_ms=round(ms["sample"], 4), device_part_ms=round(ms["device"], 4), step_ms=round(ms["step"], 4),
                   sample_over_step=round(ms["sample"]/ms["step"], 3),
                   rounds_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                   algorithmic_field_passes=nfields, algorithmic_mfield_passes=nmf, algorithmic_bytes=int(nbytes),
                   TBps_on_algorithmic_bytes=round(nbytes/(ms["device"]*1e-3)/1e12, 3), share_of_copy_rate=round(nbytes/(ms["device"]*1e-3)/1e12/COPY_TBPS, 3))
        lines.append(row)
        print(json.dumps(row), flush=True)
        hp.close(); del hp, st
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
