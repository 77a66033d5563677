"""What a budget sample costs: hp.stats.sample() with and without budget=Budget2() against the step time of the same run.

drycblles, fp64, the default mask alone and three masks (default, wplus, wmin). A timed window holds `--calls` consecutive calls
between two synchronisations, so that it is tens of milliseconds of work and the host clock's resolution and the launch jitter of a
single call do not show; a figure is the window's time over its calls, the median of `--repeats` windows after `--warmup` untimed
ones, with the spread (min .. max). sample() ends with a synchronisation and the copies of the profiles to the host, which are part of
what a sample costs and are inside the window. Prints one JSON line; --write puts the table between the two `budget_cost` markers of
profiles/budget.md.

    python scripts/budget_cost.py [--n 256] [--calls 10] [--repeats 9] [--warmup 2] [--write]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DOC = os.path.join(ROOT, "profiles", "budget.md")
BEGIN, END = "<!-- budget_cost:begin -->", "<!-- budget_cost:end -->"


def timed(fn, sync, calls, warmup, repeats):
    def window():
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        return (time.perf_counter() - t0)*1e3/calls
    for _ in range(warmup):
        window()
    out = [window() for _ in range(repeats)]
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def table(res):
    lines = ["drycblles %d^3 %s; %d calls per timed window, %d warm-up windows, the median of %d windows with the spread."
             % (res["n"], res["dtype"], res["calls"], res["warmup"], res["repeats"]), "",
             "| masks | budget | step ms (min .. max) | sample ms (min .. max) |", "|---|---|---|---|"]
    for r in res["runs"]:
        lines.append("| %d | %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) |" % (
            r["masks"], "yes, %d profiles" % r["nprofs"] if r["budget"] else "no", r["step"]["median_ms"], r["step"]["min_ms"], r["step"]["max_ms"],
            r["sample"]["median_ms"], r["sample"]["min_ms"], r["sample"]["max_ms"]))
    by = {(r["masks"], r["budget"]): r["sample"]["median_ms"] for r in res["runs"]}
    step = statistics.median(r["step"]["median_ms"] for r in res["runs"])
    lines += ["", "The budget adds %.2f ms to a sample under one mask and %.2f ms under three: %.1f and %.1f steps of %.2f ms."
              % (by[(1, True)] - by[(1, False)], by[(3, True)] - by[(3, False)], (by[(1, True)] - by[(1, False)])/step,
                 (by[(3, True)] - by[(3, False)])/step, step)]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from microhh_amd.budget import Budget2
    from microhh_amd.model import HotPath
    from microhh_amd.stats import Stats
    res = dict(case="drycblles", n=a.n, dtype="f64", calls=a.calls, repeats=a.repeats, warmup=a.warmup, runs=[])
    for masks in (("default",), ("default", "wplus", "wmin")):
        for with_budget in (False, True):
            hp = HotPath("drycblles", a.n, a.n, a.n, dtype=np.float64, stats=Stats(masks=masks), budget=Budget2() if with_budget else None)
            for _ in range(2):
                hp.step()
            step = timed(hp.step, hp.sync, a.calls, a.warmup, a.repeats)
            sample = timed(hp.stats.sample, hp.sync, a.calls, a.warmup, a.repeats)
            res["runs"].append(dict(masks=len(masks), budget=with_budget, nprofs=len(hp.budget.names) if with_budget else 0, step=step, sample=sample))
            hp.close()
            del hp
    print(json.dumps(res))
    if a.write:
        doc = open(DOC).read()
        i, j = doc.index(BEGIN) + len(BEGIN), doc.index(END)
        open(DOC, "w").write(doc[:i] + "\n" + table(res) + "\n" + doc[j:])


if __name__ == "__main__":
    main()
