"""What a scalar costs in the RHS on one GPU: one beyond the first in (advec_2i5, diff_smag2), any one in (advec_4, diff_4).

Times HotPath.rhs() (fused: mhh_rhs_exec) and HotPath.rhs_unfused() (mhh_advec_exec + mhh_diff_exec) with HIP events for
drycblles at 256^3 and 512^3 (fp64) with 1, 2 and 3 scalars, with the scalar pass of the marching kernel (default) and with
MHH_SCALAR_IMPL=cell (scalars 1, 2 in the per-field cell kernels), all in the same process. Every grid first runs the fused
call for --settle seconds untimed (the first timed calls of a process otherwise run before the engine clock has settled). One
JSON line per configuration (median of --reps calls after --warmup calls), then one summary line per size and scalar count:
the cost of each extra scalar against the one-scalar fused call. With one scalar every form runs the same kernels: the
one-scalar baseline is the median over the forms.

    python scripts/scalar_cost.py [--sizes 256 512] [--nscalars 1 2 3] [--reps 10] [--warmup 3] [--settle 1.0] [--batch1]

--case drycbl times the fourth-order pair instead, whose marching kernel carries no scalar: every scalar takes its two per-field
kernels (MHH_SCALAR_IMPL=cell, and the default) or, MHH_SCALAR_IMPL=march, the scalar pass of k_march4.hip, so --nscalars may include 0 and the summary is the cost per
scalar against the call without scalars, (rhs(n) - rhs(0)) / n, for the pass, the pass one scalar per launch (MHH_SCALAR_BATCH=1)
and the per-field kernels, with the rate of the pass over its algorithmic traffic: u, v, w once per launch and s, st read, st
written per scalar, i.e. 6 array passes for a batch of one (48 B/cell in fp64), 9 for a batch of two (72 B/cell, 36 per scalar).
The rate is a lower bound: with buoyancy, rhs(n) - rhs(0) also holds the buoyancy of b (a fold into the u, v, w kernel or a launch
of its own), which a call without scalars does not have. --shapes takes grids that are not cubes:

    python scripts/scalar_cost.py --case drycbl --shapes 512x256x256 1024x1x384 --nscalars 0 1 2 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(hp, fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    hp.sync()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms)//2]


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs)//2] if len(xs) % 2 else 0.5*(xs[len(xs)//2 - 1] + xs[len(xs)//2])


def _settle(hp, seconds):
    t0 = time.time()
    while time.time() - t0 < seconds:
        for _ in range(5):
            hp.rhs()
        hp.sync()


def _summary_fourth(a, n, shape, impls, res):
    """(rhs(nsc) - rhs(0)) / nsc per form of the scalars, and the rate of the pass over its algorithmic traffic."""
    if 0 not in a.nscalars:
        return
    base = {form: _median([res[(0, impl)][form] for impl, _ in impls]) for form in ("rhs_ms", "rhs_unfused_ms")}
    cells = shape[0] * shape[1] * shape[2]
    for nsc in a.nscalars:
        if nsc == 0:
            continue
        summ = {"summary": "per_scalar", "n": n, "nscalars": nsc, "no_scalar_fused_ms": round(base["rhs_ms"], 4), "no_scalar_unfused_ms": round(base["rhs_unfused_ms"], 4)}
        for impl, _ in impls:
            for form in ("rhs_ms", "rhs_unfused_ms"):
                summ["%s_%s_per_scalar_ms" % (impl, form[:-3])] = round((res[(nsc, impl)][form] - base[form]) / nsc, 4)
        # array passes of the fused call's launches: batches of two and a last batch of one. dt also holds the buoyancy of b, which
        # exists only with a scalar, so the rate is biased low
        passes = (nsc // 2) * 9 + (nsc % 2) * 6
        dt = res[(nsc, "pass")]["rhs_ms"] - base["rhs_ms"]
        summ["pass_bytes_per_cell_per_scalar"] = round(8. * passes / nsc, 1)
        summ["pass_TB_per_s"] = round(8. * passes * cells / (dt * 1e-3) / 1e12, 3) if dt > 0 else None
        summ["cell_over_pass_per_scalar"] = round(summ["cell_rhs_per_scalar_ms"] / summ["pass_rhs_per_scalar_ms"], 2) if summ["pass_rhs_per_scalar_ms"] > 0 else None
        print(json.dumps(summ), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="drycblles", choices=["drycblles", "drycbl"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--shapes", nargs="+", default=None, help="grids as ITOTxJTOTxKTOT, e.g. 512x256x256 1024x1x384 (instead of --sizes)")
    ap.add_argument("--nscalars", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of untimed fused calls on every grid before its first timing")
    ap.add_argument("--batch1", action="store_true", help="also time the scalar pass one scalar per launch (MHH_SCALAR_BATCH=1)")
    a = ap.parse_args()
    import torch
    from microhh_amd.model import HotPath
    fourth = a.case == "drycbl"
    if fourth:       # the 4th-order pass is opt-in (MHH_SCALAR_IMPL=march); a build without it runs its per-field kernels in all three
        impls = [("pass", {"MHH_SCALAR_IMPL": "march"}), ("cell", {"MHH_SCALAR_IMPL": "cell"}), ("pass1", {"MHH_SCALAR_IMPL": "march", "MHH_SCALAR_BATCH": "1"})]
    else:
        impls = [("pass", {}), ("cell", {"MHH_SCALAR_IMPL": "cell"})] + ([("pass1", {"MHH_SCALAR_BATCH": "1"})] if a.batch1 else [])
    shapes = [tuple(int(x) for x in sh.split("x")) for sh in a.shapes] if a.shapes else [(n, n, n) for n in a.sizes]
    for shape in shapes:
        n = shape[0] if shape[0] == shape[1] == shape[2] else "x".join(str(x) for x in shape)
        res = {}
        for nsc in a.nscalars:
            hp = HotPath(a.case, *shape, device="cuda:0", nscalars=nsc)
            hp.cyclic_prognostic(); hp.exec_viscosity(); hp.sync()
            _settle(hp, a.settle)
            for impl, env in impls:
                old = {k: os.environ.get(k) for k in env}
                os.environ.update(env)
                try:
                    line = {"case": a.case, "n": n, "dtype": "float64", "nscalars": nsc, "scalar_impl": impl,
                            "rhs_ms": round(_time(hp, hp.rhs, a.reps, a.warmup), 4),
                            "rhs_unfused_ms": round(_time(hp, hp.rhs_unfused, a.reps, a.warmup), 4)}
                finally:
                    for k, v in old.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                res[(nsc, impl)] = line
                print(json.dumps(line), flush=True)
            hp.close(); del hp
            torch.cuda.empty_cache()
        if fourth:
            _summary_fourth(a, n, shape, impls, res)
            continue
        if 1 not in a.nscalars:
            continue
        base = {form: _median([res[(1, impl)][form] for impl, _ in impls]) for form in ("rhs_ms", "rhs_unfused_ms")}
        for nsc in a.nscalars:
            if nsc == 1:
                continue
            summ = {"summary": "extra_scalar", "n": n, "nscalars": nsc, "extra_scalars": nsc - 1,
                    "one_scalar_fused_ms": round(base["rhs_ms"], 4), "one_scalar_unfused_ms": round(base["rhs_unfused_ms"], 4)}
            for impl, _ in impls:
                for form in ("rhs_ms", "rhs_unfused_ms"):
                    summ["%s_%s_per_extra_scalar_ms" % (impl, form[:-3])] = round((res[(nsc, impl)][form] - base[form]) / (nsc - 1), 4)
            summ["pass_ratio_to_one_scalar_fused"] = round(summ["pass_rhs_per_extra_scalar_ms"] / base["rhs_ms"], 3)
            summ["cell_over_pass_per_extra_scalar"] = round(summ["cell_rhs_per_extra_scalar_ms"] / summ["pass_rhs_per_extra_scalar_ms"], 2)
            print(json.dumps(summ), flush=True)


if __name__ == "__main__":
    main()
