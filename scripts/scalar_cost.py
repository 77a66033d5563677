"""What a scalar beyond the first costs in the (advec_2i5, diff_smag2) RHS on one GPU.

Times HotPath.rhs() (fused: mhh_rhs_exec) and HotPath.rhs_unfused() (mhh_advec_exec + mhh_diff_exec) with HIP events for
drycblles at 256^3 and 512^3 (fp64) with 1, 2 and 3 scalars, with the scalar pass of the marching kernel (default) and with
MHH_SCALAR_IMPL=cell (scalars 1, 2 in the per-field cell kernels), all in the same process. Every grid first runs the fused
call for --settle seconds untimed (the first timed calls of a process otherwise run before the engine clock has settled). One
JSON line per configuration (median of --reps calls after --warmup calls), then one summary line per size and scalar count:
the cost of each extra scalar against the one-scalar fused call. With one scalar every form runs the same kernels: the
one-scalar baseline is the median over the forms.

    python scripts/scalar_cost.py [--sizes 256 512] [--nscalars 1 2 3] [--reps 10] [--warmup 3] [--settle 1.0] [--batch1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--nscalars", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of untimed fused calls on every grid before its first timing")
    ap.add_argument("--batch1", action="store_true", help="also time the scalar pass one scalar per launch (MHH_SCALAR_BATCH=1)")
    a = ap.parse_args()
    import torch
    from microhh_amd.model import HotPath
    impls = [("pass", {}), ("cell", {"MHH_SCALAR_IMPL": "cell"})] + ([("pass1", {"MHH_SCALAR_BATCH": "1"})] if a.batch1 else [])
    for n in a.sizes:
        res = {}
        for nsc in a.nscalars:
            hp = HotPath("drycblles", n, n, n, device="cuda:0", nscalars=nsc)
            hp.cyclic_prognostic(); hp.exec_viscosity(); hp.sync()
            _settle(hp, a.settle)
            for impl, env in impls:
                old = {k: os.environ.get(k) for k in env}
                os.environ.update(env)
                try:
                    line = {"case": "drycblles", "n": n, "dtype": "float64", "nscalars": nsc, "scalar_impl": impl,
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
