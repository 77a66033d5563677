"""What Thermo_buoy costs in the hot path on one GPU, folded and on its own.

For the Thermo_buoy cases of microhh_amd.model (scalar 0 is the buoyancy b), times with HIP events (median of --reps calls after
--warmup calls, fp64, every grid first runs --settle seconds of untimed calls):
  * the RHS pass with the flat buoyancy folded in (HotPath.rhs(): mhh_rhs_exec, buoyancy_kind = 1), against the separate launch
    (mhh_thermo_buoy_tend, then mhh_rhs_exec without buoyancy) and against the pass without any buoyancy: the rhs25 marching kernel
    for sbl, the rhs44 marching kernel (a register window of b) for drycbl;
  * the stand-alone mhh_thermo_buoy_tend (flat form) by itself;
  * exec_viscosity with the N2 of b evaluated inside it, against N2 through a pointer: mhh_thermo_buoy_N2 into a 3-D field first
    (get_thermo_field("N2")) and that field read by exec_viscosity (diff_smag2 cases only).
One JSON line per grid.

    python scripts/buoy_cost.py [--grids sbl:256 sbl:512 drycbl:512x256x256 drycbl:1024x1x384] [--reps 20] [--warmup 3] [--settle 1.0]
"""
import argparse
import ctypes as C
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


def _shape(s):
    name, dims = s.split(":")
    d = [int(x) for x in dims.split("x")]
    return name, (d * 3 if len(d) == 1 else d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["sbl:256", "sbl:512", "drycbl:512x256x256", "drycbl:1024x1x384"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    from microhh_amd.model import HotPath
    from microhh_amd.grid import DIFF_SMAG2
    for spec in a.grids:
        case, shape = _shape(spec)
        hp = HotPath(case, *shape, device="cuda:0")
        lib, p, F, P = hp.lib, hp.params, C.byref(hp.fields), C.byref(hp.params)
        order = p.buoyancy
        hp.cyclic_prognostic(); hp.exec_viscosity(); hp.sync()

        def alone():
            hp._ok(lib.mhh_thermo_buoy_tend(hp.G, order, F, 0, 0., 0., 0., hp.stream))

        def rhs_plain():
            p.buoyancy = 0
            try:
                hp.rhs()
            finally:
                p.buoyancy = order

        def rhs_separate():
            alone(); rhs_plain()
        t0 = time.time()
        while time.time() - t0 < a.settle:
            for _ in range(5):
                hp.rhs()
            hp.sync()
        line = {"case": case, "shape": list(shape), "dtype": "float64", "order": order,
                "rhs_fold_ms": round(_time(hp, hp.rhs, a.reps, a.warmup), 4),
                "rhs_separate_ms": round(_time(hp, rhs_separate, a.reps, a.warmup), 4),
                "rhs_no_buoyancy_ms": round(_time(hp, rhs_plain, a.reps, a.warmup), 4),
                "buoy_tend_alone_ms": round(_time(hp, alone, a.reps, a.warmup), 4)}
        line["fold_cost_ms"] = round(line["rhs_fold_ms"] - line["rhs_no_buoyancy_ms"], 4)
        line["fold_saves_ms"] = round(line["rhs_separate_ms"] - line["rhs_fold_ms"], 4)
        if hp.cfg["diff"] == DIFF_SMAG2:
            n2 = torch.empty_like(hp.evisc)

            def visc_pointer():
                hp._ok(lib.mhh_thermo_buoy_N2(hp.G, n2.data_ptr(), hp.s[0].data_ptr(), p.bg_n2, hp.stream))
                p.N2 = n2.data_ptr()
                try:
                    hp._ok(lib.mhh_diff_exec_viscosity(hp.G, DIFF_SMAG2, F, P, hp.stream))
                finally:
                    p.N2 = None
            line["visc_inline_N2_ms"] = round(_time(hp, hp.exec_viscosity, a.reps, a.warmup), 4)
            line["visc_N2_pointer_incl_calc_N2_ms"] = round(_time(hp, visc_pointer, a.reps, a.warmup), 4)
            line["inline_saves_ms"] = round(line["visc_N2_pointer_incl_calc_N2_ms"] - line["visc_inline_N2_ms"], 4)
        print(json.dumps(line), flush=True)
        hp.close(); del hp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
