"""Cost of the Buffer / Force passes and of the horizontal means against mhh_thermo_buoy_tend in the same process.

    python scripts/force_cost.py [--grids drycbl:256 drycbl:512 gabls1:1024x1024x256:float32] [--out profiles/force_cost.jsonl]

Per grid: every new pass alone, the fused pass, and the yardstick, each as the median of 20 calls timed with device events. Every
call's return code is checked, so a refused call stops the script instead of being timed as a no-op. One JSON line per pass with
  tb_per_s          achieved bytes/s on the ALGORITHMIC bytes (s = bytes per value): s per cell and field for a mean, 6s per cell for
                    Coriolis, 2s per field over the buffer levels for the sponge (the tendency's read-modify-write), 3s per cell for
                    the buoyancy tendency (24 B/cell in fp64);
  traffic_tb_per_s  the same on what the pass moves: the sponge also reads the field (3s per field and buffer cell); in the fused
                    pass the sponge on u and v rides on Coriolis' loads and stores and only w and the scalars add their 3s;
  vs_yardstick      tb_per_s over the yardstick's tb_per_s in that run (the streaming passes are expected at 0.85 or more),
then one summary line per grid: the fused pass against buffer + force."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

YARDSTICK = "thermo_buoy_tend"


def median_ms(torch, fn, n=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _grid(spec):
    parts = spec.split(":")
    d = [int(x) for x in parts[1].split("x")]
    return parts[0], tuple(d * 3 if len(d) == 1 else d), np.dtype(parts[2] if len(parts) > 2 else "float64").type


def make(case, shape, dtype, **kw):
    """A HotPath of the case with gabls1's switches: the sponge over the top quarter relaxing to the mean profiles, Coriolis."""
    from microhh_amd.forcing import Forcing
    from microhh_amd.model import CASES, HotPath
    cfg = CASES[case]
    kcells = shape[2] + 2 * cfg["gc"][2]
    rs = np.random.RandomState(1)
    ug, vg = rs.random_sample(kcells), rs.random_sample(kcells)
    return HotPath(case, *shape, dtype=dtype, forcing=Forcing(swbuffer=True, zstart=0.75 * cfg["size"][2], swupdate=True, swlspres="geo",
                                                              fc=1.39e-4, ug=ug, vg=vg), **kw)


def passes(hp):
    """{name: (call, algorithmic bytes, bytes moved)}; every call checks its return code."""
    lib, F, fo, g, ok = hp.lib, C.byref(hp.fields), hp.forcing, hp.grid, hp._ok
    s = g.np_dtype.itemsize
    cells = g.itot * g.jtot * g.ktot
    level = g.itot * g.jtot
    nf = 3 + len(hp.s)
    buf_cells = level * (g.kend - fo.bparams.bufferkstart)             # w starts at bufferkstarth: at most one level off
    sums = hp.torch.zeros(2, device=hp.device, dtype=hp.torch.float64)
    one, prof1, two = hp._ptrs([hp.u]), hp._ptrs([fo.mean_prof["u"]]), hp._ptrs([hp.u, hp.ut])
    scratch, order = fo.scratch.data_ptr(), hp.cfg["order"]
    return {
        "mean_profile_1": (lambda: ok(lib.mhh_field_mean_profile(hp.G, one, 1, prof1, scratch, hp.stream)), s * level * g.kcells, s * level * g.kcells),
        "mean_profile_all": (fo.means, s * nf * level * g.kcells, s * nf * level * g.kcells),
        "mean_sum_2": (lambda: ok(lib.mhh_field_mean_sum(hp.G, two, 2, sums.data_ptr(), scratch, hp.stream)), 2 * s * cells, 2 * s * cells),
        "buffer": (lambda: ok(lib.mhh_buffer_exec(hp.G, F, C.byref(fo.bparams), hp.stream)), 2 * s * nf * buf_cells, 3 * s * nf * buf_cells),
        "force_geo": (lambda: ok(lib.mhh_force_exec(hp.G, F, C.byref(fo.fparams), hp.stream)), 6 * s * cells, 6 * s * cells),
        "fused": (fo.exec, 6 * s * cells + 2 * s * nf * buf_cells, 6 * s * cells + 3 * s * (nf - 2) * buf_cells),
        YARDSTICK: (lambda: ok(lib.mhh_thermo_buoy_tend(hp.G, order, F, 0, 0., 0., 0., hp.stream)), 3 * s * cells, 3 * s * cells),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["drycbl:256", "drycbl:512", "gabls1:1024x1024x256:float32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for spec in args.grids:
        case, shape, dtype = _grid(spec)
        hp = make(case, shape, dtype)
        head = dict(case=case, shape=list(shape), dtype=np.dtype(dtype).name)
        rows = {}
        for name, (fn, nbytes, moved) in passes(hp).items():
            ms = median_ms(torch, fn)
            rows[name] = dict(head, name=name, ms=round(ms, 4), bytes=nbytes, tb_per_s=round(nbytes / ms * 1e-9, 3), traffic_tb_per_s=round(moved / ms * 1e-9, 3))
        for r in rows.values():
            r["vs_yardstick"] = round(r["tb_per_s"] / rows[YARDSTICK]["tb_per_s"], 3)
            emit(r)
        parts = rows["buffer"]["ms"] + rows["force_geo"]["ms"]
        emit(dict(head, name="fused_vs_parts", fused_ms=rows["fused"]["ms"], buffer_plus_force_ms=round(parts, 4), ratio=round(rows["fused"]["ms"] / parts, 3)))
        hp.close(); del hp
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
