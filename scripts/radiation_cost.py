"""Cost of the GCSS radiation: mhh_radiation_gcss_exec in its two forms, and the dycoms step with and without it.

    python scripts/radiation_cost.py [--grids 256x256x256 512x512x128] [--step 256] [--out profiles/radiation_gcss.jsonl]

Per grid (fp64 unless the grid says `:float32`), on the synthetic stratocumulus field of radiation.synthetic_stratocumulus by day
(noon of day 160 at 32.5 N): the sweep form and the plain form of mhh_radiation_gcss_exec with both parts on, alternated in the same
process, once with ql handed in and once with ql = NULL (the saturation adjustment into scratch 0, as HotPath calls it): the median of
15 windows of `reps` calls timed with device events (reps chosen so that a window lasts about 50 ms), and the bandwidth that time means
on the algorithmic bytes of the sweep form with ql handed in: 7 array passes per cell (up: ql, qt read, flx_up written; down: flx_up,
ql read, thlt read and written), 56 B in fp64. The two forms' results are compared bit for bit at every size timed. Then one step() of
HotPath("dycoms", N, N, N, thermo=Moist, micro=Warm2mom) with and without radiation=Gcss in the same process, and exec alone. Every
call's return code is checked. One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEP, PLAIN = 0, 1
PASSES = 7
NOON = 160.5


def median_ms(torch, fn, n=15, warmup=3, reps=1):
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="*", default=["256x256x256", "512x512x128"])
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from microhh_amd import capi, microphys, radiation, thermo
    from microhh_amd.grid import Grid
    from microhh_amd.model import CASES
    cfg = CASES["dycoms"]
    lib = capi.lib()
    dev = torch.device("cuda:0")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)     # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    for spec in args.grids:
        parts = spec.split(":")
        shape = tuple(int(x) for x in parts[0].split("x"))
        dtype = np.dtype(parts[1] if len(parts) > 1 else "float64").type
        g = Grid(shape[0], shape[1], shape[2], *cfg["size"], order=2, igc=3, jgc=3, kgc=1, dtype=dtype)
        G = g.device_struct(dev)
        zc = g.z[g.kstart:g.kend].astype(np.float64)
        thl0, qt0 = radiation.dycoms_profiles(zc)
        bs = thermo.base_state(lib, g, thl0, qt0, cfg["pbot"])
        tab = {n: up(bs[n]) for n in ("rhoref", "pref", "exnref")}
        thl_i, qt_i = radiation.synthetic_stratocumulus(zc, (g.kmax, g.jmax, g.imax), np.random.RandomState(3))

        def field(a):
            full = np.zeros(g.shape3, dtype=dtype)
            full[g.interior] = a
            full[:g.kstart] = full[g.kstart]; full[g.kend:] = full[g.kend-1]
            return up(full)
        thl, qt = field(thl_i), field(qt_i)
        del thl_i, qt_i
        tt = thl.dtype
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ql = torch.zeros(g.shape3, dtype=tt, device=dev)
        capi.check(lib.mhh_thermo_moist_fields(G, P(thl), P(qt), P(tab["pref"]), P(tab["exnref"]), None, None, P(ql), None, None, P(count), stream()))
        torch.cuda.synchronize()
        cloudy = float((ql[g.interior] > 1e-5).any(dim=0).float().mean())
        mu = C.c_double(0)
        capi.check(lib.mhh_radiation_gcss_zenith_host(g.dtype, cfg["lat"], cfg["lon"], NOON, C.byref(mu)))
        p = capi.MhhRadiationGcssParams(cfg["xka"], cfg["fr0"], cfg["fr1"], cfg["div"], mu.value, radiation.LW | radiation.SW)
        scratch = torch.zeros((2, g.ncells), dtype=tt, device=dev)
        sp = (C.c_void_p*2)(*[scratch[n].data_ptr() for n in range(2)])
        ncell = g.imax*g.jmax*g.kmax
        nbytes = PASSES*np.dtype(dtype).itemsize*ncell
        head = dict(shape=list(shape), dtype=np.dtype(dtype).name, mu=mu.value, cloudy_columns=round(cloudy, 4))
        thlt = {impl: torch.zeros(g.shape3, dtype=tt, device=dev) for impl in (SWEEP, PLAIN)}
        for fed in (True, False):
            def call(impl):
                capi.check(lib.mhh_radiation_gcss_exec_impl(G, impl, C.byref(p), P(thlt[impl]), P(ql) if fed else None, P(thl), P(qt), P(tab["rhoref"]),
                                                            P(tab["pref"]), P(tab["exnref"]), None, None, sp, P(count), stream()))
            for t in thlt.values():
                t.zero_()
            call(SWEEP); call(PLAIN); torch.cuda.synchronize()
            same = bool(torch.equal(thlt[SWEEP], thlt[PLAIN])) and bool((thlt[SWEEP] != 0).any())
            once, _, _ = median_ms(torch, lambda: call(SWEEP), n=3)
            reps = max(1, int(50. / max(once, 1e-3)))
            res = {}
            for rnd in range(2):                      # alternate the two forms, twice: the spread between the rounds is the noise
                for impl, name in ((SWEEP, "sweep"), (PLAIN, "plain")):
                    res.setdefault(name, []).append(median_ms(torch, lambda: call(impl), reps=reps))
            row = dict(head, name="exec", ql="handed in" if fed else "NULL", same_bits=same, nonconverged=int(count.cpu()[0]), reps=reps,
                       algorithmic_bytes_per_cell=PASSES*np.dtype(dtype).itemsize)
            for name in ("sweep", "plain"):
                ms = min(r[0] for r in res[name])
                row[name + "_ms"] = round(ms, 4); row[name + "_ms_rounds"] = [round(r[0], 4) for r in res[name]]
                row[name + "_TBps_on_%d_passes" % PASSES] = round(nbytes / (ms*1e-3) / 1e12, 3)
            emit(row)
        del thl, qt, ql, scratch, thlt
        torch.cuda.empty_cache()

    if args.step:
        from microhh_amd.model import HotPath
        n, ms = args.step, {}
        thl0, qt0 = radiation.dycoms_profiles((np.arange(n) + 0.5)*cfg["size"][2]/n)
        for rad in (False, True):
            hp = HotPath("dycoms", n, n, n, dt=2., thermo=thermo.Moist(cfg["pbot"], thl0=thl0, qt0=qt0), micro=microphys.Warm2mom(cfg["Nc0"], dt=6.),
                         radiation=radiation.Gcss(cfg["xka"], cfg["fr0"], cfg["fr1"], cfg["div"], cfg["lat"], cfg["lon"], NOON) if rad else None)
            ms[rad] = median_ms(torch, hp.step)[0]
            if rad:
                ms["exec"] = median_ms(torch, hp.radiation.exec, reps=10)[0]
            hp.thermo.check()
            hp.close(); del hp
            torch.cuda.empty_cache()
        emit(dict(name="step", shape=[n, n, n], dtype="float64", step_ms=round(ms[False], 4), step_with_radiation_ms=round(ms[True], 4),
                  exec_ms=round(ms["exec"], 4), share_of_step=round((ms[True] - ms[False]) / ms[False], 4)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
