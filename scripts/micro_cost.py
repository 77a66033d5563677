"""Cost of the warm-rain microphysics: Microphys_2mom_warm::exec in its two forms, and the step with and without it.

    python scripts/micro_cost.py [--grids 256x256x256 512x512x512] [--step 256] [--out profiles/microphys_2mom_warm.jsonl]

Per grid (fp64 unless the grid says `:float32`), on two fields -- the synthetic RICO field (thermo.bomex_synthetic on RICO's domain
with microphys.synthetic_rain: rain in about half of the columns) and the same without rain (qr = nr = 0: autoconversion alone has
work) -- the marching form and the one-thread-per-cell form of mhh_micro_2mom_warm_exec with every process on, alternated in the same
process: the median of 15 windows of `reps` calls timed with device events (reps chosen so that a window lasts about 50 ms), and the
bandwidth that time means on the algorithmic bytes of the marching form: 28 array passes per cell (pass A: qr, nr, thl, qt read, four
tendencies read and written, qr, nr and four scratch arrays written = 18; pass B: qr, nr and the four scratch arrays read, qrt and
nrt read and written = 10; what the gathers re-read of the levels above is left to the caches), 224 B in fp64. The two forms'
results are compared bit for bit at every size timed. The sedimentation CFL number is timed with its host read-back. Then one step()
of HotPath("rico", N, N, N, thermo=Moist) with and without micro=Warm2mom in the same process, and exec and limit alone. Every call's
return code is checked. One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PBOT, NC0, DT = 101540., 70.e6, 6.
MARCH, CELL = 0, 1
PASSES = 28


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
    ap.add_argument("--grids", nargs="*", default=["256x256x256", "512x512x512"])
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from microhh_amd import capi, microphys, thermo
    from microhh_amd.grid import Grid
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
        g = Grid(shape[0], shape[1], shape[2], 12800., 12800., 4000., order=2, igc=3, jgc=3, kgc=1, dtype=dtype)
        G = g.device_struct(dev)
        thl0, qt0 = thermo.bomex_profiles(g.z[g.kstart:g.kend])
        bs = thermo.base_state(lib, g, thl0, qt0, PBOT)
        tab = [up(bs[n]) for n in ("rhoref", "pref", "exnref")]
        thl_h, qt_h = thermo.bomex_synthetic(g, seed=1)
        thl, qt = up(thl_h), up(qt_h)
        del thl_h, qt_h
        qr_i, nr_i = microphys.synthetic_rain(g.z[g.kstart:g.kend], (g.kmax, g.jmax, g.imax), np.random.RandomState(2))
        ncell = g.imax*g.jmax*g.kmax
        nbytes = PASSES*np.dtype(dtype).itemsize*ncell
        head = dict(shape=list(shape), dtype=np.dtype(dtype).name)
        tt = thl.dtype
        scratch = torch.zeros((4, g.ncells), dtype=tt, device=dev)
        sp = (C.c_void_p*4)(*[scratch[n].data_ptr() for n in range(4)])
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        work = torch.zeros(16, dtype=torch.float64, device=dev)
        for fname in ("rico", "rain_free"):
            def field(a):
                full = np.zeros(g.shape3, dtype=dtype)
                if fname == "rico":
                    full[g.interior] = a
                    full[:g.kstart] = full[g.kstart]; full[g.kend:] = full[g.kend-1]
                return up(full)
            qr0, nr0 = field(qr_i), field(nr_i)
            rain_share = float((qr0[g.interior] > 1e-15).float().mean())
            p = capi.MhhMicroParams(NC0, DT, microphys.ALL)
            st = {impl: dict(qr=qr0.clone(), nr=nr0.clone(), t=[torch.zeros(g.shape3, dtype=tt, device=dev) for _ in range(4)],
                             rr=torch.zeros(g.shape2, dtype=tt, device=dev)) for impl in (MARCH, CELL)}

            def call(impl):
                s = st[impl]
                capi.check(lib.mhh_micro_2mom_warm_exec_impl(G, impl, C.byref(p), P(s["qr"]), P(s["nr"]), P(thl), P(qt), P(s["t"][0]), P(s["t"][1]),
                                                             P(s["t"][2]), P(s["t"][3]), P(s["rr"]), P(tab[0]), P(tab[1]), P(tab[2]), sp, P(count), stream()))
            call(MARCH); call(CELL); torch.cuda.synchronize()
            same = all(bool(torch.equal(a, b)) for a, b in zip(st[MARCH]["t"] + [st[MARCH]["rr"]], st[CELL]["t"] + [st[CELL]["rr"]]))
            once, _, _ = median_ms(torch, lambda: call(MARCH), n=3)
            reps = max(1, int(50. / max(once, 1e-3)))
            res = {}
            for rnd in range(2):                      # alternate the two forms, twice: the spread between the rounds is the noise
                for impl, name in ((MARCH, "march"), (CELL, "cell")):
                    res.setdefault(name, []).append(median_ms(torch, lambda: call(impl), reps=reps))
            row = dict(head, name="exec", field=fname, rain_share=round(rain_share, 4), same_bits=same, nonconverged=int(count.cpu()[0]), reps=reps,
                       algorithmic_bytes_per_cell=PASSES*np.dtype(dtype).itemsize)
            for name in ("march", "cell"):
                ms = min(r[0] for r in res[name])
                row[name + "_ms"] = round(ms, 4); row[name + "_ms_rounds"] = [round(r[0], 4) for r in res[name]]
                row[name + "_TBps_on_%d_passes" % PASSES] = round(nbytes / (ms*1e-3) / 1e12, 3)
            out = C.c_double(0)

            def cfl():
                capi.check(lib.mhh_micro_2mom_warm_cfl(G, P(qr0), P(nr0), P(tab[0]), DT, P(work), C.byref(out), stream()))
            row["cfl_with_readback_ms"] = round(median_ms(torch, cfl, reps=5)[0], 4)
            row["cfl"] = out.value
            emit(row)
            del st, qr0, nr0
            torch.cuda.empty_cache()
        del thl, qt, scratch
        torch.cuda.empty_cache()

    if args.step:
        from microhh_amd.model import HotPath
        n, ms = args.step, {}
        for micro in (False, True):
            hp = HotPath("rico", n, n, n, dt=2., thermo=thermo.Moist(PBOT), micro=microphys.Warm2mom(NC0, dt=DT) if micro else None)
            ms[micro] = median_ms(torch, hp.step)[0]
            if micro:
                ms["exec"] = median_ms(torch, hp.micro.exec, reps=10)[0]
                ms["limit"] = median_ms(torch, hp.micro.limit, reps=10)[0]
            hp.thermo.check()
            hp.close(); del hp
            torch.cuda.empty_cache()
        emit(dict(name="step", shape=[n, n, n], dtype="float64", step_ms=round(ms[False], 4), step_with_micro_ms=round(ms[True], 4),
                  exec_ms=round(ms["exec"], 4), limit_ms=round(ms["limit"], 4), share_of_step=round((ms[True] - ms[False]) / ms[False], 4)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
