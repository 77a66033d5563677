"""Cost of the ice microphysics: the kernels of Microphys_nsw6::exec in both forms of the powers.

    python scripts/nsw6_cost.py [--grids 512x512x128 512x512x128:float32] [--out profiles/microphys_nsw6.jsonl]

Per grid (fp64 unless the grid says `:float32`), on the synthetic deep-convection field (thermo.rcemip_interior with
microphys.synthetic_precip on the domain of cases/rcemip): the conversion kernel alone in the forms NSW6_POW and NSW6_SQRT, with ql
and qi given (from mhh_thermo_moist_fields) and with sat_adjust inline, then the sedimentation of the three species alone (and, in NSW6_SQRT, as
one launch against one launch per species: each call's launch carries three slices in z, those of the species outside the mask return
at once), the forms alternated in the same process: the median of 15 windows of `reps` calls timed with device events (reps chosen so that a window lasts
about 50 ms), twice; the smaller median counts and both are printed. Beside them: a device-to-device copy that moves the 15 array
passes of conversion with sat_adjust inline (five fields read, five tendencies read and written: 120 B per cell in fp64), and
mhh_micro_2mom_warm_exec with every process on, on the synthetic RICO field of the same shape (scripts/micro_cost.py). The two forms'
tendencies are compared at every size timed (the largest difference relative to each array's maximum). Every call's return code is
checked. One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PBOT, NC0, DT = 101480., 100.e6, 6.
POW, SQRT = 0, 1
CONV, SEDI = 1, 2 | 4 | 8
PASSES_CONV, PASSES_SEDI = 15, 24          # sedimentation per species: q read, CFL and slope written and read back, tendency read and written, ~8


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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="*", default=["512x512x128", "512x512x128:float32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from microhh_amd import capi, microphys, thermo
    from microhh_amd.grid import Grid
    lib = capi.lib()
    dev = torch.device("cuda:0")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)     # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None         # noqa: E731
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    def timed(calls, once_of):
        """calls: {name: fn}. Alternated, two rounds; returns {name: (best median, [rounds])} and the reps used."""
        torch.cuda.synchronize()
        once = median_ms(torch, calls[once_of], n=3)
        reps = max(1, int(50. / max(once, 1e-3)))
        res = {}
        for _ in range(2):
            for name, fn in calls.items():
                res.setdefault(name, []).append(median_ms(torch, fn, reps=reps))
        return {k: (min(v), [round(x, 4) for x in v]) for k, v in res.items()}, reps

    for spec in args.grids:
        parts = spec.split(":")
        shape = tuple(int(x) for x in parts[0].split("x"))
        dtype = np.dtype(parts[1] if len(parts) > 1 else "float64").type
        size = np.dtype(dtype).itemsize
        head = dict(shape=list(shape), dtype=np.dtype(dtype).name)
        n3i = (shape[2], shape[1], shape[0])

        def ghosted(g, a):
            full = np.zeros(g.shape3, dtype=dtype)
            full[g.interior] = a
            full[:g.kstart] = full[g.kstart]; full[g.kend:] = full[g.kend-1]
            return up(full)

        # ---- Microphys_nsw6 on the deep-convection field
        g = Grid(shape[0], shape[1], shape[2], 12800., 12800., 32250., order=2, igc=3, jgc=3, kgc=1, dtype=dtype)
        G = g.device_struct(dev)
        ncell = g.imax*g.jmax*g.kmax
        z = g.z[g.kstart:g.kend]
        bs = thermo.base_state(lib, g, *thermo.rcemip_profiles(z), PBOT)
        tab = [up(bs[n]) for n in ("rhoref", "pref", "exnref", "thvref")]
        rs = np.random.RandomState(2)
        thl, qt = (ghosted(g, a) for a in thermo.rcemip_interior(z, n3i, rs))
        q = [ghosted(g, a) for a in microphys.synthetic_precip(z, n3i, rs)]
        tt = thl.dtype
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ql, qi = torch.zeros(g.shape3, dtype=tt, device=dev), torch.zeros(g.shape3, dtype=tt, device=dev)
        capi.check(lib.mhh_thermo_moist_fields(G, P(thl), P(qt), P(tab[1]), P(tab[2]), P(tab[3]), None, P(ql), P(qi), None, P(count), stream()), lib)
        scratch = torch.zeros((6, g.ncells), dtype=tt, device=dev)
        sp = (C.c_void_p*6)(*[scratch[n].data_ptr() for n in range(6)])
        tend = {impl: [torch.zeros(g.shape3, dtype=tt, device=dev) for _ in range(5)] for impl in (POW, SQRT)}
        bot = torch.zeros((3,) + tuple(g.shape2), dtype=tt, device=dev)
        share = {n: round(float((a[g.interior] > lim).float().mean()), 4) for n, a, lim in
                 (("ql", ql, 1e-7), ("qi", qi, 1e-7), ("qr", q[0], 1e-12), ("qs", q[1], 1e-12), ("qg", q[2], 1e-12))}
        busy = (ql > 1e-7) | (qi > 1e-7) | (q[0] > 1e-12) | (q[1] > 1e-12) | (q[2] > 1e-12)
        share["busy"] = round(float(busy[g.interior].float().mean()), 4)
        del busy

        def call(impl, mask, given):
            p = capi.MhhMicroParams(NC0, DT, mask)
            t = tend[impl]
            capi.check(lib.mhh_micro_nsw6_exec_impl(G, impl, C.byref(p), P(q[0]), P(q[1]), P(q[2]), P(thl), P(qt), P(ql) if given else None,
                                                    P(qi) if given else None, P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), P(bot[0]), P(bot[1]), P(bot[2]),
                                                    P(tab[0]), P(tab[1]), P(tab[2]), sp, P(count), stream()), lib)

        for given in (True, False):
            for t in tend[POW] + tend[SQRT]:
                t.zero_()
            call(POW, CONV, given); call(SQRT, CONV, given); torch.cuda.synchronize()
            diff = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(tend[POW], tend[SQRT]))
            res, reps = timed({"pow": lambda: call(POW, CONV, given), "sqrt": lambda: call(SQRT, CONV, given)}, "pow")
            nbytes = (PASSES_CONV + (2 if given else 0))*size*ncell
            row = dict(head, name="conversion", ql_qi="given" if given else "sat_adjust inline", share=share, reps=reps, sqrt_vs_pow_rel=diff,
                       nonconverged=int(count.cpu()[0]), algorithmic_bytes_per_cell=(PASSES_CONV + (2 if given else 0))*size)
            for k, (ms, rounds) in res.items():
                row[k + "_ms"] = round(ms, 4); row[k + "_ms_rounds"] = rounds
                row[k + "_TBps"] = round(nbytes / (ms*1e-3) / 1e12, 3)
            emit(row)
        res, reps = timed({"pow": lambda: call(POW, SEDI, True), "sqrt": lambda: call(SQRT, SEDI, True)}, "pow")
        row = dict(head, name="sedimentation", species=3, launches=1, reps=reps, algorithmic_bytes_per_cell=PASSES_SEDI*size)
        for k, (ms, rounds) in res.items():
            row[k + "_ms"] = round(ms, 4); row[k + "_ms_rounds"] = rounds
            row[k + "_TBps"] = round(PASSES_SEDI*size*ncell / (ms*1e-3) / 1e12, 3)
        emit(row)

        def by_species():
            for m in (2, 4, 8):
                call(SQRT, m, True)
        res, reps = timed({"one_launch": lambda: call(SQRT, SEDI, True), "three_launches": by_species}, "one_launch")
        emit(dict(head, name="sedimentation launches", form="sqrt", reps=reps, **{k + "_ms": round(v[0], 4) for k, v in res.items()},
                  **{k + "_ms_rounds": v[1] for k, v in res.items()}))
        out = C.c_double(0)
        work = torch.zeros(16, dtype=torch.float64, device=dev)

        def cfl():
            capi.check(lib.mhh_micro_nsw6_cfl(G, P(q[0]), P(q[1]), P(q[2]), P(tab[0]), DT, P(work), C.byref(out), stream()), lib)
        emit(dict(head, name="cfl", with_readback_ms=round(median_ms(torch, cfl, reps=5), 4), cfl=out.value))
        # ---- the copy that moves conversion's 15 array passes: 7.5 arrays read, 7.5 written
        n = (PASSES_CONV*ncell)//2
        del tend, scratch
        src, dst = torch.zeros(n, dtype=tt, device=dev), torch.empty(n, dtype=tt, device=dev)
        once = median_ms(torch, lambda: dst.copy_(src), n=3)
        ms = median_ms(torch, lambda: dst.copy_(src), reps=max(1, int(50. / max(once, 1e-3))))
        emit(dict(head, name="copy", bytes_per_cell=PASSES_CONV*size, ms=round(ms, 4), TBps=round(2*n*size / (ms*1e-3) / 1e12, 3)))
        del src, dst, ql, qi, q, thl, qt
        torch.cuda.empty_cache()

        # ---- Microphys_2mom_warm on the synthetic RICO field of the same shape
        g = Grid(shape[0], shape[1], shape[2], 12800., 12800., 4000., order=2, igc=3, jgc=3, kgc=1, dtype=dtype)
        G = g.device_struct(dev)
        z = g.z[g.kstart:g.kend]
        bs = thermo.base_state(lib, g, *thermo.bomex_profiles(z), 101540.)
        tab = [up(bs[n]) for n in ("rhoref", "pref", "exnref")]
        thl_h, qt_h = thermo.bomex_synthetic(g, seed=1)
        thl, qt = up(thl_h), up(qt_h)
        del thl_h, qt_h
        qr, nr = (ghosted(g, a) for a in microphys.synthetic_rain(z, n3i, np.random.RandomState(2)))
        t4 = [torch.zeros(g.shape3, dtype=tt, device=dev) for _ in range(4)]
        rr = torch.zeros(g.shape2, dtype=tt, device=dev)
        scratch = torch.zeros((4, g.ncells), dtype=tt, device=dev)
        sp4 = (C.c_void_p*4)(*[scratch[n].data_ptr() for n in range(4)])
        p = capi.MhhMicroParams(70.e6, DT, microphys.ALL)

        def warm():
            capi.check(lib.mhh_micro_2mom_warm_exec(G, C.byref(p), P(qr), P(nr), P(thl), P(qt), P(t4[0]), P(t4[1]), P(t4[2]), P(t4[3]), P(rr), P(tab[0]),
                                                    P(tab[1]), P(tab[2]), sp4, P(count), stream()), lib)
        once = median_ms(torch, warm, n=3)
        ms = median_ms(torch, warm, reps=max(1, int(50. / max(once, 1e-3))))
        emit(dict(head, name="micro_2mom_warm_exec", ms=round(ms, 4)))
        del thl, qt, qr, nr, t4, scratch
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
