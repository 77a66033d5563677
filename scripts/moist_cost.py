"""Cost of the moist thermodynamics: the buoyancy tendency in its two forms, and the base state on the device.

    python scripts/moist_cost.py [--grids 256x256x256 512x512x512 256x256x256:float32] [--ktot 64 256 512] [--step 256] [--out profiles/thermo_moist.jsonl]

Per grid, on three fields -- the synthetic BOMEX field (microhh_amd.thermo.bomex_synthetic), the same with qt halved (no cell
saturated) and with 4 g/kg added between 500 and 1500 m (every cloud-layer cell saturated) -- the marching form and the
one-thread-per-cell form of mhh_thermo_moist_buoyancy_tend, alternated in the same process: the median of 15 windows of `reps`
calls timed with device events (reps chosen so that a window lasts about 50 ms), the bandwidth that time means on the 32 B/cell (fp64)
of the four array passes the marching form needs, the share of w-level cells that are saturated and the share of 64-cell row
segments (one wave of the marching form) with at least one such cell, from a pass of mhh_thermo_moist_sat_adjust over the w-level
values. The two forms' results are compared bit for bit at every size timed.
Then the base-state recurrence at each --ktot on the BOMEX profile: the device kernel (device events, windows of 20 calls) against
the reference's way on the same box -- two device-to-host copies of the mean profiles, the host entry, eight uploads and a
synchronise (host clock around the synchronised sequence). Then one step() of HotPath("bomex", N, N, N) with and without
thermo=Moist(pbot) in the same process, each without and with surface= and forcing= (BOMEX's fixed ustar and fluxes, subsidence
and drying; without thermo= the surface layer takes thl for Thermo_dry's th: a yardstick of cost only), and the thermodynamics' calls
alone (means, base state, tendency). Every call's return code
is checked. One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PBOT = 101500.
MARCH, CELL = 0, 1


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
    ap.add_argument("--grids", nargs="*", default=["256x256x256", "512x512x512", "256x256x256:float32"])
    ap.add_argument("--ktot", nargs="*", type=int, default=[64, 256, 512])
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from microhh_amd import capi, thermo
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
        g = Grid(shape[0], shape[1], shape[2], 6400., 6400., 3000., order=2, igc=3, jgc=3, kgc=1, dtype=dtype)
        G = g.device_struct(dev)
        thl0, qt0 = thermo.bomex_profiles(g.z[g.kstart:g.kend])
        bs = thermo.base_state(lib, g, thl0, qt0, PBOT)
        tab = [up(bs[n]) for n in ("prefh", "exnrefh", "thvrefh")]
        thl_h, qt_h = thermo.bomex_synthetic(g, seed=1)
        z = g.z.astype(np.float64)[:, None, None]
        layer = ((z > 500.) & (z < 1500.))
        fields = {"bomex": qt_h, "unsaturated": (0.5*qt_h).astype(dtype), "cloud_layer_saturated": (qt_h + 4.e-3*layer).astype(dtype)}
        thl = up(thl_h)
        ncell = g.imax*g.jmax*(g.kmax - 1)
        nbytes = 4*np.dtype(dtype).itemsize*ncell
        head = dict(shape=list(shape), dtype=np.dtype(dtype).name)
        for fname, q in fields.items():
            qt = up(q)
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            # the w-level values, their saturation, and the 64-cell row segments (one wave each) that hold a saturated cell
            ks, ke = g.kstart, g.kend
            inner = (slice(None), slice(g.jstart, g.jend), slice(g.istart, g.iend))
            thlh = (0.5*(thl[ks:ke-1] + thl[ks+1:ke]))[inner].contiguous()
            qth = (0.5*(qt[ks:ke-1] + qt[ks+1:ke]))[inner].contiguous()
            ph = tab[0][ks+1:ke, None, None].expand_as(thlh).contiguous(); exh = tab[1][ks+1:ke, None, None].expand_as(thlh).contiguous()
            ql, qi = torch.zeros_like(thlh), torch.zeros_like(thlh)
            capi.check(lib.mhh_thermo_moist_sat_adjust(g.dtype, thlh.numel(), P(thlh), P(qth), P(ph), P(exh), P(ql), P(qi), None, None, P(count), stream()))
            sat = (ql + qi) > 0
            nseg = (g.imax + 63)//64
            pad = torch.zeros(sat.shape[:2] + (nseg*64,), dtype=torch.bool, device=dev); pad[..., :g.imax] = sat
            waves = pad.reshape(sat.shape[0], sat.shape[1], nseg, 64).any(dim=-1)
            sat_share, wave_share = float(sat.float().mean()), float(waves.float().mean())
            del thlh, qth, ph, exh, ql, qi, sat, pad, waves
            wt = {MARCH: torch.zeros(g.shape3, dtype=thl.dtype, device=dev), CELL: torch.zeros(g.shape3, dtype=thl.dtype, device=dev)}

            def call(impl):
                capi.check(lib.mhh_thermo_moist_buoyancy_tend_impl(G, impl, P(wt[impl]), P(thl), P(qt), P(tab[0]), P(tab[1]), P(tab[2]), P(count), stream()))
            call(MARCH); call(CELL); torch.cuda.synchronize()
            same = bool(torch.equal(wt[MARCH], wt[CELL]))
            once, _, _ = median_ms(torch, lambda: call(MARCH), n=3)
            reps = max(1, int(50. / max(once, 1e-3)))
            res = {}
            for rnd in range(2):                      # alternate the two forms, twice: the spread between the rounds is the noise
                for impl, name in ((MARCH, "march"), (CELL, "cell")):
                    res.setdefault(name, []).append(median_ms(torch, lambda: call(impl), reps=reps))
            row = dict(head, name="tend", field=fname, saturated_share=round(sat_share, 4), iterating_wave_share=round(wave_share, 4),
                       same_bits=same, nonconverged=int(count.cpu()[0]), reps=reps)
            for name in ("march", "cell"):
                ms = min(r[0] for r in res[name])
                row[name + "_ms"] = round(ms, 4); row[name + "_ms_rounds"] = [round(r[0], 4) for r in res[name]]
                row[name + "_TBps_on_4_passes"] = round(nbytes / (ms*1e-3) / 1e12, 3)
            emit(row)
            del qt, wt
            torch.cuda.empty_cache()
        del thl
        torch.cuda.empty_cache()

    for ktot in args.ktot:
        g = Grid(64, 64, ktot, 6400., 6400., 3000., order=2, igc=3, jgc=3, kgc=1, dtype=np.float64)
        G = g.device_struct(dev)
        thl0, qt0 = thermo.bomex_profiles(g.z[g.kstart:g.kend])
        bs = thermo.base_state(lib, g, thl0, qt0, PBOT)
        mean = [up(bs["thl0"]), up(bs["qt0"])]
        out = [torch.zeros(g.kcells, dtype=torch.float64, device=dev) for _ in thermo.BASE_STATE]
        count = torch.zeros(1, dtype=torch.int32, device=dev)

        def device_form():
            capi.check(lib.mhh_thermo_moist_base_state(G, P(mean[0]), P(mean[1]), PBOT, *[P(o) for o in out], P(count), stream()))
        hbuf = [np.zeros(g.kcells) for _ in thermo.BASE_STATE]
        pinned = [torch.from_numpy(h) for h in hbuf]
        Gh = g.host_struct()
        n = C.c_int(0)

        def round_trip():
            a, b = mean[0].cpu().numpy(), mean[1].cpu().numpy()
            capi.check(lib.mhh_thermo_moist_base_state_host(Gh, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), PBOT, 0, 0.,
                                                            *[C.c_void_p(h.ctypes.data) for h in hbuf], C.byref(n)))
            for o, h in zip(out, pinned):
                o.copy_(h, non_blocking=True)
            torch.cuda.synchronize()
        dev_ms = median_ms(torch, device_form, reps=20)
        for _ in range(3):
            round_trip()
        ts = []
        for _ in range(15):
            t0 = time.perf_counter()
            for _ in range(20):
                round_trip()
            ts.append((time.perf_counter() - t0)/20*1e3)
        emit(dict(name="base_state", ktot=ktot, dtype="float64", device_kernel_ms=round(dev_ms[0], 4), device_kernel_ms_min_max=[round(dev_ms[1], 4), round(dev_ms[2], 4)],
                  host_round_trip_ms=round(float(np.median(ts)), 4), host_round_trip_ms_min_max=[round(min(ts), 4), round(max(ts), 4)]))
    if args.step:
        from microhh_amd.forcing import Forcing
        from microhh_amd.model import HotPath
        from microhh_amd.surface import Surface
        n, ms = args.step, {}

        def extras():        # BOMEX's surface (fixed ustar, two fluxes) and large-scale terms in kind (subsidence on the means, drying of qt)
            z = Grid(n, n, n, 6400., 6400., 3000., order=2, igc=3, jgc=3, kgc=1).z.astype(np.float64)
            wls = -0.0065*np.minimum(z/1500., 1.)*np.clip((2100. - z)/600., 0., 1.)
            return dict(surface=Surface(mbcbot="ustar", ustar=0.28, sbcbot="flux", sbot=[8e-3, 5.2e-5]),
                        forcing=Forcing(swwls="mean", wls=wls, lsprofs={"s1": -1.2e-8*np.clip((500. - z)/200. + 1., 0., 1.)}))
        for full in (False, True):
            for moist in (False, True):
                hp = HotPath("bomex", n, n, n, thermo=thermo.Moist(PBOT) if moist else None, **(extras() if full else {}))
                ms[full, moist] = median_ms(torch, hp.step)[0]
                if moist and not full:
                    th = hp.thermo
                    ms["means"] = median_ms(torch, th.means, reps=20)[0]
                    ms["base"] = median_ms(torch, th.update_base_state, reps=20)[0]
                    ms["tend"] = median_ms(torch, th.tend, reps=20)[0]
                if moist:
                    hp.thermo.check()
                hp.close(); del hp
                torch.cuda.empty_cache()
        emit(dict(name="step", shape=[n, n, n], dtype="float64", step_ms=round(ms[False, False], 4), step_with_thermo_ms=round(ms[False, True], 4),
                  means_ms=round(ms["means"], 4), base_state_ms=round(ms["base"], 4), tendency_ms=round(ms["tend"], 4),
                  share_of_step=round((ms[False, True] - ms[False, False]) / ms[False, False], 4),
                  step_surface_forcing_ms=round(ms[True, False], 4), step_surface_forcing_thermo_ms=round(ms[True, True], 4),
                  share_of_full_step=round((ms[True, True] - ms[True, False]) / ms[True, False], 4)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
