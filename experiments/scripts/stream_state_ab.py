"""Nine-level table launches with streamed state planes (option "stream_state" 2, round 10) against the default cache policy (option 0).
    python experiments/scripts/stream_state_ab.py [reps] [NYxNX ...]      (default: 2400x3600 1800x3600 1440x2880)
BASELINE config 3's grid and filter (IRREGULAR_WITH_LAND, Taper, n_steps 63) on the fixture mask.  Two plans per shape (folded anew, so their
planes land elsewhere), the options alternating (0, 2, 0, 2, ...) on one plan; per round the time of an application (host clock around
`reps` applications and a synchronise) and, from the plan's own event pairs, the launches of the dominant kernel.  Also: what the default
(option 1, stream_state_ok) takes at this shape, and whether the three give the same values."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 100
cases = args or ["2400x3600", "1800x3600", "1440x2880"]
OPTS = (0, 2)
rounds = 4
for case in cases:
    shape = tuple(int(v) for v in case.split("x"))
    wl = T.baseline_workload(3, shape=shape)
    grid, fk, gv = wl["grid"], wl["fk"], wl["grid_vars"]
    for placement in range(2):   # (a plan runs its launches in one of two modes a few per cent apart, by where its planes land in HBM)
        clear_plan_cache()
        keep = torch.empty((48 << 20) * (placement + 1), dtype=torch.uint8, device="cuda")
        flt = Filter(grid_type=GridType[grid], grid_vars=gv, filter_scale=fk["filter_scale"], dx_min=fk["dx_min"], filter_shape=FilterShape[fk["filter_shape"]])
        plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, shape)
        d = torch.from_numpy(wl["fields"][0]).cuda()
        outs, ran, times, launch = {}, {}, {o: [] for o in OPTS}, {}
        for opt in (1,) + OPTS:
            plan.set_option("stream_state", opt)
            plan.last_kernel()
            outs[opt] = flt.apply(d).cpu().numpy()
            ran[opt] = (plan.last_kernel(), plan.last_kernel_geometry())
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            flt.apply(d); torch.cuda.synchronize()
        for r in range(rounds):
            for opt in OPTS:
                plan.set_option("stream_state", opt)
                for _ in range(10):
                    flt.apply(d)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    flt.apply(d)
                torch.cuda.synchronize()
                times[opt].append((time.perf_counter() - t0) / reps * 1e6)
        for opt in OPTS:
            plan.set_option("stream_state", opt)
            plan.set_timing(2)
            ms = n = 0
            for _ in range(5):
                flt.apply(d)
                a, b, lo, hi = plan.last_kernel_timing()
                ms, n = ms + a, n + b
            plan.set_timing(False)
            launch[opt] = 1e3 * ms / max(n, 1)
        plan.set_option("stream_state", 1)
        same = all(np.array_equal(outs[1], outs[o], equal_nan=True) for o in OPTS)
        print(f"{case}, plan {placement}: n_steps {flt.n_steps}, same values under options 0, 1, 2: {same}; the default (option 1) ran {ran[1][1]}")
        for opt in OPTS:
            t = times[opt]
            print(f"   stream_state {opt}: {ran[opt][0]} {ran[opt][1]}\n      us per application {[round(x, 1) for x in t]} median {np.median(t):.1f} spread {100 * (max(t) - min(t)) / np.median(t):.2f} %;"
                  f" dominant launch {launch[opt]:.1f} us (event pairs)", flush=True)
        print(f"   option {OPTS[1]} / option {OPTS[0]}: {np.median(times[OPTS[1]]) / np.median(times[OPTS[0]]):.4f}", flush=True)
        del keep, d
