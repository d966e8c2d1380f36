"""The tight cut of k_ringcz's wet-row table (option "wet_rows" 3, round 8) against the table of round 7 (option 1).
    python experiments/scripts/wet_tight_ab.py [reps] [NYxNX | NYxNX:row0 ...]      (default: 2400x3600 2400x3600:row0)
BASELINE config 3's grid and filter (IRREGULAR_WITH_LAND, Taper, n_steps 63) on the fixture mask, or (":row0") with only row 0 land, where the
policy of either option must refuse the table.  Two plans per case (folded anew, so their planes land elsewhere), the options alternating
(1, 3, 1, 3, ...) on one plan; per round the time of an application (host clock around `reps` applications and a synchronise) and, from the
plan's own event pairs, the launches of the dominant kernel.  Also: same values as option 0?  A build from before round 8 takes 3 as "whenever
eligible" of round 7's cut: the script then measures round 7 against itself."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 100
cases = args or ["2400x3600", "2400x3600:row0"]
OPTS = (1, 3)
rounds = 4
for case in cases:
    dims, _, variant = case.partition(":")
    shape = tuple(int(v) for v in dims.split("x"))
    wl = T.baseline_workload(3, shape=shape)
    grid, fk = wl["grid"], wl["fk"]
    mask = wl["grid_vars"]["wet_mask"]
    if variant == "row0":
        mask = np.ones(shape)
        mask[0, :] = 0
    gv = dict(wl["grid_vars"], wet_mask=mask)
    for placement in range(2):   # (a plan runs its launches in one of two modes a few per cent apart, by where its planes land in HBM)
        clear_plan_cache()
        keep = torch.empty((48 << 20) * (placement + 1), dtype=torch.uint8, device="cuda")
        flt = Filter(grid_type=GridType[grid], grid_vars=gv, filter_scale=fk["filter_scale"], dx_min=fk["dx_min"], filter_shape=FilterShape[fk["filter_shape"]])
        plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, shape)
        d = torch.from_numpy(wl["fields"][0]).cuda()
        outs, ran, times, launch = {}, {}, {o: [] for o in OPTS}, {}
        for opt in (0,) + OPTS:
            plan.set_option("wet_rows", opt)
            plan.last_kernel()
            outs[opt] = flt.apply(d).cpu().numpy()
            ran[opt] = (plan.last_kernel(), plan.last_kernel_geometry())
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            flt.apply(d); torch.cuda.synchronize()
        for r in range(rounds):
            for opt in OPTS:
                plan.set_option("wet_rows", opt)
                for _ in range(10):
                    flt.apply(d)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    flt.apply(d)
                torch.cuda.synchronize()
                times[opt].append((time.perf_counter() - t0) / reps * 1e6)
        for opt in OPTS:
            plan.set_option("wet_rows", opt)
            plan.set_timing(2)
            ms = n = 0
            for _ in range(5):
                flt.apply(d)
                a, b, lo, hi = plan.last_kernel_timing()
                ms, n = ms + a, n + b
            plan.set_timing(False)
            launch[opt] = 1e3 * ms / max(n, 1)
        same = all(np.array_equal(outs[0], outs[o], equal_nan=True) for o in OPTS)
        print(f"{case}, plan {placement}: n_steps {flt.n_steps}, same values as option 0: {same}")
        for opt in OPTS:
            t = times[opt]
            print(f"   wet_rows {opt}: {ran[opt][0]} {ran[opt][1]}\n      us per application {[round(x, 1) for x in t]} median {np.median(t):.1f} spread {100 * (max(t) - min(t)) / np.median(t):.2f} %;"
                  f" dominant launch {launch[opt]:.1f} us (event pairs)", flush=True)
        print(f"   option {OPTS[1]} / option {OPTS[0]}: {np.median(times[OPTS[1]]) / np.median(times[OPTS[0]]):.4f}", flush=True)
        del keep, d
