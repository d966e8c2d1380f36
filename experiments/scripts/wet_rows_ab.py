"""k_ringcz's strips cut from the wet rows of each window (option "wet_rows") against the even cut.   python experiments/scripts/wet_rows_ab.py [reps]
BASELINE config 3 (2400 x 3600 IRREGULAR_WITH_LAND, Taper, n_steps 63) on two masks: the fixture's (row 0 and the south-west quadrant are land:
the table is taken) and row 0 alone (the table marches what the even cut marches: the policy of option 1 must leave the launch as it is).
Two plans per mask (folded anew, so their planes land elsewhere), the options alternating (0, 1, 0, 1, ...); per round the time of an application (host clock around `reps` applications and a
synchronise) and, from the plan's own event pairs, the launches of the dominant kernel.  Also: same values?"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100


def set_wet_rows(plan, opt):
    """(a build from before the option has one behaviour: the script then measures that build against itself)"""
    try:
        plan.set_option("wet_rows", opt)
    except _lib.GcmfError:
        pass


rounds = 4
wl = T.baseline_workload(3)
grid, fk = wl["grid"], wl["fk"]
shape = wl["fields"][0].shape[-2:]
row0 = np.ones(shape)
row0[0, :] = 0
for name, mask in (("fixture mask", wl["grid_vars"]["wet_mask"]), ("row 0 land only", row0)):
    gv = dict(wl["grid_vars"], wet_mask=mask)
    keep = []
    for placement in range(2):   # (a plan runs its launches in one of two modes a few per cent apart, by where its planes land in HBM: two plans per mask)
        clear_plan_cache()
        keep.append(torch.empty(48 << 20, dtype=torch.uint8, device="cuda"))
        flt = Filter(grid_type=GridType[grid], grid_vars=gv, filter_scale=fk["filter_scale"], dx_min=fk["dx_min"], filter_shape=FilterShape[fk["filter_shape"]])
        plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, shape)
        d = torch.from_numpy(wl["fields"][0]).cuda()
        outs, ran, times, launch = {}, {}, {0: [], 1: []}, {}
        for opt in (0, 1):
            set_wet_rows(plan, opt)
            plan.last_kernel()
            outs[opt] = flt.apply(d).cpu().numpy()
            ran[opt] = (plan.last_kernel(), plan.last_kernel_geometry())
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.2:
            flt.apply(d); torch.cuda.synchronize()
        for r in range(rounds):
            for opt in (0, 1):
                set_wet_rows(plan, opt)
                for _ in range(10):
                    flt.apply(d)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    flt.apply(d)
                torch.cuda.synchronize()
                times[opt].append((time.perf_counter() - t0) / reps * 1e6)
        for opt in (0, 1):
            set_wet_rows(plan, opt)
            plan.set_timing(2)
            ms = n = 0
            for _ in range(5):
                flt.apply(d)
                a, b, lo, hi = plan.last_kernel_timing()
                ms, n = ms + a, n + b
            plan.set_timing(False)
            launch[opt] = 1e3 * ms / max(n, 1)
        set_wet_rows(plan, 1)
        print(f"{name}, plan {placement}: n_steps {flt.n_steps}, same values {np.array_equal(outs[0], outs[1], equal_nan=True)}")
        for opt in (0, 1):
            t = times[opt]
            print(f"   wet_rows {opt}: {ran[opt][0]} {ran[opt][1]}\n      us per application {[round(x, 1) for x in t]} median {np.median(t):.1f} spread {100 * (max(t) - min(t)) / np.median(t):.2f} %;"
                  f" dominant launch {launch[opt]:.1f} us (event pairs)", flush=True)
        print(f"   option 1 / option 0: {np.median(times[1]) / np.median(times[0]):.4f}", flush=True)
