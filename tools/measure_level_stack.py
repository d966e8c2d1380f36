"""A 3-D field on a 3-D wet mask -- temp(z, y, x) with wet_mask(z, y, x), land growing with depth -- on IRREGULAR_WITH_LAND: what the
stacked plan (gcmf_plan_create_levels: one plan, one call, entry b on level b % nlev) costs against the per-level route (one plan and one
call per level, the results copied into place).  Device-resident float64 fields, BASELINE config 3's filter (Taper, 16 dx: n_steps 63):
  (a) the stacked route (GCMF_STACK_LEVELS=1; the default for more than 64 levels);
  (b) the per-level route, plans cached (GCMF_STACK_LEVELS=0; the default up to 64 levels);
  (c) the per-level route on its first call: the plan cache is emptied first, so every level's plan is built (one application per
      block; (a) and (b) are warmed up again afterwards, untimed).
Workload 1: 16 levels of 2400 x 3600.  Workload 2: 80 levels of 1080 x 1440, (a) and (b) -- 80 per-level plans cycle through the
64-entry plan cache, so every level of (b) misses on every call.
The routes ALTERNATE inside each of five blocks; a block times `reps` applications between two device synchronisations (wall clock: the
per-level route's cost is partly the host's); median of the five blocks, spread = (max - min) / median.  The tool compares the outputs of
(a) and (b) bit for bit and says so.
    python tools/measure_level_stack.py [applications per block] [levels of workload 1] [levels of workload 2]"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCMF_RESIDENT", "0")
import torch  # noqa: E402

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T  # noqa: E402
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache  # noqa: E402

KIND = "IRREGULAR_WITH_LAND"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
NLEV1 = int(sys.argv[2]) if len(sys.argv) > 2 else 16
NLEV2 = int(sys.argv[3]) if len(sys.argv) > 3 else 80


def eroding_mask(shape, nlev, per_level=1):
    """The island mask of the benchmarks on level 0; every level below loses the wet cells that touch land (4 neighbours), `per_level`
    times: the ocean narrows with depth."""
    m = T.island_mask(shape, 7).astype(bool)
    out = np.empty((nlev,) + tuple(shape))
    for l in range(nlev):
        out[l] = m
        for _ in range(per_level):
            m = m & np.roll(m, 1, 0) & np.roll(m, -1, 0) & np.roll(m, 1, 1) & np.roll(m, -1, 1)
    return out


def workload(shape, nlev):
    gv = T.scalar_grid_vars(KIND, shape)
    gv["wet_mask"] = eroding_mask(shape, nlev)
    dx = T.grid_dx_min(KIND, gv)
    kw = dict(filter_scale=16 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, grid_type=GridType[KIND], grid_vars=gv)
    rng = np.random.Generator(np.random.PCG64(11))
    field = torch.from_numpy(rng.random((nlev,) + tuple(shape))).cuda()
    return gv, kw, field


def with_stack(on, fn):
    def run():
        old = os.environ.get("GCMF_STACK_LEVELS")
        os.environ["GCMF_STACK_LEVELS"] = "1" if on else "0"
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["GCMF_STACK_LEVELS"]
            else:
                os.environ["GCMF_STACK_LEVELS"] = old
    return run


def alternate(routes, first_call=None, reps=REPS, nblocks=5):
    """{name: (median ms per application, spread, the blocks)}; the routes take turns inside every block.  first_call = (name, fn): timed
    once per block right after the plan cache was emptied; the routes are then warmed up again."""
    def warm():
        for fn in routes.values():
            fn()
            fn()
    warm()
    ms = {k: [] for k in routes}
    if first_call:
        ms[first_call[0]] = []
    for _ in range(nblocks):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
        if first_call:
            torch.cuda.synchronize()
            clear_plan_cache()
            t0 = time.perf_counter()
            first_call[1]()
            torch.cuda.synchronize()
            ms[first_call[0]].append((time.perf_counter() - t0) * 1e3)
            warm()
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), v) for k, v in ms.items()}


def report(shape, nlev, cold):
    gv, kw, field = workload(shape, nlev)
    print(f"--- {KIND} {shape} f64, {nlev} levels, wet fraction {gv['wet_mask'][0].mean():.3f} (top) .. {gv['wet_mask'][-1].mean():.3f} (bottom), "
          f"build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)
    stacked, per_level = Filter(**kw), Filter(**kw)
    routes = {"(a) stacked plan, one call": with_stack(True, lambda: stacked.apply(field)),
              "(b) per level, plans cached": with_stack(False, lambda: per_level.apply(field))}
    first = ("(c) per level, first call", routes["(b) per level, plans cached"]) if cold else None
    a = routes["(a) stacked plan, one call"]()
    # (asked before (b) runs: 80 per-level plans push the stacked one out of the plan cache)
    plan = ALL_KERNELS[GridType[KIND]](*[gv[k] for k in ALL_KERNELS[GridType[KIND]].required_grid_args()],
                                       _stack_levels=True)._stacked_plan(field.device.index)
    ran = f"cut {plan.clenshaw_cut(stacked.n_steps, nlev)}, ran {plan.last_kernel()} {plan.last_kernel_geometry()}"
    b = routes["(b) per level, plans cached"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)) and torch.equal(torch.isnan(a), torch.isnan(b)))
    print(f"n_steps {stacked.n_steps}, {ran}; (a) and (b) bit for bit equal: {same}", flush=True)
    del a, b
    res = alternate(routes, first)
    for k, (med, spread, blocks) in res.items():
        print(f"{k:30s} {med:9.3f} ms = {med / nlev:7.3f} ms per level   spread {100 * spread:4.1f} %   blocks {' '.join(f'{x:.3f}' for x in blocks)}",
              flush=True)
    (ma, sa, _), (mb, sb, _) = res["(a) stacked plan, one call"], res["(b) per level, plans cached"]
    margin = (mb - ma) / mb
    print(f"(a) takes {100 * margin:+.1f} % less time than (b); the larger spread of the two is {100 * max(sa, sb):.1f} %: "
          f"{'faster beyond the spread' if margin > max(sa, sb) else 'NOT faster beyond the spread'}", flush=True)
    clear_plan_cache()
    return same


ok = report(T.BASELINE_SHAPE, NLEV1, cold=True)
ok = report((1080, 1440), NLEV2, cold=False) and ok
sys.exit(0 if ok else 1)
