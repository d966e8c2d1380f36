"""What filter-and-coarsen in one call saves: Filter.apply_coarsened (gcmf_apply_coarsen: gcmf_apply's schedule, then one streaming pass
that writes weighted block means) against Filter.apply followed by the same block mean outside the library.  2400 x 3600 f64
IRREGULAR_WITH_LAND, n_steps 63, one field, factors (4, 4) and (10, 10):
  (a) a device tensor in and out: apply_coarsened against apply + the block mean in torch (the rule: skip land and NaN, weight by area);
  (b) numpy in and out: apply_coarsened against apply + the block mean in numpy (gcm_filters_amd.coarsen.block_means);
  (c) the pass alone, in GB/s, beside the two scaling passes of gcmf_apply_adjoint on the same plane: both as the difference to
      gcmf_apply of the same short polynomial (3 steps, so that the schedule is small beside the passes), device pointers.
The routes alternate in one process; warm-up first, then five blocks per route, median and spread = (max - min) / median.  Device routes
are timed with device events around a block of calls, host routes with the wall clock around each call.
    python tools/measure_coarsen.py [calls per device block] [ny nx]"""
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCMF_RESIDENT", "0")
import torch  # noqa: E402

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, coarsen, testing as T  # noqa: E402
from gcm_filters_amd.kernels import ALL_KERNELS  # noqa: E402

KIND = "IRREGULAR_WITH_LAND"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
SHAPE = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else T.BASELINE_SHAPE
N_STEPS = 63
FACTORS = ((4, 4), (10, 10))


def device_block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def host_block(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(routes, block, reps, nblocks=5):
    """{name: (median ms per call, spread, the blocks)}: the routes take turns, block by block."""
    for fn in routes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(nblocks):
        for k, fn in routes.items():
            ms[k].append(block(fn, reps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), v) for k, v in ms.items()}


def line(name, res, extra=""):
    med, spread, ms = res
    print(f"{name:44s} {med:9.3f} ms   spread {100 * spread:5.1f} %   blocks {' '.join(f'{x:.3f}' for x in ms)}   {extra}", flush=True)


def torch_block_means(F, w, fy, fx):
    """The rule in torch, as a device user writes it: skip land (w <= 0) and NaN, weight by w, NaN where nothing counts."""
    ny, nx = F.shape[-2:]
    counts = (w > 0) & ~torch.isnan(F)
    wc = torch.where(counts, w, torch.zeros_like(w))
    prod = torch.where(counts, w * torch.where(counts, F, torch.zeros_like(F)), torch.zeros_like(F))
    blocks = lambda a: a.reshape(a.shape[:-2] + (ny // fy, fy, nx // fx, fx)).sum(dim=(-3, -1))
    ws = blocks(wc.expand_as(F))
    return torch.where(ws > 0, blocks(prod) / ws, torch.full_like(ws, float("nan")))


gv = T.scalar_grid_vars(KIND, SHAPE)
gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
dx = T.grid_dx_min(KIND, gv)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    flt = Filter(filter_scale=8.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=N_STEPS, grid_type=GridType[KIND], grid_vars=gv)
print(f"{KIND} {SHAPE} f64, n_steps {N_STEPS}, one field, build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)
ncell = SHAPE[0] * SHAPE[1]
w_host = coarsen.default_weights(GridType[KIND], gv)
w_dev = torch.from_numpy(w_host).cuda()
f_host = T.random_field(SHAPE, 100)[None]
f_dev = torch.from_numpy(f_host).cuda()

for fy, fx in FACTORS:
    print(f"-- factor ({fy}, {fx})", flush=True)
    got = flt.apply_coarsened(f_dev, (fy, fx))
    ref = torch_block_means(flt.apply(f_dev), w_dev, fy, fx)
    ok = ~torch.isnan(ref)
    assert bool((torch.isnan(got) == torch.isnan(ref)).all())
    print(f"   largest |one call - apply + torch| / largest |value|: {float((got - ref)[ok].abs().max() / ref[ok].abs().max()):.2e}", flush=True)
    res = alternate({"one": lambda: flt.apply_coarsened(f_dev, (fy, fx)), "two": lambda: torch_block_means(flt.apply(f_dev), w_dev, fy, fx),
                     "fine": lambda: flt.apply(f_dev)}, device_block, REPS)
    line("(a) device  apply_coarsened", res["one"])
    line("(a) device  apply + torch block mean", res["two"], f"{res['two'][0] / res['one'][0]:.2f} x the one call")
    line("(a) device  apply alone", res["fine"])
    res = alternate({"one": lambda: flt.apply_coarsened(f_host, (fy, fx)), "two": lambda: coarsen.block_means(flt.apply(f_host), w_host, (fy, fx)),
                     "fine": lambda: flt.apply(f_host)}, host_block, 2)
    line("(b) numpy   apply_coarsened", res["one"])
    line("(b) numpy   apply + numpy block mean", res["two"], f"{res['two'][0] / res['one'][0]:.2f} x the one call")
    line("(b) numpy   apply alone", res["fine"])

# (c) the pass beside the adjoint's scaling passes: differences to gcmf_apply of a 3-step polynomial, through the plan
plan = ALL_KERNELS[GridType[KIND]](**gv)._plan(_lib.F64, SHAPE)
p, c = np.array([0.5, 0.3, 0.15, 0.05]), 2 / flt.filter_spec.s_max
stream = torch.cuda.current_stream().cuda_stream
x, fine, adj = f_dev[0].contiguous(), torch.empty(SHAPE, dtype=torch.float64, device="cuda"), torch.empty(SHAPE, dtype=torch.float64, device="cuda")
with coarsen._plan_lock(plan):      # (the Filter's weights are on the plan: the grid's own)
    for fy, fx in FACTORS:
        co = torch.empty((SHAPE[0] // fy, SHAPE[1] // fx), dtype=torch.float64, device="cuda")
        res = alternate({"apply": lambda: plan.apply(p, c, [x.data_ptr()], [fine.data_ptr()], 1, device_ptrs=True, stream=stream),
                         "coarsen": lambda: plan.apply_coarsen(p, c, [x.data_ptr()], [co.data_ptr()], 1, fy, fx, device_ptrs=True, stream=stream),
                         "adjoint": lambda: plan.apply_adjoint(p, c, [x.data_ptr()], [adj.data_ptr()], 1, device_ptrs=True, stream=stream)},
                        device_block, 4 * REPS)
        print(f"-- (c) factor ({fy}, {fx}), 3 steps", flush=True)
        for k in ("apply", "coarsen", "adjoint"):
            line("(c) gcmf_" + {"apply": "apply", "coarsen": "apply_coarsen", "adjoint": "apply_adjoint"}[k], res[k])
        d_co, d_adj = res["coarsen"][0] - res["apply"][0], res["adjoint"][0] - res["apply"][0]
        b_co, b_adj = ncell * (16 + 8 / (fy * fx)), ncell * 2 * 25      # fine + weights in, coarse out; twice (plane + 1 / area + land byte in, plane out)
        rate = lambda b, ms: f"{b / (ms * 1e-3) / 1e9:7.0f} GB/s" if ms > 0 else "inside the spread"
        print(f"   the coarsening pass:      +{d_co:6.3f} ms for {b_co / 1e6:6.1f} MB = {rate(b_co, d_co)}", flush=True)
        print(f"   the two scaling passes:   +{d_adj:6.3f} ms for {b_adj / 1e6:6.1f} MB = {rate(b_adj, d_adj)}", flush=True)
