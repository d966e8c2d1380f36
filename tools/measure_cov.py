"""What subfilter covariances in one call save: Filter.apply_covariance (gcmf_apply_cov: a pre pass, ONE gcmf_apply on the 3 N entries of
N pairs, a post pass) against the composition a user writes, apply(f * g) - apply(f) * apply(g).  2400 x 3600 f64 IRREGULAR_WITH_LAND,
n_steps 63, one pair and 16 pairs:
  (a) device tensors in and out: apply_covariance against three apply calls plus the torch arithmetic (16 pairs also with the
      scratch bound raised so that the call is one run, not two);
  (b) numpy in and out: the same, the arithmetic in numpy;
  (v) the variance form (other=None) against apply(f * f) - apply(f) ** 2, device tensors;
  (c) the two passes alone, in GB/s, beside the coarsening pass and the two scaling passes of gcmf_apply_adjoint on the same planes:
      each as the difference to gcmf_apply of the same short polynomial (3 steps, so that the schedule is small beside the passes) on
      the same number of entries, device pointers.
The routes alternate in one process; warm-up first, then five blocks per route, median and spread = (max - min) / median.  Device routes
are timed with device events around a block of calls, host routes with the wall clock around each call.  The baseline is the composed
route of the same run; a row where the one call does not win is printed like any other.
    python tools/measure_cov.py [calls per device block] [ny nx]"""
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCMF_RESIDENT", "0")
import torch  # noqa: E402

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T  # noqa: E402
from gcm_filters_amd.kernels import ALL_KERNELS  # noqa: E402

KIND = "IRREGULAR_WITH_LAND"
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
SHAPE = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else T.BASELINE_SHAPE
N_STEPS = 63
NPAIRS = (1, 16)


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
    print(f"{name:48s} {med:9.3f} ms   spread {100 * spread:5.1f} %   blocks {' '.join(f'{x:.3f}' for x in ms)}   {extra}", flush=True)


gv = T.scalar_grid_vars(KIND, SHAPE)
gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
dx = T.grid_dx_min(KIND, gv)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    flt = Filter(filter_scale=8.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=N_STEPS, grid_type=GridType[KIND], grid_vars=gv)
print(f"{KIND} {SHAPE} f64, n_steps {N_STEPS}, build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)
ncell = SHAPE[0] * SHAPE[1]
plan = ALL_KERNELS[GridType[KIND]](**gv)._plan(_lib.F64, SHAPE)      # the cached plan the Filter runs on

for n in NPAIRS:
    print(f"-- {n} pair(s)", flush=True)
    f_host = np.stack([T.random_field(SHAPE, 100 + b) for b in range(n)])
    g_host = np.stack([T.random_field(SHAPE, 500 + b) for b in range(n)])
    f_dev, g_dev = torch.from_numpy(f_host).cuda(), torch.from_numpy(g_host).cuda()
    composed = lambda f, g: flt.apply(f * g) - flt.apply(f) * flt.apply(g)
    got, ref = flt.apply_covariance(f_dev, g_dev), composed(f_dev, g_dev)
    print(f"   one call and composition: {'the same bits' if torch.equal(got, ref) else 'DIFFERENT BITS'}", flush=True)
    del got, ref
    reps = REPS if n == 1 else max(1, REPS // 4)
    res = alternate({"one": lambda: flt.apply_covariance(f_dev, g_dev), "three": lambda: composed(f_dev, g_dev), "apply": lambda: flt.apply(f_dev)},
                    device_block, reps)
    line("(a) device  apply_covariance", res["one"])
    line("(a) device  3 x apply + torch arithmetic", res["three"], f"{res['three'][0] / res['one'][0]:.2f} x the one call")
    line("(a) device  apply alone (n fields)", res["apply"])
    if 6 * n * ncell * 8 > 4096 << 20:      # the default bound cuts the call into runs: the same call as ONE run
        plan.set_option("cov_scratch_mb", 16384)
        try:
            res = alternate({"one": lambda: flt.apply_covariance(f_dev, g_dev)}, device_block, reps)
        finally:
            plan.set_option("cov_scratch_mb", 4096)
        line('(a) device  apply_covariance, "cov_scratch_mb" 16384', res["one"], "one run")
    res = alternate({"one": lambda: flt.apply_covariance(f_dev), "three": lambda: composed(f_dev, f_dev)}, device_block, reps)
    line("(v) device  apply_covariance, variance", res["one"])
    line("(v) device  apply(f f) - apply(f)^2", res["three"], f"{res['three'][0] / res['one'][0]:.2f} x the one call")
    res = alternate({"one": lambda: flt.apply_covariance(f_host, g_host), "three": lambda: composed(f_host, g_host)}, host_block, 1 if n > 1 else 2)
    line("(b) numpy   apply_covariance", res["one"])
    line("(b) numpy   3 x apply + numpy arithmetic", res["three"], f"{res['three'][0] / res['one'][0]:.2f} x the one call")
    del f_dev, g_dev

# (c) the passes alone: differences to gcmf_apply of a 3-step polynomial on as many entries, through the plan
p, c = np.array([0.5, 0.3, 0.15, 0.05]), 2 / flt.filter_spec.s_max
stream = torch.cuda.current_stream().cuda_stream
rate = lambda b, ms: f"{b / (ms * 1e-3) / 1e9:7.0f} GB/s" if ms > 0 else "inside the spread"
for n in (1, 4):
    x = torch.from_numpy(np.stack([T.random_field(SHAPE, 100 + b) for b in range(3 * n)])).cuda()
    y, out3 = x[n:2 * n], torch.empty_like(x)
    tau, co = torch.empty_like(x[:n]), torch.empty((3 * n, SHAPE[0] // 4, SHAPE[1] // 4), dtype=torch.float64, device="cuda")
    res = alternate({"apply3": lambda: plan.apply(p, c, [x.data_ptr()], [out3.data_ptr()], 3 * n, device_ptrs=True, stream=stream),
                     "apply2": lambda: plan.apply(p, c, [x.data_ptr()], [out3.data_ptr()], 2 * n, device_ptrs=True, stream=stream),
                     "cov": lambda: plan.apply_cov(p, c, x.data_ptr(), y.data_ptr(), tau.data_ptr(), n, device_ptrs=True, stream=stream),
                     "var": lambda: plan.apply_cov(p, c, x.data_ptr(), None, tau.data_ptr(), n, device_ptrs=True, stream=stream),
                     "coarsen": lambda: plan.apply_coarsen(p, c, [x.data_ptr()], [co.data_ptr()], 3 * n, 4, 4, device_ptrs=True, stream=stream),
                     "adjoint": lambda: plan.apply_adjoint(p, c, [x.data_ptr()], [out3.data_ptr()], 3 * n, device_ptrs=True, stream=stream)},
                    device_block, 4 * REPS if n == 1 else REPS)
    print(f"-- (c) {n} pair(s), 3 steps", flush=True)
    names = {"apply3": f"apply, {3 * n} entries", "apply2": f"apply, {2 * n} entries", "cov": f"apply_cov, {n} pair(s)", "var": f"apply_cov, variance, {n}",
             "coarsen": f"apply_coarsen (4, 4), {3 * n} entries", "adjoint": f"apply_adjoint, {3 * n} entries"}
    for k, name in names.items():
        line("(c) gcmf_" + name, res[k])
    d_cov, d_var = res["cov"][0] - res["apply3"][0], res["var"][0] - res["apply2"][0]
    d_co, d_adj = res["coarsen"][0] - res["apply3"][0], res["adjoint"][0] - res["apply3"][0]
    # pre: f, g in, f', g', fg out; post: three planes in, one out (variance: 1 in 2 out; 2 in 1 out)
    b_cov, b_var = n * ncell * 8 * 9, n * ncell * 8 * 6
    b_co, b_adj = 3 * n * ncell * (16 + 8 / 16), 3 * n * ncell * 2 * 25
    print(f"   the covariance's two passes:  +{d_cov:6.3f} ms for {b_cov / 1e6:7.1f} MB = {rate(b_cov, d_cov)}", flush=True)
    print(f"   the variance's two passes:    +{d_var:6.3f} ms for {b_var / 1e6:7.1f} MB = {rate(b_var, d_var)}", flush=True)
    print(f"   the coarsening pass:          +{d_co:6.3f} ms for {b_co / 1e6:7.1f} MB = {rate(b_co, d_co)}", flush=True)
    print(f"   the two scaling passes:       +{d_adj:6.3f} ms for {b_adj / 1e6:7.1f} MB = {rate(b_adj, d_adj)}", flush=True)
