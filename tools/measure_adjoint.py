"""What the adjoint costs against the forward filter: Filter.adjoint (gcmf_apply_adjoint: a pre-scale pass, gcmf_apply's own schedule,
a post-scale pass in place) against Filter.apply on the same workload.  Device-resident 2400 x 3600 f64 IRREGULAR_WITH_LAND fields,
n_steps 63: one lone field, and a batch of 16.  Forward and adjoint alternate in one process; device events around blocks of
applications, warm-up first, median of five blocks; spread = (max - min) / median of the five.  The two passes move 24 bytes per cell
each on this grid type (the plane in, 1 / area, the plane out; + a land byte): the last lines say what fraction of 8 TB/s the difference
of the two medians makes of them.
    python tools/measure_adjoint.py [n_fields] [applications per block] [ny nx]"""
import os
import statistics
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCMF_RESIDENT", "0")
import torch  # noqa: E402

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T  # noqa: E402
from gcm_filters_amd.kernels import ALL_KERNELS  # noqa: E402

KIND = "IRREGULAR_WITH_LAND"
NB = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SHAPE = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else T.BASELINE_SHAPE
N_STEPS = 63
PEAK = 8.0e12   # bytes per second


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(routes, reps, nblocks=5):
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


def line(name, res, per, extra=""):
    med, spread, ms = res
    print(f"{name:34s} {med:9.3f} ms per call = {med / per:7.3f} ms per field   spread {100 * spread:4.1f} %   "
          f"blocks {' '.join(f'{x:.3f}' for x in ms)}   {extra}", flush=True)


gv = T.scalar_grid_vars(KIND, SHAPE)
gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
dx = T.grid_dx_min(KIND, gv)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    flt = Filter(filter_scale=8.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=N_STEPS, grid_type=GridType[KIND], grid_vars=gv)
plan = ALL_KERNELS[GridType[KIND]](**gv)._plan(_lib.F64, SHAPE)
print(f"{KIND} {SHAPE} f64, n_steps {N_STEPS}, build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)
ncell = SHAPE[0] * SHAPE[1]
for nb, reps in ((1, 4 * REPS), (NB, REPS)):
    f = torch.from_numpy(np.stack([T.random_field(SHAPE, 100 + b) for b in range(nb)])).cuda()
    f[:, torch.from_numpy(gv["wet_mask"] == 0).cuda()] = float("nan")
    g = torch.from_numpy(np.stack([T.random_field(SHAPE, 200 + b) for b in range(nb)])).cuda()
    res = alternate({"forward": lambda: flt.apply(f), "adjoint": lambda: flt.adjoint(g), "adjoint, like": lambda: flt.adjoint(g, like=f)}, reps)
    names = {}
    for k, fn in (("forward", lambda: flt.apply(f)), ("adjoint", lambda: flt.adjoint(g))):
        plan.last_kernel()
        fn()
        names[k] = plan.last_kernel()
    print(f"-- {nb} field{'s' if nb > 1 else ''}", flush=True)
    line("forward  Filter.apply", res["forward"], nb, names["forward"])
    line("adjoint  Filter.adjoint", res["adjoint"], nb, names["adjoint"])
    line("adjoint  Filter.adjoint(like=)", res["adjoint, like"], nb)
    for k in ("adjoint", "adjoint, like"):
        extra_ms = res[k][0] - res["forward"][0]
        moved = nb * ncell * (2 * 24 + 2 + (16 if k.endswith("like") else 0))     # two passes; `like` is read by both
        frac = f"{100 * moved / (extra_ms * 1e-3) / PEAK:4.1f} % of 8 TB/s for the {moved / 1e9:.2f} GB of the two passes" if extra_ms > 0 else "inside the spread"
        print(f"   {k:14s} / forward = {res[k][0] / res['forward'][0]:5.3f}   (+{extra_ms:6.3f} ms per call: {frac})", flush=True)
