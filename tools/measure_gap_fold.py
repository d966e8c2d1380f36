"""Gappy fields on a flux-form grid: what Filter(nan_mask="auto") (GCMF_FACES_FROM_NAN) costs against the routes through explicit masks.
16 device-resident 2400 x 3600 f64 fields with distinct gaps (~16 % of the cells), IRREGULAR_WITH_LAND, n_steps 63:
  (a) nan_mask="auto": every entry's face coefficients folded on the device inside the call, a stacked plan's launches;
  (b) the stacked plan of wet_mask(n, y, x) = wet_mask * notnull(field), plan CACHED: the floor -- the same launches without the fold;
  (c) the same with the plan built on EVERY call: what gaps that change from call to call cost before the flag, what (a) must beat;
  (d) the same batch, NaNs filled, one shared mask: the ceiling.
The routes alternate in one process; device events around blocks of applications, warm-up first, median of five blocks; spread =
(max - min) / median of the five.  Then one lone field, flagged against unflagged (the flagged call gives up the zipped strips and the
wet-row table), and the fold kernel alone: its time and the fraction of 8 TB/s that the bytes it moves make.
    python tools/measure_gap_fold.py [n_fields] [applications per block] [ny nx]"""
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
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache  # noqa: E402

KIND = "IRREGULAR_WITH_LAND"
NB = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
SHAPE = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else T.BASELINE_SHAPE
N_STEPS = 63
PEAK = 8.0e12   # bytes per second


def gappy(shape, nb):
    rng = np.random.Generator(np.random.PCG64(2025))
    out = np.empty((nb,) + shape)
    for b in range(nb):
        f = T.random_field(shape, 100 + b)
        f[rng.random(shape) < 0.15] = np.nan
        for _ in range(6):
            j0, i0 = int(rng.integers(1, shape[0] - 1)), int(rng.integers(0, shape[1] - 1))
            f[j0:j0 + int(rng.integers(shape[0] // 120 + 1, shape[0] // 12 + 2)), i0:i0 + int(rng.integers(shape[1] // 180 + 1, shape[1] // 12 + 2))] = np.nan
        out[b] = f
    return out


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(routes, reps=REPS, nblocks=5):
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


def line(name, res, per=NB, extra=""):
    med, spread, ms = res
    print(f"{name:44s} {med:9.3f} ms per call = {med / per:7.3f} ms per field   spread {100 * spread:4.1f} %   "
          f"blocks {' '.join(f'{x:.3f}' for x in ms)}   {extra}", flush=True)


gv = T.scalar_grid_vars(KIND, SHAPE)
gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
dx = T.grid_dx_min(KIND, gv)
host = gappy(SHAPE, NB)
dev = torch.from_numpy(host).cuda()
filled = torch.nan_to_num(dev, nan=0.5)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    kw = dict(filter_scale=8.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=N_STEPS, grid_type=GridType[KIND])
    auto = Filter(grid_vars=gv, nan_mask="auto", **kw)
    plain = Filter(grid_vars=gv, **kw)
print(f"{KIND} {SHAPE} f64, {NB} fields, n_steps {N_STEPS}, gaps {np.isnan(host).mean():.3f} of the cells, "
      f"build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)

lap = ALL_KERNELS[GridType[KIND]](**gv)
plan = lap._plan(_lib.F64, SHAPE)
spec = auto.filter_spec
m_dev = torch.from_numpy(gv["wet_mask"].copy()).cuda() * (~torch.isnan(dev)).to(torch.float64)
gv_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in gv.items()}


def explicit():
    """The stacked plan of the explicit masks (device-resident grid variables: nothing crosses the host link)."""
    e = ALL_KERNELS[GridType[KIND]](**{**gv_dev, "wet_mask": m_dev}, _stack_levels=True)
    return e._run([dev], spec=spec)[0]


def explicit_fresh():
    clear_plan_cache()
    return explicit()


assert torch.equal(torch.nan_to_num(auto.apply(dev)), torch.nan_to_num(explicit())), "the flagged call and the explicit masks disagree"

res = alternate({"a": lambda: auto.apply(dev), "b": explicit, "d": lambda: plain.apply(filled)})
plan.last_kernel()
auto.apply(dev)
line('(a) nan_mask="auto"', res["a"], extra=plan.last_kernel())
line("(b) explicit masks, stacked plan cached", res["b"])
line("(d) shared mask, no gaps: the ceiling", res["d"])
clear_plan_cache()
res_c = alternate({"c": explicit_fresh}, reps=1)
line("(c) explicit masks, plan built per call", res_c["c"])
clear_plan_cache()
torch.cuda.synchronize()
t0 = time.perf_counter()
explicit()
torch.cuda.synchronize()
print(f"{'    first call of (b), wall clock':44s} {(time.perf_counter() - t0) * 1e3:9.1f} ms", flush=True)

# one lone field: the flagged call gives up the zipped strips and the wet-row table
plan = lap._plan(_lib.F64, SHAPE)
one, one_filled = dev[:1].contiguous(), filled[:1].contiguous()
res1 = alternate({"flagged": lambda: auto.apply(one), "unflagged": lambda: plain.apply(one), "filled": lambda: plain.apply(one_filled)}, reps=4 * REPS)
plan.last_kernel()
auto.apply(one)
line("one field, flagged", res1["flagged"], per=1, extra=plan.last_kernel())
plain.apply(one)
line("one field, unflagged (gaps read as zeros)", res1["unflagged"], per=1, extra=plan.last_kernel())
line("one field, unflagged, no gaps", res1["filled"], per=1)

# the fold alone: (a) minus (b) is what the call pays for it; its own time through the plan's launch count is not separable from the
# outside, so the kernel is timed as the difference of the two alternated routes and bounded by its bytes
ncell = SHAPE[0] * SHAPE[1]
moved = NB * ncell * (8 + 24 + 25)      # per cell and entry: the field (8) and the plan's cE, cN, ra (24) read, cE, cN, ra and a land byte (25) written
fold_ms = res["a"][0] - res["b"][0]
if fold_ms > 0:
    print(f"fold = (a) - (b): {fold_ms:7.3f} ms for {NB} fields = {fold_ms / NB:6.3f} ms per field; it moves {moved / 1e9:5.2f} GB "
          f"(57 bytes per cell and entry): {100 * moved / (fold_ms * 1e-3) / PEAK:4.1f} % of 8 TB/s", flush=True)
else:
    print(f"fold = (a) - (b): {fold_ms:7.3f} ms (inside the spread)", flush=True)
