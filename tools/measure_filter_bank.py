"""One field filtered at M scales -- a sweep, as filtering spectra and scale-dependent energies need it -- on IRREGULAR_WITH_LAND: what
FilterBank's one-batch route (gcmf_apply_bank: the M scales as M batch entries of the plain strips, a polynomial per entry) costs against the
loop over the scales that a user writes without it.  Device-resident float64 field, Taper, M = 4, 8 and 16 scales spread geometrically
between 4 and 16 dx_min; the degree is the bank's own (the largest default: 63 steps).  Grids 2400 x 3600 and 1080 x 1440.
TRIPOLAR_POP_WITH_LAND (--pop) in the same way: there the bank runs the plain strips below the tripole seam and k_fold_band's per-entry form on
its rows in launches of at most eight levels, the loop a lone field each on the zipped fold strips in launches of up to nine (or the on-chip
kernel on a small grid) -- so the rows are measured at 56 steps (seven launches either way) and at 63 (eight against seven), on 2400 x 3600,
1080 x 1440 and 384 x 320, the 1-degree POP grid.
  (a) FilterBank.apply with GCMF_FILTER_BANK=1 (last_route "bank");
  (b) [f.apply(field) for f in bank.filters], plans cached: a lone field each, on whatever the library runs a lone field on (zipped strips,
      wet-row tables).
Gappy fields (--gaps), IRREGULAR_WITH_LAND: N = 1 and 4 device-resident fields with distinct gaps (~16 % of the cells, as
tools/measure_gap_fold.py draws them) at M scales, 63 steps:
  (a) FilterBank(nan_mask="auto").apply with GCMF_FILTER_BANK=1 (gcmf_apply_bank_gaps: N folds, one batch of M N entries);
  (b) [f.apply(fields) for f in bank.filters], each Filter(nan_mask="auto"), plans cached: M flagged calls of N entries, M N folds.
The routes ALTERNATE inside each of five blocks; a block times `reps` applications (on small grids as many more as fill a quarter of a
second) between two device synchronisations (wall clock: the
loop's cost is partly the host's); median of the five blocks, spread = (max - min) / median.  The tool compares the outputs of (a) and (b)
bit for bit and says so.
    python tools/measure_filter_bank.py [--pop | --gaps] [applications per block] [M ...]"""
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gcm_filters_amd import FilterBank, FilterShape, GridType, _lib, testing as T  # noqa: E402
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache  # noqa: E402

POP = "--pop" in sys.argv[1:]
GAPS = "--gaps" in sys.argv[1:]
ARGV = [a for a in sys.argv[1:] if a not in ("--pop", "--gaps")]
KIND = "TRIPOLAR_POP_WITH_LAND" if POP else "IRREGULAR_WITH_LAND"
REPS = int(ARGV[0]) if ARGV else 3
MS = [int(a) for a in ARGV[1:]] or [4, 8, 16]


def alternate(routes, reps=REPS, nblocks=5):
    """{name: (median ms per application, spread, the blocks)}; the routes take turns inside every block."""
    for fn in routes.values():
        fn()
        fn()
    # small grids: as many applications per block as fill a quarter of a second (a shorter window times the clock and the scheduler)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    reps = max(reps, min(2000, int(0.25 * len(routes) / max(1e-6, time.perf_counter() - t0)) + 1))
    ms = {k: [] for k in routes}
    for _ in range(nblocks):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), v) for k, v in ms.items()}


def gappy(shape, nb):
    """nb fields with distinct gaps, ~16 % of the cells (tools/measure_gap_fold.py)."""
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


def report(shape, M, n_steps=0, nfield=0):
    """n_steps = 0: the bank's own degree; nfield > 0: that many gappy fields, each filtered under its own gaps"""
    gv = T.scalar_grid_vars(KIND, shape)
    gv["wet_mask"] = T.island_mask(shape, 7)     # (row 0 is land: what the tripolar kinds ask for)
    dx = T.grid_dx_min(KIND, gv)
    scales = [float(s) * dx for s in np.geomspace(4.0, 16.0, M)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # ("n_steps below the default": 56 steps are chosen for their launch cut)
        bank = FilterBank(filter_scales=scales, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=n_steps, grid_type=GridType[KIND], grid_vars=gv,
                          nan_mask="auto" if nfield else False)
    if nfield:
        host = gappy(shape, nfield)
        field = torch.from_numpy(host).cuda()
        print(f"--- gaps {np.isnan(host).mean():.3f} of the cells, {nfield} field(s), nan_mask=\"auto\"")
        del host
    else:
        field = torch.from_numpy(np.random.Generator(np.random.PCG64(11)).random(shape)).cuda()
    print(f"--- {KIND} {shape} f64, {M} scales {scales[0] / dx:.1f} .. {scales[-1] / dx:.1f} dx, n_steps {bank.n_steps}, wet fraction "
          f"{gv['wet_mask'].mean():.3f}, build {_lib.load().gcmf_build_id().decode()[:12]}", flush=True)

    def banked():
        os.environ["GCMF_FILTER_BANK"] = "1"
        try:
            return bank.apply(field)
        finally:
            del os.environ["GCMF_FILTER_BANK"]

    def looped():
        return [f.apply(field) for f in bank.filters]

    plan = ALL_KERNELS[GridType[KIND]](**gv)._plan(_lib.F64, tuple(shape), field.device.index)
    a = banked()
    assert bank.last_route == "bank", bank.last_route
    ran_a = f"cut {plan.bank_cut(bank.n_steps, M * max(1, nfield))}, ran {plan.last_kernel()} {plan.last_kernel_geometry()}"
    b = torch.stack(looped())
    ran_b = f"cut {plan.clenshaw_cut(bank.n_steps, 1)}, path {plan.last_path()}, ran {plan.last_kernel()} {plan.last_kernel_geometry()}"
    torch.cuda.synchronize()
    same = bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)) and torch.equal(torch.isnan(a), torch.isnan(b)))
    print(f"(a) {ran_a}\n(b) {ran_b}\n(a) and (b) bit for bit equal: {same}", flush=True)
    del a, b
    routes = {"(a) FilterBank, one batch": banked, "(b) loop over the scales": looped}
    res = alternate(routes)
    cells = shape[0] * shape[1] * bank.n_steps * M * max(1, nfield)
    for k, (med, spread, blocks) in res.items():
        print(f"{k:28s} {med:9.3f} ms = {med / M:7.3f} ms per scale = {cells / med * 1e-6:6.1f} G cells.steps/s   spread {100 * spread:4.1f} %   "
              f"blocks {' '.join(f'{x:.3f}' for x in blocks)}", flush=True)
    (ma, sa, _), (mb, sb, _) = res["(a) FilterBank, one batch"], res["(b) loop over the scales"]
    margin = (mb - ma) / mb
    verdict = "bank at least as fast beyond the spreads" if margin > max(sa, sb) else \
              "loop faster beyond the spreads" if -margin > max(sa, sb) else "inside the spreads"
    print(f"(a) takes {100 * margin:+.1f} % less time than (b); the larger spread of the two is {100 * max(sa, sb):.1f} %: {verdict}", flush=True)
    clear_plan_cache()
    return same


ok = True
if GAPS:
    for shape in (T.BASELINE_SHAPE, (1080, 1440)):
        for nfield in (1, 4):
            for M in MS:
                ok = report(tuple(shape), M, 63, nfield) and ok
elif POP:
    for shape in (T.BASELINE_SHAPE, (1080, 1440), (384, 320)):
        for n_steps in (56, 63):
            for M in MS:
                ok = report(tuple(shape), M, n_steps) and ok
else:
    for shape in (T.BASELINE_SHAPE, (1080, 1440)):
        for M in MS:
            ok = report(tuple(shape), M) and ok
sys.exit(0 if ok else 1)
