#!/usr/bin/env python3
"""bench.py -- throughput of the fused iterated-Laplacian filter on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config {2,3,4,5}] [--scaling strong|weak] [--full [--no-cpu] [--no-extra]]
                    [--dump-outputs DIR]

A "step" is ONE whole filter application (all n_steps Chebyshev/Laplacian steps) of the workload's field(s),
inputs already resident in HBM.  metric = grid-cells * Laplacian-steps / second (BASELINE.json).
Default workload = BASELINE config 3, the one the north-star target is quoted on:
IRREGULAR_WITH_LAND 2400x3600 fp64, Taper filter, filter_scale = 16 dx_min  =>  n_steps 63.

N > 1: one rank per GPU.  Under torch.distributed.run the ranks are already there; started as a plain
`python bench.py --gpus N` the script launches its own N ranks (a child `python -m torch.distributed.run`, started
before this process touches a GPU).  Scalar configs are cut into row slabs along y with halo rows exchanged over
xGMI (gcm_filters_amd/distributed.py); the default is STRONG scaling (the one BASELINE grid cut N ways), a weak
figure (N x ny rows) is measured in the same run and printed as `weak`.  Config 5 (50 levels) shards its levels
over the ranks: no communication at all.

Prints ONE JSON line on rank 0 (task contract).  N = 1: a plain run sets up, warms up, times the K steps, writes --dump-outputs and
prints the line (`value`, `ms_per_step`, the spread of the timed blocks) -- nothing else.  `--full` adds `roofline`, `parity`,
`cpu_baseline`, `extra_configs`, `host_path` and `summary`, and then the run FAILS (exit 1) if the timed workload's output differs from
the oracle / the reference-generated probes.  The N > 1 line and `--kinds` do not depend on `--full`.
"""
import argparse
import json
import math
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from bench_common import *  # noqa: E402,F401,F403  (tools/bench_common.py: byte counts, CPU baseline, parity helpers, run_single, roofline_of)
from bench_host import run_host_path  # noqa: E402


def run_config1(dev):
    """BASELINE config 1 (REGULAR 512x512 fp64, Gaussian filter_scale 4, n_steps 16): the reference's CPU-runnable case.  On the
    GPU it is a latency measurement (two launches); output checked against the probe the imported reference produced
    (tests/golden/reference_generated.npz: REGULAR/config1)."""
    import torch

    from gcm_filters_amd import Filter, GridType, testing as T

    f = T.random_field((512, 512), 100)
    flt = Filter(filter_scale=4.0, dx_min=1.0, n_steps=16, grid_type=GridType.REGULAR)
    d = torch.from_numpy(f).to(dev)
    for _ in range(5):
        out = flt.apply(d)
    torch.cuda.synchronize()
    reps, blocks = 200, []
    for _ in range(5):   # five blocks, the median one is reported (a 30-us measurement is easily hit by a one-off stall)
        t0 = time.perf_counter()
        for _ in range(reps):
            out = flt.apply(d)
        torch.cuda.synchronize()
        blocks.append(time.perf_counter() - t0)
    el = sorted(blocks)[2]
    rec = {"config": "BASELINE config 1: REGULAR 512x512, Gaussian filter_scale=4, n_steps=16 (HBM-resident, back-to-back calls)",
           "n_steps": 16, "steps": reps, "value": 512 * 512 * 16 * reps / el, "unit": "cell-steps/s",
           "us_per_application": 1e6 * el / reps, "us_per_application_min_max": [1e6 * min(blocks) / reps, 1e6 * max(blocks) / reps],
           "dtype": "f64"}
    gp = os.path.join(REPO, "tests", "golden", "reference_generated.npz")
    if os.path.exists(gp):
        with np.load(gp) as z:
            probe, sums = z["REGULAR/config1/probe"], z["REGULAR/config1/sums"]
        got = out.cpu().numpy()
        rec["parity"] = {"fixture": "tests/golden/reference_generated.npz:REGULAR/config1", "n_probes": int(probe.size),
                         "rel_err": float(np.abs(got[::8, ::8] - probe).max() / np.abs(probe).max()),
                         "sum_rel_err": float(abs(got.sum() - sums[0]) / abs(sums[0])), "tolerance": 1e-6,
                         "source": "imported reference (tests/golden/make_golden.py)"}
    return rec


def run_small_onchip(dev, no_cpu):
    """Not a BASELINE config: a small flux-form grid (IRREGULAR_WITH_LAND 512x512, the headline's filter: Taper, filter_scale 16 dx_min,
    n_steps 63) -- the north star's "whole n_steps polynomial fused into a single launch": gcmf_apply runs whole grids of up to 400 k
    cells on the chip (csrc/gcmf_resident.hip).  Reports the on-chip launch, the strip-marching launches of the same
    filter (GCMF_RESIDENT=0: eight launches, same bits) and, unless --no-cpu, the oracle parity of the result."""
    import torch

    from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
    from gcm_filters_amd.kernels import ALL_KERNELS

    shape = (512, 512)
    f, gv = T.scalar_case("IRREGULAR_WITH_LAND", shape)
    dx = T.grid_dx_min("IRREGULAR_WITH_LAND", gv)
    flt = Filter(filter_scale=16 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, grid_type=GridType.IRREGULAR_WITH_LAND, grid_vars=gv)
    plan = ALL_KERNELS[GridType.IRREGULAR_WITH_LAND](**gv)._plan(_lib.F64, shape, dev.index)
    d = torch.from_numpy(f).to(dev)

    def timed():
        for _ in range(5):
            out = flt.apply(d)
        torch.cuda.synchronize()
        plan.last_kernel()
        blocks = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(100):
                out = flt.apply(d)
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / 100)
        return sorted(blocks)[2], out, plan.last_kernel(), plan.last_kernel_geometry()
    before = os.environ.get("GCMF_RESIDENT")
    try:
        t_chip, out, k_chip, geom = timed()
        os.environ["GCMF_RESIDENT"] = "0"
        t_strip, out2, k_strip, _ = timed()
    finally:
        if before is None:
            os.environ.pop("GCMF_RESIDENT", None)
        else:
            os.environ["GCMF_RESIDENT"] = before
    n = int(flt.n_steps)
    rec = {"config": f"extra: IRREGULAR_WITH_LAND 512x512 f64, Taper filter_scale=16 dx_min, n_steps={n} (small grid: whole polynomial on the chip)",
           "n_steps": n, "value": shape[0] * shape[1] * n / t_chip, "unit": "cell-steps/s", "us_per_application": 1e6 * t_chip,
           "kernel": k_chip, "geometry": geom, "launches_per_application": 1 if "k_resident" in k_chip else None,
           "strip_marching": {"us_per_application": 1e6 * t_strip, "kernel": k_strip, "same_bits": bool(torch.equal(out.nan_to_num(), out2.nan_to_num()))},
           "dtype": "f64"}
    if not no_cpu:
        from oracle import gcmf_oracle as O
        fs = flt.filter_spec
        want = O.filter_func(O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq), "IRREGULAR_WITH_LAND", f, gv)
        got = out.cpu().numpy()
        rec["parity"] = {"rel_err": float(np.abs(got - want).max() / np.abs(want).max()), "tolerance": 1e-6,
                         "checked_against": "oracle, same grid / field / whole polynomial"}
    return rec


def run_midsize(dev, grid="IRREGULAR_WITH_LAND"):
    """The reference's own tutorial size (1080 x 1440, /docs/examples/example_tripole_grid.ipynb: a 1/4-degree ocean) with the headline's
    grid type and filter (IRREGULAR_WITH_LAND f64, Taper, filter_scale 16 dx_min, n_steps 63) -- and, second call, with the tutorial's own
    grid type (TRIPOLAR_POP_WITH_LAND, the seam included): too big for the on-chip kernel, small enough that the strips of the marching
    launches are short.  Not a BASELINE config; reported in `summary`."""
    import torch

    from gcm_filters_amd import Filter, FilterShape, GridType, testing as T

    shape = (1080, 1440)
    f, gv = T.scalar_case(grid, shape)
    dx = T.grid_dx_min(grid, gv)
    flt = Filter(filter_scale=16 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, grid_type=GridType[grid], grid_vars=gv)
    d = torch.from_numpy(f).to(dev)
    for _ in range(5):
        flt.apply(d)
    torch.cuda.synchronize()
    blocks = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(50):
            flt.apply(d)
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / 50)
    t = sorted(blocks)[2]
    n = int(flt.n_steps)
    return {"config": f"extra: {grid} 1080x1440 f64, Taper filter_scale=16 dx_min, n_steps={n} (the reference's tutorial size)",
            "n_steps": n, "value": shape[0] * shape[1] * n / t, "unit": "cell-steps/s", "us_per_application": 1e6 * t, "dtype": "f64"}


def run_single_launch(dev, args):
    """The north star's literal form on the headline workload: BASELINE config 3 with the whole n_steps polynomial in ONE persistent launch
    (csrc/gcmf_ringc_one.hip; opt-in: plan option "single_launch" / GCMF_SINGLE_LAUNCH=1) next to the default (seven back-to-back
    launches of nine levels), same process, alternating; same bits required."""
    import torch

    from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
    from gcm_filters_amd.kernels import ALL_KERNELS

    wl = T.baseline_workload(3, (args.ny, args.nx))
    fk = wl["fk"]
    flt = Filter(grid_type=GridType[wl["grid"]], grid_vars=wl["grid_vars"], filter_scale=fk["filter_scale"], dx_min=fk["dx_min"],
                 filter_shape=FilterShape[fk["filter_shape"]])
    cls = ALL_KERNELS[GridType[wl["grid"]]]
    plan = cls(*[wl["grid_vars"][k] for k in cls.required_grid_args()])._plan(_lib.F64, (args.ny, args.nx), dev.index)
    d = torch.from_numpy(wl["fields"][0]).to(dev)
    res, outs, kern = {0: [], 1: []}, {}, {}
    try:
        for rnd in range(3):
            for opt in (0, 1):
                plan.set_option("single_launch", opt)
                for _ in range(5):
                    flt.apply(d)
                torch.cuda.synchronize()
                plan.last_kernel()
                t0 = time.perf_counter()
                for _ in range(40):
                    outs[opt] = flt.apply(d)
                torch.cuda.synchronize()
                res[opt].append((time.perf_counter() - t0) / 40)
                kern[opt] = plan.last_kernel()
    finally:
        plan.set_option("single_launch", 0)
    n = int(flt.n_steps)
    cells = args.ny * args.nx
    t0, t1 = sorted(res[0])[1], sorted(res[1])[1]
    return {"config": f"extra: BASELINE config 3 with the whole polynomial in ONE persistent launch (opt-in; n_steps={n})",
            "n_steps": n, "value": cells * n / t1, "unit": "cell-steps/s", "us_per_application": 1e6 * t1, "kernel": kern[1],
            "launches_per_application": 1, "dtype": "f64",
            "back_to_back_launches": {"value": cells * n / t0, "us_per_application": 1e6 * t0, "kernel": kern[0]},
            "same_bits": bool(torch.equal(outs[0].nan_to_num(), outs[1].nan_to_num()))}


def build_summary(out):
    """The whole round in <= 1.5 KB, printed LAST in the line (the driver's record keeps the tail): per workload
    [G cell-steps/s, roofline frac (algorithmic bytes of one launch / launch time / 8 TB/s), counter traffic / algorithmic bytes, parity
    rel_err vs the imported reference's probes] -- None where a figure does not exist -- plus the host path's three numbers."""
    g = lambda v: None if v is None else round(v / 1e9, 1)
    r3 = lambda v: None if v is None else round(v, 3)
    e = lambda v: None if v is None else float(f"{v:.1e}")

    def row(rec, parity=None):
        rf = rec.get("roofline") or {}
        par = parity if parity is not None else (rec.get("parity") or {})
        err = par.get("rel_err", (par.get("reference_probes") or {}).get("rel_err"))
        return [g(rec.get("value")), r3(rf.get("frac")), r3(rf.get("traffic_over_alg_bytes")), e(err)]
    s = {"cols": ["G cell-steps/s", "frac", "traffic/alg", "parity rel_err"]}
    main_cfg = out["config"]["workload"].split(":")[0].split()[-1]
    s["cfg" + main_cfg] = row(out, out.get("parity"))
    for rec in out.get("extra_configs") or []:
        name = rec["config"]
        if name.startswith("BASELINE config"):
            key = "cfg" + name.split(":")[0].split()[-1]
        elif "512x512" in name:
            key = "onchip_512"
        elif "1080x1440" in name:
            key = "mid_1080x1440_pop" if "TRIPOLAR" in name else "mid_1080x1440"
        elif "ONE persistent launch" in name:
            key = "cfg3_one_launch"
        else:
            key = name[:24]
        s[key] = row(rec)
        opt = rec.get("forward_reference_opt_in")
        if opt:
            s[key + "_ref_scheme"] = row(opt)
    cb = out.get("cpu_baseline") or {}
    if cb:
        s["cpu_1core_M"] = round(cb["value"] / 1e6, 1)
    hp = out.get("host_path")
    if hp:
        s["host_ms"] = {"h2d": r3(hp.get("h2d_ms_page_locked")), "d2h": r3(hp.get("d2h_ms_page_locked")),
                        "pipeline": r3(hp.get("row_block_pipeline_ms")), "batch8_per_field": r3(hp.get("batch_of_8_ms_per_field"))}
    return s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=3, help="BASELINE.json config number (2..5), default 3")
    ap.add_argument("--ny", type=int, default=2400)
    ap.add_argument("--nx", type=int, default=3600)
    ap.add_argument("--nlev", type=int, default=0, help="vertical levels of config 5 (default 50) / config 6 (default 1)")
    ap.add_argument("--f32", action="store_true", help="config 6 only: f32 state instead of f64")
    ap.add_argument("--f64", action="store_true", help="config 5 only: f64 state instead of the BASELINE's f32")
    ap.add_argument("--filter-scale", type=float, default=0.0, help="filter scale in dx_min units (0 = the config's own)")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="N>1, scalar configs: strong = one (ny, nx) grid cut into N row slabs (reported as value); "
                         "weak = every GPU owns ny rows of an (N*ny, nx) grid")
    ap.add_argument("--no-weak", action="store_true", help="N>1: skip the second (weak-scaling) measurement")
    ap.add_argument("--batch-levels", type=int, default=16,
                    help="N>1, scalar configs: time levels of the third measurement -- the same grid cut N ways with a BATCH of fields "
                         "(strips get tall again on short slabs: the strong-scaling workload that can use 8 GPUs); 0 skips it")
    ap.add_argument("--halo", type=int, default=0, help="N>1: ghost rows per exchange (0 = auto)")
    ap.add_argument("--exchange", choices=["auto", "native", "torch", "p2p"], default="auto",
                    help="N>1 halo exchange: native = RCCL send / recv issued by libgcmf on a side stream; torch = torch.distributed P2P; "
                         "p2p = peer stores into IPC-mapped mailboxes + flags on the compute stream (csrc/gcmf_p2p.hip, one node)")
    ap.add_argument("--full", action="store_true",
                    help="--gpus 1: besides the headline figure, measure and check everything else (roofline of the dominant kernel, parity "
                         "against the oracle and the reference probes, cpu_baseline, extra_configs, host_path, summary); without it the run "
                         "sets up, warms up, times the K steps, writes --dump-outputs and prints the result line")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg (and the oracle parity check)")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the extra_configs measurements (configs 1, 2, 4, 5, the smaller grids, "
                                                            "the single launch) and host_path")
    ap.add_argument("--no-replan", action="store_true", help="keep ONE plan for all timed blocks (profiling runs: one placement)")
    ap.add_argument("--kinds", action="store_true", help="instead of the BASELINE line: one roofline record per Laplacian kind that is not a "
                    "BASELINE config (B-grid, MOM5U/T, the area-weighted and tripolar regular kinds) at --ny x --nx (tools/bench_kinds.py)")
    ap.add_argument("--kinds-only", default="", help="--kinds: comma-separated subset of the kind names")
    ap.add_argument("--cpu-steps", type=int, default=64, help="Laplacian steps of the CPU sample")
    ap.add_argument("--rows-per-wave", type=int, default=0)
    ap.add_argument("--xcd-remap", type=int, default=-1)
    ap.add_argument("--multi", type=int, default=0, help="recurrence steps fused per HBM pass (0 = library default, 1 = off)")
    ap.add_argument("--strip", type=int, default=0, help="rows per wave strip of the temporally blocked kernel (0 = auto)")
    ap.add_argument("--prefetch", type=int, default=0, help="operand rows in flight per wave (0 = default)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB "
                         "in all: larger outputs as a fixed, seeded sample of their cells); --gpus 1 only")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64_000_000
DUMP_SEED = 20240601


def dump_outputs(outs, directory):
    """Write the outputs of the timed path's last step to `directory` as <name>.npy: `filtered` (a scalar field) or `filtered_u` /
    `filtered_v` (a vector field), in the dtype the caller received.  When they exceed DUMP_LIMIT_BYTES together, every array is
    replaced by the same share of its cells, picked from the flattened array by a generator with a fixed seed and kept in flat-index
    order: the same arguments give the same cells, run after run and build after build.  Returns a record for the result line."""
    import torch

    names = ["filtered"] if len(outs) == 1 else ["filtered_u", "filtered_v"]
    total = sum(o.numel() * o.element_size() for o in outs)
    budget = DUMP_LIMIT_BYTES - 1024 * len(outs)          # (room for the .npy headers)
    frac = 1.0 if total <= budget else budget / total
    os.makedirs(directory, exist_ok=True)
    rec = {"dir": directory, "files": {}, "sampled": frac < 1.0, "seed": DUMP_SEED if frac < 1.0 else None}
    for k, (name, o) in enumerate(zip(names, outs)):
        if o.dtype not in (torch.float32, torch.float64):
            raise SystemExit(f"bench.py --dump-outputs: output {name} has dtype {o.dtype}, not float32 / float64")
        if frac < 1.0:
            n = o.numel()
            rng = np.random.default_rng([DUMP_SEED, k])
            idx = np.unique(rng.integers(0, n, size=int(n * frac)))
            arr = o.reshape(-1)[torch.from_numpy(idx).to(o.device)].cpu().numpy()
        else:
            arr = o.cpu().numpy()
        path = os.path.join(directory, name + ".npy")
        np.save(path, arr)
        rec["files"][name] = {"shape": list(arr.shape), "of_shape": list(o.shape), "dtype": str(arr.dtype)}
    return rec


def main_single(args):
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tuned = bool(args.rows_per_wave or args.xcd_remap >= 0 or args.multi or args.strip or args.prefetch)
    # north-star gate (fp64).  f32 state: SURVEY 8d's gate is 1e-4; held to 1e-5 here -- config 5 (n_steps 44) measures 1.1e-6 against
    # the reference's probes (the reference's own f32 path is 3e-6 off f64 arithmetic, the default here 1.8e-6)
    tol = lambda itemsize: 1e-6 if itemsize == 8 else 1e-5
    r = run_single(args.config, args, dev, args.steps, args.warmup, scale=args.filter_scale, tuned=tuned, kernel_timing=args.full)
    sp = spread_of(r)
    fk = r["fk"]
    out = {
        "metric": "grid-cells*Laplacian-steps/sec", "value": sp["value"], "unit": "cell-steps/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": sp["ms_per_step"],
        # the K timed applications ran as `blocks` synchronised blocks; value = the median block, the plan was folded anew between two
        # of them (a plan's placement in HBM decides between two launch-time modes ~10 % apart)
        "value_min": sp["value_min"], "value_max": sp["value_max"], "value_mean": sp["value_mean"],
        "timing": {k: sp[k] for k in ("blocks", "applications_per_block", "block_ms", "plans_refolded_between_blocks")},
        # N = 1 is the first point of the strong-scaling curve `--gpus N` reports (same global grid at every N)
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f64" if r["itemsize"] == 8 else "f32", "data": "synthetic",
        "config": {"workload": workload_name(args.config, r, args),
                   "filter": f"{fk['filter_shape']} filter_scale={fk['filter_scale']:.6g} dx_min={fk['dx_min']:.6g}",
                   "n_steps": r["n_steps"], "global_grid": [args.ny, args.nx], "parallelism": "single GPU"},
    }
    if args.full:
        out["roofline"] = roofline_of(args.config, r, args.steps, not tuned)
    if args.dump_outputs:
        out["dump_outputs"] = dump_outputs(r["outs"], args.dump_outputs)
    if not args.full:   # a plain run: the headline figure and nothing else
        print(json.dumps(out))
        return 0
    nbatch_main = r["nbatch"]
    failed = []
    # ---- parity of the TIMED workload's output -----------------------------------------------------------------
    parity = {"tolerance": tol(r["itemsize"])}
    chk = golden_probe_check(args.config, args.filter_scale, (args.ny, args.nx), r["outs"])
    if chk is not None:
        parity["reference_probes"] = finish_probe_check(chk)
        if not parity["reference_probes"]["rel_err"] <= parity["tolerance"]:
            failed.append(f"reference probes: rel_err {parity['reference_probes']['rel_err']:.3e}")
    if not args.no_cpu:
        cpu, want, n_cpu = cpu_baseline(r["wl"], args.cpu_steps)
        out["cpu_baseline"] = cpu
        if n_cpu == r["n_steps"]:
            got = [o if o.ndim == 2 else o[0] for o in r["outs"]]
            what = "oracle, same grid / field / whole polynomial as the timed workload" + (" (level 0)" if r["nbatch"] > 1 else "")
        else:  # the CPU sample ran a truncated polynomial: one more (untimed) GPU application with the same one
            from gcm_filters_amd import filter as F
            spec = r["flt"].filter_spec
            short = F.FilterSpec(n_cpu, spec.s_max, np.asarray(spec.p)[: n_cpu + 1], spec.dx_min_sq)
            lev0 = [d if d.ndim == 2 else d[:1] for d in r["d_in"]]
            cls = r["flt"].Laplacian
            gargs = [r["wl"]["grid_vars"][k] for k in cls.required_grid_args()]
            if len(lev0) == 2:
                got = F._create_filter_func_vec(short, cls)(lev0[0], lev0[1], *gargs)
            else:
                got = (F._create_filter_func(short, cls)(lev0[0], *gargs),)
            got = [g.reshape(g.shape[-2:]) for g in got]
            what = f"oracle, same grid / field, polynomial truncated to n_steps={n_cpu} on both sides (level 0)"
        err, same = rel_err_and_nan([g.cpu().numpy() for g in got], want)
        parity.update({"rel_err": err, "nan_pattern_equal": same, "checked_against": what})
        if not (err <= parity["tolerance"] and same):
            failed.append(f"oracle: rel_err {err:.3e}, nan_pattern_equal {same}")
        del want
    else:
        out["cpu_baseline"] = None
    out["parity"] = parity
    # ---- the other BASELINE configs, briefly ---------------------------------------------------------------------
    if not args.no_extra:
        extras = [run_config1(dev)]
        if not extras[0].get("parity", {"rel_err": 0})["rel_err"] <= 1e-6:
            failed.append(f"config 1 reference probe: rel_err {extras[0]['parity']['rel_err']:.3e}")
        small = run_small_onchip(dev, args.no_cpu)
        if not small.get("parity", {"rel_err": 0})["rel_err"] <= 1e-6 or not small["strip_marching"]["same_bits"]:
            failed.append(f"small on-chip grid: parity {small.get('parity')} same bits as the strip-marching launches: {small['strip_marching']['same_bits']}")
        for cfg in (2, 4, 5):
            if cfg == args.config:
                continue
            r = None
            free_gpu()
            # an application of configs 2 / 4 takes ~1 ms: three of them after the idle seconds of the CPU leg are timed on a
            # GPU that has not clocked up again (measured 7 % low); config 5 takes 70 ms per application
            xs, xw = (5, 2) if cfg == 5 else (50, 5)
            r = run_single(cfg, args, dev, steps=xs, warmup=xw)
            xsp = spread_of(r)
            rec = {"config": workload_name(cfg, r, args), "n_steps": r["n_steps"], "steps": xs, "warmup": xw,
                   "value": xsp["value"], "value_min": xsp["value_min"], "value_max": xsp["value_max"], "unit": "cell-steps/s",
                   "ms_per_step": xsp["ms_per_step"], "dtype": "f64" if r["itemsize"] == 8 else "f32",
                   "roofline": roofline_of(cfg, r, xs, True)}
            chk = golden_probe_check(cfg, 0.0, (args.ny, args.nx), r["outs"])
            if chk is not None:
                rec["parity"] = dict(finish_probe_check(chk), tolerance=tol(r["itemsize"]))
                if not rec["parity"]["rel_err"] <= rec["parity"]["tolerance"]:
                    failed.append(f"config {cfg} reference probes: rel_err {rec['parity']['rel_err']:.3e}")
            if cfg == 5 and not args.no_cpu:
                rec["cpu_baseline_pool"] = cpu_baseline_pool(5, args.ny, args.nx, r["nbatch"], 4)
            if cfg == 5:
                # The default carries the whole polynomial in f32 (backward evaluation, k_cgrid_ring); the reference sums f32 fields in an f64
                # running sum (NumPy >= 2 promotion, reference filter.py:192-206).  Filter(evaluation="reference") runs exactly that scheme
                # (forward recurrence, f64 fbar): measured here so that the like-for-like figure is on record next to the default.
                r2 = None
                free_gpu()
                r2 = run_single(cfg, args, dev, steps=xs, warmup=xw, evaluation="reference")
                osp = spread_of(r2)
                opt = {"evaluation": "reference",   # forward recurrence, f32 T_k, f64 running sum: the reference's own scheme (NOT the default)
                       "kernel": r2["kernel"], "value": osp["value"], "value_min": osp["value_min"], "value_max": osp["value_max"], "unit": "cell-steps/s",
                       "ms_per_step": osp["ms_per_step"], "roofline": roofline_of(cfg, r2, xs, True)}
                chk2 = golden_probe_check(cfg, 0.0, (args.ny, args.nx), r2["outs"])
                if chk2 is not None:
                    opt["parity"] = dict(finish_probe_check(chk2), tolerance=tol(r2["itemsize"]))
                    if not opt["parity"]["rel_err"] <= opt["parity"]["tolerance"]:
                        failed.append(f"config {cfg} forward (reference) evaluation: rel_err {opt['parity']['rel_err']:.3e}")
                rec["forward_reference_opt_in"] = opt
                r2 = None
            if cfg == 2:
                # The default since round 4 evaluates the land-mask (and REGULAR) types backwards too (k_ringc: fused multiply-adds,
                # one plane less, <= 1e-14 from numpy).  Filter(evaluation="reference") is the escape that stays bit-exact with
                # numpy (the reference's forward recurrence, k_ring): measured here so that the price of bit-exactness is on record.
                r2 = None
                free_gpu()
                r2 = run_single(cfg, args, dev, steps=xs, warmup=xw, evaluation="reference")
                osp = spread_of(r2)
                opt = {"evaluation": "reference", "kernel": r2["kernel"],
                       "value": osp["value"], "value_min": osp["value_min"], "value_max": osp["value_max"], "unit": "cell-steps/s",
                       "ms_per_step": osp["ms_per_step"]}
                chk2 = golden_probe_check(cfg, 0.0, (args.ny, args.nx), r2["outs"])
                if chk2 is not None:
                    opt["parity"] = dict(finish_probe_check(chk2), tolerance=tol(r2["itemsize"]))
                    if not opt["parity"]["rel_err"] <= opt["parity"]["tolerance"]:
                        failed.append(f"config {cfg} forward (reference) evaluation: rel_err {opt['parity']['rel_err']:.3e}")
                rec["forward_reference_opt_in"] = opt
            extras.append(rec)
        extras.append(small)
        extras.append(run_midsize(dev))
        extras.append(run_midsize(dev, "TRIPOLAR_POP_WITH_LAND"))
        if args.config == 3 and (args.ny, args.nx) == (2400, 3600):
            one = run_single_launch(dev, args)
            if not one["same_bits"] or "k_ringc_one" not in one["kernel"]:
                failed.append(f"single launch: same bits {one['same_bits']}, kernel {one['kernel']}")
            extras.append(one)
        out["extra_configs"] = extras
        if args.config == 3 and (args.ny, args.nx) == (2400, 3600):
            r = None
            free_gpu()
            out["host_path"] = run_host_path(dev, args)
    if args.config == 5 and not args.no_cpu:
        out["cpu_baseline_pool"] = cpu_baseline_pool(5, args.ny, args.nx, nbatch_main, 4)
    out["summary"] = build_summary(out)   # LAST key: the tail of the line carries every config's value / frac / traffic / parity
    print(json.dumps(out))
    if failed:
        print("bench.py: PARITY FAILURE -- " + "; ".join(failed), file=sys.stderr)
        return 1
    return 0


def main():
    args = parse()
    if args.nlev <= 0 and args.config == 6:
        args.nlev = 0
    if args.dump_outputs and (args.gpus > 1 or args.kinds):
        raise SystemExit("bench.py: --dump-outputs writes the single-GPU workload's outputs (--gpus 1, not --kinds)")
    world = int(os.environ.get("WORLD_SIZE", "0"))
    if world == 0 and args.gpus > 1:
        from bench_multi import self_launch
        self_launch(args)  # does not return
    world = max(world, 1)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if args.kinds:
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import bench_kinds
        return bench_kinds.main(args)
    if world == 1:
        return main_single(args)
    from bench_multi import main_multi
    return main_multi(args, world, int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")))


if __name__ == "__main__":
    sys.exit(main())
