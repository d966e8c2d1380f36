#!/usr/bin/env python3
"""Regenerate the golden vectors in this directory.  Runs ONLY where /root/reference is mounted.

Outputs (committed):
  reference_zarr.npz       the reference's own 18 known-answer arrays
                           (tests/test_data_kernels/*.zarr, tests/test_data_filter/*.zarr upstream),
                           decoded from their Blosc/LZ4 zarr-v2 chunks to float32 numpy arrays.
  reference_generated.npz  float64 outputs obtained by *importing the reference* (with a stub for its
                           one missing import, xarray) and running its kernels / filter_func on the seeded
                           inputs of gcm_filters_amd.testing.  Inputs are NOT stored -- tests rebuild them
                           from the same seeds.  The case list is `CASES` below; its keys are the npz keys.
  reference_spec.npz       n_steps defaults and Chebyshev coefficients p[] from the reference for a table
                           of (shape, scale, dx_min, transition_width, ndim, n_steps).
  reference_fullsize.npz   (`--fullsize`, ~6 min of reference time) BASELINE configs 2-5 at 2400 x 3600 run through the
                           imported reference with their full polynomials: 300 seeded (j, i) probes of the output +
                           sum / sum of squares / max-abs per case (the planes themselves are too big to
                           store).  Inputs come from gcm_filters_amd.testing.baseline_workload, like bench.py's.

  reference_gridbatched.npz (`--gridbatched`) grid variables with a leading level dim (wet_mask(z, y, x), kappa(z, y, x), ...)
                           against fields of shape (2, z, y, x): L(f) and the Gaussian filter from the imported reference.

  reference_coastlines.npz, reference_coastlines_lap.npz (`--coastlines`) every land kind x every coastline of
                           gcm_filters_amd.testing.COASTLINES (and two C-grid mask variants) at 40 x 64: the 24-step Gaussian filter
                           and L(f) from the imported reference, in three treatments of the values on land.

  reference_vector_metrics.npz (`--vector-metrics`) both vector kinds at 40 x 64 on testing.vector_grid_vars_irregular -- metric planes that
                           all differ and vary along both axes, B-grid coupling weights that are not zero: L(u, v), the Gaussian at
                           8 dx_min and the Taper at 4 dx_min from the imported reference; the C-grid also on a speckle coastline.

`--out DIR` writes into DIR instead of this directory (to check that the committed files regenerate).

No reference source text is copied anywhere: only numbers leave this script.
"""
import ctypes
import ctypes.util
import json
import os
import struct
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


# ------------------------------------------------------------------------------------------------
# zarr-v2 / Blosc-1 / LZ4 single-chunk decoder (no zarr / numcodecs in this image)
# ------------------------------------------------------------------------------------------------
def _lz4():
    lib = ctypes.CDLL(ctypes.util.find_library("lz4") or "liblz4.so.1")
    lib.LZ4_decompress_safe.restype = ctypes.c_int
    lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    return lib


def blosc1_decompress(buf: bytes) -> bytes:
    version, versionlz, flags, typesize, nbytes, blocksize, cbytes = struct.unpack_from("<BBBBIII", buf, 0)
    assert cbytes == len(buf), (cbytes, len(buf))
    if flags & 0x2:  # memcpyed
        return buf[16:16 + nbytes]
    assert (flags >> 5) == 1, "expected the LZ4 codec"
    shuffled = bool(flags & 0x1)
    nblocks = (nbytes + blocksize - 1) // blocksize
    bstarts = struct.unpack_from(f"<{nblocks}I", buf, 16)
    lz4 = _lz4()
    out = bytearray()
    for b in range(nblocks):
        bsize = min(blocksize, nbytes - b * blocksize)
        leftover = bsize != blocksize
        # blosc splits a block into `typesize` streams unless it is the leftover block / split disabled
        nsplits = typesize if (not (flags & 0x10) and not leftover and typesize <= 16 and bsize // typesize >= 128) else 1
        pos = bstarts[b]
        block = bytearray()
        for _ in range(nsplits):
            (csize,) = struct.unpack_from("<i", buf, pos)
            pos += 4
            want = bsize // nsplits
            if csize == want:
                block += buf[pos:pos + csize]
            else:
                dst = ctypes.create_string_buffer(want)
                got = lz4.LZ4_decompress_safe(buf[pos:pos + csize], dst, csize, want)
                assert got == want, (got, want)
                block += dst.raw
            pos += csize
        if shuffled and typesize > 1:
            n = bsize // typesize
            arr = np.frombuffer(bytes(block[: n * typesize]), dtype=np.uint8).reshape(typesize, n).T.copy()
            block = bytearray(arr.tobytes()) + block[n * typesize:]
        out += block
    assert len(out) == nbytes
    return bytes(out)


def read_zarr_array(path: str) -> np.ndarray:
    meta = json.load(open(os.path.join(path, ".zarray")))
    assert meta["zarr_format"] == 2 and meta["order"] == "C" and meta["chunks"] == meta["shape"]
    assert meta["compressor"]["id"] == "blosc" and meta["filters"] is None
    chunk = ".".join(["0"] * len(meta["shape"]))
    raw = blosc1_decompress(open(os.path.join(path, chunk), "rb").read())
    return np.frombuffer(raw, dtype=np.dtype(meta["dtype"])).reshape(meta["shape"]).copy()


# ------------------------------------------------------------------------------------------------
# import the reference (its only unavailable import is xarray; the array-level path never uses it)
# ------------------------------------------------------------------------------------------------
def import_reference():
    xr = types.ModuleType("xarray")

    class _Unused:
        def __init__(self, *a, **k):
            pass

    xr.Dataset = xr.DataArray = _Unused
    sys.modules.setdefault("xarray", xr)
    sys.path.insert(0, REF)
    import gcm_filters.filter as rf
    import gcm_filters.kernels as rk
    return rf, rk


# ------------------------------------------------------------------------------------------------
# case table for reference_generated.npz -- also imported by the tests to rebuild the inputs
# ------------------------------------------------------------------------------------------------
SMALL = (40, 64)


def build_case(name: str):
    """Return (grid_type, fields tuple, grid_vars, filter kwargs or None) for a case key."""
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    parts = name.split("/")
    grid, kind = parts[0], parts[1]
    variant = parts[2] if len(parts) > 2 else "base"
    shape = (128, 256) if variant == "full" else SMALL
    vec = grid in T.VECTOR_GRIDS
    if vec:
        fields, gv = T.vector_case(grid, shape)
    else:
        f, gv = T.scalar_case(grid, shape)
        fields = (f,)
    if variant == "kappa":  # spatially varying kappa <= 1 with max exactly 1
        if grid == "IRREGULAR_WITH_LAND":
            gv["kappa_w"] = T.smooth_kappa(shape, 11)
            gv["kappa_s"] = T.smooth_kappa(shape, 12)
        elif grid == "VECTOR_C_GRID":
            gv["kappa_iso"] = T.smooth_kappa(shape, 13)
            gv["kappa_aniso"] = 0.5 * T.smooth_kappa(shape, 14)
    if variant == "nanland":  # NaN on land cells of the input
        mk = [k for k in gv if k.startswith("wet_mask")][0]
        fields = tuple(np.where(gv[mk] == 0, np.nan, f) for f in fields)
    if variant == "batched":
        fields = tuple(np.stack([np.stack([T.random_field(shape, 1000 + 10 * a + b + 100 * c) for b in range(2)])
                                 for a in range(3)]) for c, _ in enumerate(fields))
    if variant == "f32":
        fields = tuple(f.astype(np.float32) for f in fields)
    if variant == "allf32":
        fields = tuple(f.astype(np.float32) for f in fields)
        gv = {k: v.astype(np.float32) for k, v in gv.items()}
    if variant == "zeroarea" and grid == "VECTOR_C_GRID":
        gv["area_u"] = gv["area_u"].copy()
        gv["area_v"] = gv["area_v"].copy()
        gv["area_u"][5:9, 7:12] = 0
        gv["area_v"][20:22, 30:40] = 0
    dimensional = grid in ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T", "TRIPOLAR_POP_WITH_LAND") or vec
    dx_min = T.grid_dx_min(grid, gv) if dimensional else 1.0
    fk = None
    if kind == "gauss":
        fk = dict(filter_scale=8.0 * dx_min, dx_min=dx_min, filter_shape="GAUSSIAN", n_steps=0)
    elif kind == "gauss_ref":  # exactly the upstream validation-test filter (dx_min = 1 on every grid)
        fk = dict(filter_scale=8.0, dx_min=1.0, filter_shape="GAUSSIAN", n_steps=0)
    elif kind == "taper":
        fk = dict(filter_scale=4.0 * dx_min, dx_min=dx_min, filter_shape="TAPER", n_steps=0)
    elif kind == "lap":
        fk = None
    else:
        raise KeyError(kind)
    return grid, fields, gv, fk


def case_names():
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    names = []
    for g in T.ALL_GRIDS:
        names += [f"{g}/lap", f"{g}/gauss", f"{g}/taper", f"{g}/gauss/batched", f"{g}/gauss/f32",
                  f"{g}/gauss/allf32"]
        if g in ("MOM5U", "MOM5T"):
            names += [f"{g}/lap/full", f"{g}/gauss_ref/full"]
        if any(k.startswith("wet_mask") for k in T.FIXTURE_ARG_ORDER[g]):
            names += [f"{g}/gauss/nanland", f"{g}/lap/nanland"]
    names += ["IRREGULAR_WITH_LAND/lap/kappa", "IRREGULAR_WITH_LAND/taper/kappa",
              "VECTOR_C_GRID/lap/kappa", "VECTOR_C_GRID/gauss/kappa", "VECTOR_C_GRID/lap/zeroarea"]
    names += ["REGULAR/config1"]
    return names


SPEC_TABLE = [
    # (shape, filter_scale, dx_min, transition_width, ndim, n_steps)
    ("GAUSSIAN", 10.0, 1.0, np.pi, 2, 0), ("TAPER", 2.0, 1.0, np.pi, 1, 0),
    ("GAUSSIAN", 4.0, 1.0, np.pi, 2, 16), ("GAUSSIAN", 8.0, 1.0, np.pi, 2, 0), ("GAUSSIAN", 50.0, 1.0, np.pi, 2, 0),
    ("TAPER", 4.0, 1.0, np.pi, 2, 0), ("TAPER", 16.0, 1.0, np.pi, 2, 0), ("TAPER", 8.0, 1.0, 2.0, 2, 0),
    ("TAPER", 14.4, 0.9, np.pi, 2, 0), ("GAUSSIAN", 8.0, 2.0, np.pi, 2, 0), ("GAUSSIAN", 3.0, 1.0, np.pi, 2, 0),
    ("TAPER", 5.0, 1.0, np.pi, 2, 10), ("GAUSSIAN", 6.0, 1.0, np.pi, 3, 12), ("GAUSSIAN", 5.0, 1.0, np.pi, 1, 0),
    ("TAPER", 32.0, 1.0, np.pi, 2, 0), ("TAPER", 6.0, 1.5, 1.5, 1, 0),
]


# ------------------------------------------------------------------------------------------------
# grid variables with leading (level) dims: reference_gridbatched.npz -- case builder shared with the tests
# ------------------------------------------------------------------------------------------------
GRIDBATCHED_GRIDS = ["REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "TRIPOLAR_POP_WITH_LAND",
                     "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "VECTOR_C_GRID", "VECTOR_B_GRID"]


def build_gridbatched_case(grid: str):
    """(fields, grid_vars, filter kwargs): a 3-level problem whose wet mask (and kappa / a metric) differs per level while the
    other grid variables stay 2-D; fields have shape (2, 3, ny, nx) -- the leading 2 broadcasts against the grid variables."""
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    shape, nlev = SMALL, 3
    ny, nx = shape
    vec = grid in T.VECTOR_GRIDS
    gv = T.vector_grid_vars(grid, shape) if vec else T.scalar_grid_vars(grid, shape)

    def per_level(mask2d):
        m = np.stack([mask2d.copy() for _ in range(nlev)])
        for l in range(nlev):  # an island that grows with depth (never in the southernmost row)
            m[l, ny // 2 + 2: ny // 2 + 4 + 2 * l, nx // 2 + 3: nx // 2 + 6 + 3 * l] = 0
        return m

    for k in list(gv):
        if k.startswith("wet_mask"):
            gv[k] = per_level(gv[k])
    if grid == "IRREGULAR_WITH_LAND":  # kappa_w varies per level and reaches 1 only on level 0 (the reference tests the whole array)
        kw = np.stack([T.smooth_kappa(shape, 21 + l) * (1.0 if l == 0 else 0.8) for l in range(nlev)])
        gv["kappa_w"] = kw
        gv["kappa_s"] = 0.9 * T.smooth_kappa(shape, 31)
    if grid == "VECTOR_C_GRID":
        gv["kappa_iso"] = np.stack([T.smooth_kappa(shape, 41 + l) for l in range(nlev)])
    if grid == "VECTOR_B_GRID":  # no mask: let a metric depend on the level instead
        gv["TAREA"] = np.stack([gv["TAREA"] * (1.0 + 0.05 * l) for l in range(nlev)])
    ncomp = 2 if vec else 1
    fields = tuple(np.stack([np.stack([T.random_field(shape, 500 + 100 * c + 10 * a + l) for l in range(nlev)])
                             for a in range(2)]) for c in range(ncomp))
    dimensional = grid in ("IRREGULAR_WITH_LAND", "TRIPOLAR_POP_WITH_LAND") or vec
    dx_min = T.grid_dx_min(grid, gv) if dimensional else 1.0
    fk = dict(filter_scale=6.0 * dx_min, dx_min=dx_min, filter_shape="GAUSSIAN", n_steps=0)
    return fields, gv, fk


def make_gridbatched(rf, rk, outdir):
    out = {}
    for grid in GRIDBATCHED_GRIDS:
        fields, gv, fk = build_gridbatched_case(grid)
        cls = rk.ALL_KERNELS[rk.GridType[grid]]
        args = [gv[k] for k in cls.required_grid_args()]
        with np.errstate(all="ignore"):
            res = cls(**gv)(*fields)
            out[f"{grid}/lap/gridbatched"] = np.stack(res) if isinstance(res, tuple) else np.asarray(res)
            shape = rf.FilterShape[fk["filter_shape"]]
            n = rf._compute_n_steps_default(2, shape, fk["filter_scale"], fk["dx_min"], np.pi)
            spec = rf._compute_filter_spec(fk["filter_scale"], fk["dx_min"], shape, np.pi, 2, n)
            if len(fields) == 2:
                res = np.stack(rf._create_filter_func_vec(spec, cls)(*fields, *args))
            else:
                res = np.asarray(rf._create_filter_func(spec, cls)(*fields, *args))
        out[f"{grid}/gauss/gridbatched"] = res
        print(grid, "n_steps", int(n), res.shape, flush=True)
    np.savez_compressed(os.path.join(outdir, "reference_gridbatched.npz"), **out)
    print("reference_gridbatched.npz:", len(out), "arrays")


# ------------------------------------------------------------------------------------------------
# coastlines the fixture mask never draws: reference_coastlines.npz -- case builder shared with the tests
# ------------------------------------------------------------------------------------------------
COAST_LAND_GRIDS = ["REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5U", "MOM5T",
                    "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "TRIPOLAR_POP_WITH_LAND"]
COAST_FILES = {"gauss": "reference_coastlines.npz", "lap": "reference_coastlines_lap.npz"}


def coast_case_names():
    """`grid/coastline[/variant]`: every land kind x every coastline defined for it, IRREGULAR_WITH_LAND with kappa zeros, and the two
    C-grid mask variants.  A case's position in this list seeds its coastline and picks its land treatment."""
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    names = [f"{g}/{c}" for g in COAST_LAND_GRIDS for c in T.coastline_names(g.startswith("TRIPOLAR"))]
    names += ["IRREGULAR_WITH_LAND/speckle/kappa", "IRREGULAR_WITH_LAND/one_land_cell/kappa"]
    names += ["VECTOR_C_GRID/speckle/derived_q", "VECTOR_C_GRID/channels/independent_q"]
    return names


def build_coast_case(name: str, shape=SMALL):
    """(grid, fields, grid_vars, filter kwargs) of a coastline case: the seeded field of scalar_case / vector_case, land treated as
    NaN on all land / finite on all land / NaN on half the land and in three wet cells, cycling over the cases (the C-grid, whose
    stencil does not mask its input, keeps finite values)."""
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    k = coast_case_names().index(name)
    parts = name.split("/")
    grid, coast = parts[0], parts[1]
    variant = parts[2] if len(parts) > 2 else ""
    if grid == "VECTOR_C_GRID":
        fields, _ = T.vector_case(grid, shape)
        gv = T.cgrid_coast_vars(coast, shape, seed=k, independent_q=variant == "independent_q")
    else:
        f, gv = T.scalar_case(grid, shape)
        gv["wet_mask"] = T.coastline(coast, shape, seed=k, tripolar=grid.startswith("TRIPOLAR"), cuts=(10,))
        if variant == "kappa":
            gv["kappa_w"], gv["kappa_s"] = T.kappa_with_zeros(shape)
        fields = (T.treat_land(f, gv["wet_mask"], T.LAND_TREATMENTS[k % 3], seed=k),)
    dimensional = grid in ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T", "TRIPOLAR_POP_WITH_LAND", "VECTOR_C_GRID")
    dx_min = T.grid_dx_min(grid, gv) if dimensional else 1.0
    return grid, fields, gv, dict(filter_scale=8.0 * dx_min, dx_min=dx_min, filter_shape="GAUSSIAN", n_steps=24)


def make_coastlines(rf, rk, outdir):
    """The reference's Laplacian and 24-step Gaussian filter on every coastline case.  One file per kind of array, 1.7 MB together:
    this repository takes no new file above 1 MiB (the larger fixtures beside them are older than that rule), and 60 planes of either
    kind compress to 0.96 / 0.74 MB."""
    out = {"gauss": {}, "lap": {}}
    for name in coast_case_names():
        grid, fields, gv, fk = build_coast_case(name)
        cls = rk.ALL_KERNELS[rk.GridType[grid]]
        args = [gv[k] for k in cls.required_grid_args()]
        with np.errstate(all="ignore"):
            res = cls(**gv)(*fields)
            out["lap"][name] = np.stack(res) if isinstance(res, tuple) else np.asarray(res)
            spec = rf._compute_filter_spec(fk["filter_scale"], fk["dx_min"], rf.FilterShape[fk["filter_shape"]], np.pi, 2, fk["n_steps"])
            if len(fields) == 2:
                res = np.stack(rf._create_filter_func_vec(spec, cls)(*fields, *args))
            else:
                res = np.asarray(rf._create_filter_func(spec, cls)(*fields, *args))
        out["gauss"][name] = res
    for kind, fname in COAST_FILES.items():
        np.savez_compressed(os.path.join(outdir, fname), **out[kind])
        print(f"{fname}: {len(out[kind])} arrays, {sum(v.nbytes for v in out[kind].values()) // 1024} KiB raw, "
              f"{os.path.getsize(os.path.join(outdir, fname)) // 1024} KiB on disk")


# ------------------------------------------------------------------------------------------------
# the vector kinds on metric planes that differ from one another: reference_vector_metrics.npz -- case builder shared with the tests
# ------------------------------------------------------------------------------------------------
VECTOR_METRICS_FILE = "reference_vector_metrics.npz"


def vector_metrics_case_names():
    """`grid/kind[/speckle_indq]`: L(u, v), the Gaussian at 8 dx_min and the Taper at 4 dx_min (default step counts) for both vector kinds
    on testing.vector_grid_vars_irregular; the C-grid's Laplacian and Gaussian also on a speckle coastline with a wet_mask_q of its own."""
    names = [f"{g}/{k}" for g in ("VECTOR_C_GRID", "VECTOR_B_GRID") for k in ("lap", "gauss", "taper")]
    return names + ["VECTOR_C_GRID/lap/speckle_indq", "VECTOR_C_GRID/gauss/speckle_indq"]


def build_vector_metrics_case(name: str, shape=SMALL):
    """(grid, fields, grid_vars, filter kwargs or None) of a case of vector_metrics_case_names(): the seeded fields of vector_case."""
    sys.path.insert(0, REPO)
    from gcm_filters_amd import testing as T

    parts = name.split("/")
    grid, kind = parts[0], parts[1]
    coast = dict(coast="speckle", independent_q=True) if len(parts) > 2 else {}
    fields = (T.random_field(shape, 42), T.random_field(shape, 43))
    gv = T.vector_grid_vars_irregular(grid, shape, **coast)
    dx_min = T.grid_dx_min(grid, gv)
    fk = {"lap": None, "gauss": dict(filter_scale=8.0 * dx_min, dx_min=dx_min, filter_shape="GAUSSIAN", n_steps=0),
          "taper": dict(filter_scale=4.0 * dx_min, dx_min=dx_min, filter_shape="TAPER", n_steps=0)}[kind]
    return grid, fields, gv, fk


def make_vector_metrics(rf, rk, outdir):
    out = {}
    for name in vector_metrics_case_names():
        grid, fields, gv, fk = build_vector_metrics_case(name)
        cls = rk.ALL_KERNELS[rk.GridType[grid]]
        args = [gv[k] for k in cls.required_grid_args()]
        with np.errstate(all="ignore"):
            if fk is None:
                res = cls(**gv)(*fields)
            else:
                shape = rf.FilterShape[fk["filter_shape"]]
                n = rf._compute_n_steps_default(2, shape, fk["filter_scale"], fk["dx_min"], np.pi)
                spec = rf._compute_filter_spec(fk["filter_scale"], fk["dx_min"], shape, np.pi, 2, n)
                res = rf._create_filter_func_vec(spec, cls)(*fields, *args)
        out[name] = np.stack(res)
        assert out[name].dtype == np.float64 and np.isfinite(out[name]).all(), name
    path = os.path.join(outdir, VECTOR_METRICS_FILE)
    np.savez_compressed(path, **out)
    print(f"{VECTOR_METRICS_FILE}: {len(out)} arrays, {sum(v.nbytes for v in out.values()) // 1024} KiB raw, {os.path.getsize(path) // 1024} KiB on disk")


# full-size cases: key -> (BASELINE config, filter scale in dx_min units (0 = the config's own), NaN on land?[, options])
# options: level = the vertical level of config 5 (its fields are seeded per level); f32 = field AND grid variables cast to float32
# before the reference sees them (its f32-input path: f32 recurrence, f64 running sum and result)
FULLSIZE_CASES = {
    "cfg2_n11": (2, 10.0, False), "cfg2_n56": (2, 50.0, False), "cfg2_n11_nanland": (2, 10.0, True),
    "cfg3_n63": (3, 0.0, False), "cfg4_n56": (4, 0.0, False), "cfg5_lev0_n44": (5, 0.0, False),
    # round 4: two more levels of config 5 and the f32-state path of configs 3 / 4
    "cfg5_lev24_n44": (5, 0.0, False, {"level": 24}), "cfg5_lev49_n44": (5, 0.0, False, {"level": 49}),
    "cfg3_f32_n63": (3, 0.0, False, {"f32": True}), "cfg4_f32_n56": (4, 0.0, False, {"f32": True}),
}


def make_fullsize(rf, rk, outdir):
    """BASELINE configs 2-5 at full size through the imported reference -> probes + checksums."""
    import time
    from gcm_filters_amd import testing as T

    out = {}
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    if only:   # regenerate some cases, keep the others as they are in the committed file
        with np.load(os.path.join(outdir, "reference_fullsize.npz")) as z:
            out = {k: z[k] for k in z.files}
    for key, (cfg, scale, nanland, *rest) in FULLSIZE_CASES.items():
        if only and key not in only:
            continue
        opt = rest[0] if rest else {}
        wl = T.baseline_workload(cfg, T.BASELINE_SHAPE, scale=scale, levels=[opt.get("level", 0)] if cfg == 5 else None)
        grid, gv, fk = wl["grid"], wl["grid_vars"], wl["fk"]
        fields = [f[0] if f.ndim == 3 else f for f in wl["fields"]]
        if opt.get("f32"):
            gv = {k: v.astype(np.float32) for k, v in gv.items()}
            fields = [f.astype(np.float32) for f in fields]
        if nanland:
            fields = [np.where(gv["wet_mask"] == 0, np.nan, f) for f in fields]
        cls = rk.ALL_KERNELS[rk.GridType[grid]]
        args = [gv[k] for k in cls.required_grid_args()]
        shape = rf.FilterShape[fk["filter_shape"]]
        n = rf._compute_n_steps_default(2, shape, fk["filter_scale"], fk["dx_min"], np.pi)
        spec = rf._compute_filter_spec(fk["filter_scale"], fk["dx_min"], shape, np.pi, 2, n)
        assert key.endswith(f"n{int(n)}") or f"_n{int(n)}_" in key, (key, n)
        t0 = time.time()
        with np.errstate(all="ignore"):
            if len(fields) == 2:
                res = np.stack(rf._create_filter_func_vec(spec, cls)(*fields, *args))
            else:
                res = np.asarray(rf._create_filter_func(spec, cls)(*fields, *args))
        jj, ii = T.probe_points(T.BASELINE_SHAPE)
        out[key + "/probe"] = res[..., jj, ii].copy()
        fin = np.isfinite(res)
        r0 = np.where(fin, res, 0.0)
        out[key + "/sums"] = np.array([r0.sum(), (r0 * r0).sum(), np.abs(r0).max(), float((~fin).sum())])
        out[key + "/meta"] = np.array([n, spec.s_max, spec.dx_min_sq])
        out[key + "/p"] = np.asarray(spec.p)
        print(f"{key}: n_steps {int(n)} dtype {res.dtype} {time.time() - t0:.1f} s", flush=True)
    np.savez_compressed(os.path.join(outdir, "reference_fullsize.npz"), **out)
    print("reference_fullsize.npz:", len(out), "arrays")


def main():
    if not os.path.isdir(REF):
        print("reference not mounted: nothing to do")
        return 0
    sys.path.insert(0, REPO)
    rf, rk = import_reference()
    global HERE
    if "--out" in sys.argv:
        HERE = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(HERE, exist_ok=True)
    if "--fullsize" in sys.argv:
        make_fullsize(rf, rk, HERE)
        return 0
    if "--gridbatched" in sys.argv:
        make_gridbatched(rf, rk, HERE)
        return 0
    if "--coastlines" in sys.argv:
        make_coastlines(rf, rk, HERE)
        return 0
    if "--vector-metrics" in sys.argv:
        make_vector_metrics(rf, rk, HERE)
        return 0

    # 1. the reference's own goldens
    z = {}
    for sub in ("test_data_kernels", "test_data_filter"):
        d = os.path.join(REF, "tests", sub)
        for entry in sorted(os.listdir(d)):
            if entry.endswith(".zarr"):
                z[f"{sub}/{entry[:-5]}"] = read_zarr_array(os.path.join(d, entry))
    np.savez_compressed(os.path.join(HERE, "reference_zarr.npz"), **z)
    print("reference_zarr.npz:", len(z), "arrays")

    # 2. fp64 vectors from the imported reference
    out = {}
    for name in case_names():
        if name == "REGULAR/config1":  # BASELINE config 1: REGULAR 512x512, Gaussian scale 4, n_steps 16
            from gcm_filters_amd import testing as T
            f = T.random_field((512, 512), 100)
            n = 16
            spec = rf._compute_filter_spec(4.0, 1.0, rf.FilterShape.GAUSSIAN, np.pi, 2, n)
            res = rf._create_filter_func(spec, rk.ALL_KERNELS[rk.GridType.REGULAR])(f)
            # 512x512 f64 is 2 MiB: keep a strided probe + checksums instead of the full plane
            out[name + "/probe"] = res[::8, ::8].copy()
            out[name + "/sums"] = np.array([res.sum(), (res * res).sum(), np.abs(res).max()])
            continue
        grid, fields, gv, fk = build_case(name)
        gt = rk.GridType[grid]
        cls = rk.ALL_KERNELS[gt]
        args = [gv[k] for k in cls.required_grid_args()]
        if fk is None:
            lap = cls(**gv)
            res = lap(*fields)
        else:
            shape = rf.FilterShape[fk["filter_shape"]]
            n = rf._compute_n_steps_default(2, shape, fk["filter_scale"], fk["dx_min"], np.pi)
            spec = rf._compute_filter_spec(fk["filter_scale"], fk["dx_min"], shape, np.pi, 2, n)
            if len(fields) == 2:
                res = rf._create_filter_func_vec(spec, cls)(*fields, *args)
            else:
                res = rf._create_filter_func(spec, cls)(*fields, *args)
        res = np.stack(res) if isinstance(res, tuple) else np.asarray(res)
        out[name] = res
    np.savez_compressed(os.path.join(HERE, "reference_generated.npz"), **out)
    print("reference_generated.npz:", len(out), "arrays,",
          sum(v.nbytes for v in out.values()) // 1024, "KiB raw")

    # 3. polynomial table
    sp = {}
    for row in SPEC_TABLE:
        shape, scale, dx_min, tw, ndim, n = row
        fs = rf.FilterShape[shape]
        nd = int(rf._compute_n_steps_default(ndim, fs, scale, dx_min, tw)) if ndim <= 2 else n
        nn = n if n >= 3 else nd
        spec = rf._compute_filter_spec(scale, dx_min, fs, tw, ndim, nn)
        key = f"{shape}|{scale!r}|{dx_min!r}|{tw!r}|{ndim}|{n}"
        sp[key + "|p"] = np.asarray(spec.p)
        sp[key + "|meta"] = np.array([nd, spec.n_steps, spec.s_max, spec.dx_min_sq], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "reference_spec.npz"), **sp)
    print("reference_spec.npz:", len(sp) // 2, "rows")
    return 0


if __name__ == "__main__":
    sys.exit(main())
