"""One large host field: the row-block pipeline (gcm_filters_amd/host_blocks.py) must return exactly what the one-plan
path returns (same kernels on row ranges of slab plans), for every scalar kind incl. the tripole fold, NaN on land, f32."""
import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, host_blocks, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
from oracle import gcmf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture
def eager_blocks(monkeypatch):
    monkeypatch.setattr(host_blocks, "MIN_CELLS", 1)
    monkeypatch.setattr(host_blocks, "BUILD_AFTER_CALLS", 0)
    clear_plan_cache()
    yield
    clear_plan_cache()


@pytest.mark.parametrize("grid,shape,dt,n_steps,nblocks", [
    ("IRREGULAR_WITH_LAND", (520, 384), "f8", 19, 3), ("REGULAR_WITH_LAND", (400, 512), "f8", 24, 2),
    ("REGULAR", (384, 260), "f8", 16, 3), ("REGULAR_AREA_WEIGHTED", (300, 256), "f8", 11, 2),
    ("REGULAR_WITH_LAND_AREA_WEIGHTED", (512, 256), "f4", 17, 4), ("TRIPOLAR_POP_WITH_LAND", (420, 256), "f8", 18, 3),
    ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", (390, 264), "f8", 9, 2), ("MOM5T", (300, 256), "f8", 13, 2),
    ("IRREGULAR_WITH_LAND", (512, 512), "f4", 21, 4),
])
def test_row_blocks_equal_one_plan(grid, shape, dt, n_steps, nblocks, eager_blocks, monkeypatch):
    f, gv = T.scalar_case(grid, shape)
    land = gv["wet_mask"] == 0 if "wet_mask" in gv else np.zeros(shape, bool)
    f = np.where(land, np.nan, f).astype(dt)
    gv = {k: v.astype(dt) for k, v in gv.items()}
    dx = T.grid_dx_min(grid, gv) if O.DIMENSIONAL[grid] else 1.0
    flt = Filter(filter_scale=3.0 * dx, dx_min=dx, n_steps=n_steps, filter_shape=FilterShape.TAPER,
                 grid_type=GridType[grid], grid_vars=gv)
    monkeypatch.setenv("GCMF_HOST_BLOCKS", "0")
    want = flt.apply(f)
    monkeypatch.setenv("GCMF_HOST_BLOCKS", str(nblocks))
    clear_plan_cache()
    got = flt.apply(f)
    got2 = flt.apply(f[None])[0]     # a leading dimension of one takes the same route
    assert got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want, equal_nan=True), float(np.nanmax(np.abs(got - want)))
    assert np.array_equal(got2, want, equal_nan=True)
    with np.errstate(all="ignore"):
        ref = O.filter_func(O.make_spec(3.0 * dx, dx, "TAPER", n_steps=n_steps), grid, f, gv)
    err = np.nanmax(np.abs(got - ref)) / np.nanmax(np.abs(ref))
    assert err <= (1e-4 if dt == "f4" else 1e-11)


def test_row_blocks_are_built_lazily_and_really_used(monkeypatch):
    """The pipeline costs K extra plans: it appears with the third single-field host call on a plan, and from then on the
    blocked launches run on the block plans (the parent plan sees no launch)."""
    from gcm_filters_amd import _lib
    monkeypatch.setattr(host_blocks, "MIN_CELLS", 1)
    monkeypatch.delenv("GCMF_HOST_BLOCKS", raising=False)
    clear_plan_cache()
    shape = (600, 512)
    grid = "IRREGULAR_WITH_LAND"
    f, gv = T.scalar_case(grid, shape)
    dx = T.grid_dx_min(grid, gv)
    flt = Filter(filter_scale=4.0 * dx, dx_min=dx, filter_shape=FilterShape.GAUSSIAN, grid_type=GridType[grid], grid_vars=gv)
    plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, shape)
    outs = []
    for call in range(4):
        plan.last_kernel()
        outs.append(flt.apply(f))
        ran_on_parent = plan.last_kernel() != ""
        assert ran_on_parent == (call < host_blocks.BUILD_AFTER_CALLS), call
    pipes = plan.__dict__["_host_blocks"]["pipes"]
    assert list(pipes) == [flt.n_steps] and pipes[flt.n_steps].nblocks == host_blocks.choose_blocks(shape[0], flt.n_steps) >= 2
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    # a batch, a device tensor and a vector field never take this route
    import torch
    assert np.array_equal(flt.apply(np.stack([f, f]))[1], outs[0])
    assert np.array_equal(flt.apply(torch.from_numpy(f).cuda()).cpu().numpy(), outs[0])
    clear_plan_cache()
    assert "_host_blocks" not in plan.__dict__     # closing the plan closed the block plans


# ------------------------------------------------------------------------------------------------------------------------------
# row blocks on coastlines: the block boundaries (and, on the tripolar kinds, the seam the top block owns) on land, straits and gaps
# ------------------------------------------------------------------------------------------------------------------------------
def _coast_block_cases():
    out = []
    for grid, dt in (("IRREGULAR_WITH_LAND", "f8"), ("REGULAR_WITH_LAND_AREA_WEIGHTED", "f8"), ("REGULAR_WITH_LAND_AREA_WEIGHTED", "f4"),
                     ("TRIPOLAR_POP_WITH_LAND", "f8"), ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "f8")):
        for coast in ("on_the_cuts", "channels", "speckle") + (("fold",) if grid.startswith("TRIPOLAR") else ()):
            for nblocks in (2, 3):
                for n_steps in (11, 19):
                    out.append((grid, dt, coast, nblocks, n_steps))
    return out


@pytest.mark.parametrize("grid,dt,coast,nblocks,n_steps", _coast_block_cases())
def test_row_blocks_on_coastlines(grid, dt, coast, nblocks, n_steps):
    """RowBlockPipeline built directly (choose_blocks wants 128 rows per block) on 96 rows: two and three blocks whose boundaries fall on
    the rectangles of `on_the_cuts` (cuts = the block height), between the straits of `channels`, in a speckle, and -- tripolar kinds --
    with land on the seam of the top block (`fold`).  NaN on land, and a NaN in a wet cell on the last row of block 0 and on the first row
    of the top block: rows every neighbouring block holds as ghost rows.  The pipeline must give the bits of Plan.apply on the parent
    plan, the oracle's NaN pattern, and an error within test_gpu_dispatch_edges.errors()'s bound."""
    from types import SimpleNamespace
    from gcm_filters_amd import _lib
    from test_gpu_dispatch_edges import errors

    shape = (96, 256) if dt == "f4" else (96, 128)
    ny, nx = shape
    height = ny // nblocks
    tripolar = grid.startswith("TRIPOLAR")
    gv = T.scalar_grid_vars(grid, shape)
    gv["wet_mask"] = wet = T.coastline(coast, shape, seed=55, tripolar=tripolar, cuts=(height,))
    f = T.treat_land(T.random_field(shape, 100), wet, "nan")
    for j in (height - 1, ny - height):
        ii = np.nonzero(wet[j])[0]
        assert ii.size, (coast, j)
        f[j, ii[(5 * j + 1) % ii.size]] = np.nan
    gv = {k: v.astype(dt) for k, v in gv.items()}
    f = np.ascontiguousarray(f.astype(dt))
    dx = T.grid_dx_min(grid, gv) if O.DIMENSIONAL[grid] else 1.0
    flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=n_steps, filter_shape=FilterShape.GAUSSIAN, grid_type=GridType[grid], grid_vars=gv)
    fs = flt.filter_spec
    p = np.asarray(fs.p, dtype=np.float64)
    c = 2 / fs.s_max if O.DIMENSIONAL[grid] else 2 / (fs.s_max * fs.dx_min_sq)
    clear_plan_cache()
    lap = ALL_KERNELS[GridType[grid]](**gv)
    plan = lap._plan(_lib.dtype_code(dt), shape)
    pipe = None
    try:
        want = np.empty(shape)
        plan.apply(p, c, [f.ctypes.data], [want.ctypes.data], 1, device_ptrs=False)
        parent_kernel = plan.last_kernel()
        pipe = host_blocks.RowBlockPipeline(GridType[grid].value, _lib.dtype_code(dt), ny, nx, [np.asarray(a) for a in lap._planes], plan.device,
                                            n_steps, nblocks, skip_kappa_one=lap._skip_kappa_one, cut=plan.clenshaw_cut(n_steps))
        assert pipe.ok and pipe.nblocks == nblocks and [b.ro for b in pipe.blocks] == [height] * nblocks
        got = np.empty(shape)
        pipe.apply(p, c, f, got, False)
        block_kernel = pipe.blocks[-1].plan.last_kernel()
        assert block_kernel and plan.last_kernel() == ""            # the launches ran on the block plans
    finally:
        if pipe is not None:
            pipe.close()
        clear_plan_cache()
    spec = O.FilterSpec(fs.n_steps, fs.s_max, p, fs.dx_min_sq)
    with np.errstate(all="ignore"):
        truth = O.filter_func(spec, grid, f.astype("f8"), {k: v.astype("f8") for k, v in gv.items()})
        ref32 = O.filter_func(spec, grid, f, gv) if dt == "f4" else None
    assert np.isfinite(truth).any()
    assert np.array_equal(np.isnan(got), np.isnan(truth)), (grid, coast, "NaN pattern differs from the oracle's")
    r = dict(got=(got,), truth=(truth,), ref32=(ref32,), lap=(truth,), ltruth=(truth,), lref32=(ref32,))
    e, bound, _, _ = errors(SimpleNamespace(dt=dt, scheme="forward"), r)
    print(f"\n{grid} {dt} {coast} {nblocks} blocks n {n_steps}: parent {parent_kernel} blocks {block_kernel} error {e:.3e} (bound {bound:.3e})")
    assert e <= bound, (grid, coast, e, bound)
    assert np.array_equal(got, want, equal_nan=True), (grid, coast, nblocks, n_steps, float(np.nanmax(np.abs(got - want))))
