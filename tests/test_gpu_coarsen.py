"""Filter and coarsen in one call on the GPU: ``Filter.apply_coarsened``, ``Plan.apply_coarsen`` and the C ABI (``gcmf_apply_coarsen``,
``gcmf_coarsen_weights``).

The truth of a coarse plane is the numpy block mean, by the rule (``gcm_filters_amd.coarsen.block_means``; tests/test_coarsen_rule.py
checks the rule itself), of the oracle's ``filter_func`` output with the grid's own weights.  Gates: the project's rel_err <= 1e-11
for f64 with an identical NaN pattern -- a block mean is a convex combination of fine values, so it does not amplify the fine gate --
and, against the block mean of ``apply``'s own result, the rounding bound of the rule,
|got - want| <= 4 fy fx 2^-53 sum(w |F|) / sum(w) per coarse cell; wsum to 2 fy fx 2^-53 relative.  Shapes: (96, 160) -- two column
windows that wrap -- and (200, 520) -- five windows, several strips, and blocks wider than one workgroup's columns; (64, 102): nx no
multiple of 4."""
import functools
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, coarsen, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, CallOptions
from oracle import gcmf_oracle as O
from test_gpu_nan_mask import gappy_stack
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GATE = 1e-11
N_STEPS = 24
SMALL, BLOCKED, ODD = (96, 160), (200, 520), (64, 102)
KINDS = ["REGULAR", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5T", "TRIPOLAR_POP_WITH_LAND"]
GEOMETRIES = [(SMALL, (2, 2)), (SMALL, (3, 5)), (SMALL, (8, 10)), (SMALL, (1, 4)), (SMALL, SMALL), (BLOCKED, (5, 8)), (BLOCKED, (25, 13))]
POISON = -7.25e300


def geometry_id(g):
    return "%dx%d-by-%dx%d" % (g[0] + g[1])


def grid_vars(kind, shape):
    gv = dict(T.scalar_grid_vars(kind, shape))
    if kind == "IRREGULAR_WITH_LAND":
        gv["kappa_w"], gv["kappa_s"] = T.smooth_kappa(shape, 11), T.smooth_kappa(shape, 12)
    return gv


def make_filter(kind, gv, n_steps=N_STEPS, **kw):
    dx = T.grid_dx_min(kind, gv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # ("n_steps below the default": the polynomial is chosen for its launch cut)
        return Filter(filter_scale=6.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=n_steps, grid_type=GridType[kind], grid_vars=gv,
                      **kw)


def fields(shape, n, seed=300):
    return np.stack([T.random_field(shape, seed + b) for b in range(n)])


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """(grid variables, 17 fields, the oracle's filter of them, the grid's own weights): computed once, shared, left unchanged."""
    gv = grid_vars(kind, shape)
    fs = make_filter(kind, gv).filter_spec
    spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
    f = fields(shape, 17)
    with np.errstate(all="ignore"):
        fine = np.stack([O.filter_func(spec, kind, a, gv) for a in f])
    fine.flags.writeable = False
    return gv, f, fine, coarsen.default_weights(GridType[kind], gv)


def bound_of(fine, w, factor):
    """4 fy fx u sum(w |F|) / sum(w) per coarse cell (0 where no cell counts)."""
    fy, fx = factor
    mag, wsum = coarsen.block_means(np.abs(fine), w, factor)
    return 4 * fy * fx * U * np.where(wsum > 0, mag, 0.0)


def within_bound(got, fine, w, factor, what, scale=1.0):
    want, _ = coarsen.block_means(fine, w, factor)
    got = np.asarray(got)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    ok = ~np.isnan(want)
    err, lim = np.abs(got - want)[ok], scale * bound_of(fine, w, factor)[ok]
    worst = float((err / np.where(lim > 0, lim, 1.0)).max()) if err.size else 0.0
    print(f"{what}: worst |got - want| / bound {worst:.3f}")
    assert np.all(err <= lim), (what, worst)


def wsum_within_bound(got, fine, w, factor, what):
    fy, fx = factor
    _, want = coarsen.block_means(fine, w, factor)
    assert np.array_equal(np.asarray(got) == 0, want == 0), (what, "wsum == 0 pattern")
    assert np.all(np.abs(np.asarray(got) - want) <= 2 * fy * fx * U * np.abs(want)), what


def same_bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a)), np.ascontiguousarray(np.asarray(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cpu(t):
    return t.cpu().numpy()


# ---- 1. parity with the oracle, with apply's own result, and between the routes ------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 17])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=geometry_id)
@pytest.mark.parametrize("kind", KINDS)
def test_parity(kind, geometry, nb):
    import torch
    shape, factor = geometry
    fy, fx = factor
    gv, f, fine, w = case(kind, shape)
    flt = make_filter(kind, gv)
    what = (kind, shape, factor, nb)
    got, gw = flt.apply_coarsened(f[:nb], factor, return_weights=True)
    dev, dw = flt.apply_coarsened(torch.from_numpy(f[:nb]).cuda(), factor, return_weights=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (nb, shape[0] // fy, shape[1] // fx)
    assert dev.is_cuda and dev.dtype == torch.float64 and dw.is_cuda and tuple(dev.shape) == got.shape
    if w is not None:      # the fixture's mask: its south-west quadrant and its southernmost row are land
        cells = coarsen.block_means(np.ones(shape), (w > 0).astype(np.float64), factor)[1]
        if factor != shape:
            assert np.isnan(got).any() and (gw == 0).any(), (what, "no block that is all land")
        if factor != (1, 4):
            assert ((cells > 0) & (cells < fy * fx)).any(), (what, "no block that is partly land")
    # against the oracle
    want, want_w = coarsen.block_means(fine[:nb], w, factor)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    err = rel_err(got, want)
    print(f"{what}: rel_err {err:.3e}")
    assert err <= GATE, (what, err)
    # against the block mean of apply's own result, and wsum against numpy
    own = cpu(flt.apply(torch.from_numpy(f[:nb]).cuda()))
    within_bound(got, own, w, factor, what)
    wsum_within_bound(gw, own, w, factor, what)
    # numpy in and a device tensor in: the same bits
    assert same_bits(got, cpu(dev)) and same_bits(gw, cpu(dw)), (what, "numpy in and a device tensor in differ")
    # without return_weights: the coarse planes alone, the same bits
    assert same_bits(flt.apply_coarsened(f[:nb], factor), got), what


@pytest.mark.parametrize("factor", [(2, 3), (4, 17)], ids=["2x3", "4x17"])
@pytest.mark.parametrize("kind", ["REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND"])
def test_nx_no_multiple_of_four(kind, factor):
    import torch
    gv, f, fine, w = case(kind, ODD)
    flt = make_filter(kind, gv)
    for nb in (1, 3):
        what = (kind, ODD, factor, nb)
        got, gw = flt.apply_coarsened(f[:nb], factor, return_weights=True)
        want, _ = coarsen.block_means(fine[:nb], w, factor)
        assert rel_err(got, want) <= GATE, what
        own = cpu(flt.apply(torch.from_numpy(f[:nb]).cuda()))
        within_bound(got, own, w, factor, what)
        wsum_within_bound(gw, own, w, factor, what)
        assert same_bits(got, cpu(flt.apply_coarsened(torch.from_numpy(f[:nb]).cuda(), factor))), what


@pytest.mark.parametrize("shape,factor", [((48, 75), (4, 5)), ((48, 75), (48, 75)), (BLOCKED, (1, 520)), (BLOCKED, (200, 520)), ((30, 777), (3, 777))],
                         ids=["odd-nx", "odd-nx-one-block", "row-blocks", "one-block", "odd-wide-blocks"])
def test_element_loads_and_blocks_wider_than_a_workgroup(shape, factor):
    """nx odd: no 16-byte pairs; fx > 511 (pairs) or > 256 (elements): one workgroup walks a block in chunks."""
    import torch
    kind = "REGULAR_WITH_LAND"
    gv = grid_vars(kind, shape)
    flt = make_filter(kind, gv)
    f = torch.from_numpy(fields(shape, 2, 500)).cuda()
    got, gw = flt.apply_coarsened(f, factor, return_weights=True)
    own = cpu(flt.apply(f))
    within_bound(cpu(got), own, gv["wet_mask"], factor, (shape, factor))
    wsum_within_bound(cpu(gw), own, gv["wet_mask"], factor, (shape, factor))


# ---- 2. the same bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "TRIPOLAR_POP_WITH_LAND"])
def test_an_entry_alone_and_inside_a_batch_and_twice(kind):
    import torch
    gv, f, _, _ = case(kind, SMALL)
    flt = make_filter(kind, gv)
    x = torch.from_numpy(f).cuda()
    for factor in ((3, 5), SMALL):
        batch, bw = flt.apply_coarsened(x, factor, return_weights=True)
        again, aw = flt.apply_coarsened(x, factor, return_weights=True)
        assert same_bits(cpu(batch), cpu(again)) and same_bits(cpu(bw), cpu(aw)), (kind, factor, "two consecutive calls differ")
        for k in (0, 8, 16):
            alone, lw = flt.apply_coarsened(x[k:k + 1], factor, return_weights=True)
            assert same_bits(cpu(alone[0]), cpu(batch[k])) and same_bits(cpu(lw[0]), cpu(bw[k])), (kind, factor, k, "alone and in a batch of 17 differ")


def raw_plan(kind, gv, shape, **kw):
    """A plan of the test's own (not the cache's: the tests below set weights and options on it)."""
    planes = [np.ascontiguousarray(gv[k], dtype="f8") for k in ALL_KERNELS[GridType[kind]].required_grid_args()]
    return _lib.Plan(GridType[kind].value, _lib.F64, shape[0], shape[1], planes, **kw)


def poly(kind, gv):
    flt = make_filter(kind, gv)
    return np.asarray(flt.filter_spec.p, dtype=np.float64), CallOptions(spec=flt.filter_spec).shift(ALL_KERNELS[GridType[kind]].is_dimensional)


def poisoned_view(n, off):
    """n float64 values `off` elements into a poisoned device buffer with a margin on either side (torch aligns the buffer itself)."""
    import torch
    buf = torch.full((n + 64,), POISON, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[32 + off:32 + off + n]


@pytest.mark.parametrize("shape,factor", [(SMALL, (3, 5)), (BLOCKED, (25, 520))], ids=["96x160-by-3x5", "200x520-by-25x520"])
def test_views_one_element_off_the_16_byte_boundary(shape, factor):
    import torch
    kind = "IRREGULAR_WITH_LAND"
    gv, f, _, w = case(kind, shape)
    p, c = poly(kind, gv)
    plan = raw_plan(kind, gv, shape)
    plan.set_coarsen_weights(w, 1)
    stream = torch.cuda.current_stream().cuda_stream
    nb, ncell, nco = 3, shape[0] * shape[1], (shape[0] // factor[0]) * (shape[1] // factor[1])
    results = []
    for off_in, off_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
        _, fin = poisoned_view(nb * ncell, off_in)
        fin.copy_(torch.from_numpy(f[:nb].reshape(-1)))
        bufs, views = zip(*(poisoned_view(nb * nco, off_out) for _ in range(2)))
        assert fin.data_ptr() % 16 == 8 * off_in and views[0].data_ptr() % 16 == 8 * off_out
        plan.apply_coarsen(p, c, [fin.data_ptr()], [views[0].data_ptr()], nb, *factor, wsums=[views[1].data_ptr()], device_ptrs=True, stream=stream)
        torch.cuda.synchronize()
        for buf in bufs:
            outside = torch.cat([buf[:32 + off_out], buf[32 + off_out + nb * nco:]])
            assert bool((outside == POISON).all()), ("written outside the output", off_in, off_out)
        assert not bool((views[0] == POISON).any()) and not bool((views[1] == POISON).any())
        results.append((cpu(views[0]), cpu(views[1])))
    for r in results[1:]:
        assert same_bits(r[0], results[0][0]) and same_bits(r[1], results[0][1]), "the bits depend on the alignment of the planes"
    plan.close()


def test_a_batch_cut_into_runs_and_weight_levels_that_follow_the_entries():
    import torch
    kind, shape, factor = "IRREGULAR_WITH_LAND", SMALL, (8, 10)
    gv, f, _, w = case(kind, shape)
    p, c = poly(kind, gv)
    plan = raw_plan(kind, gv, shape)
    w2 = np.stack([w, w * T.random_field(shape, 77)])      # two weight levels on an ordinary plan: entry b takes level b % 2
    plan.set_coarsen_weights(w2, 2)
    x = torch.from_numpy(f[:5]).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def call(ins, n):
        out = torch.full((2, n, shape[0] // 8, shape[1] // 10), POISON, dtype=torch.float64, device="cuda")
        plan.apply_coarsen(p, c, [ins.data_ptr()], [out[0].data_ptr()], n, *factor, wsums=[out[1].data_ptr()], device_ptrs=True, stream=stream)
        torch.cuda.synchronize()
        return cpu(out)

    whole = call(x, 5)
    plan.set_option("coarsen_scratch_mb", 0)      # at least one entry per run: five runs
    runs = call(x, 5)
    assert same_bits(whole, runs), "the bits depend on how the batch is cut into runs"
    host = np.full((2, 5, shape[0] // 8, shape[1] // 10), POISON)
    plan.apply_coarsen(p, c, [f[:5].ctypes.data], [host[0].ctypes.data], 5, *factor, wsums=[host[1].ctypes.data], device_ptrs=False)
    assert same_bits(whole, host), "host pointers and device pointers differ"
    plan.set_option("coarsen_scratch_mb", 4096)
    fine = torch.empty_like(x)
    plan.apply(p, c, [x.data_ptr()], [fine.data_ptr()], 5, device_ptrs=True, stream=stream)
    fine = cpu(fine)
    for b in range(5):
        within_bound(whole[0, b], fine[b], w2[b % 2], factor, ("level of entry", b))
        wsum_within_bound(whole[1, b], fine[b], w2[b % 2], factor, ("level of entry", b))
    assert not same_bits(whole[1, 1], whole[1, 0])
    plan.close()


# ---- 3. gaps, levels, explicit weights ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nan_mask", [("IRREGULAR_WITH_LAND", "auto"), ("REGULAR_WITH_LAND_AREA_WEIGHTED", True)])
def test_gaps_drop_out_of_the_means(kind, nan_mask):
    import torch
    shape, factor = SMALL, (8, 10)
    gv, _, _, w = case(kind, shape)
    flt = make_filter(kind, gv, nan_mask=nan_mask)
    f = gappy_stack(shape, 3, 5)
    f[:, 56:64, 100:110] = np.nan      # a block of wet cells that is all gap
    assert (w[56:64, 100:110] > 0).all()
    x = torch.from_numpy(f).cuda()
    got, gw = flt.apply_coarsened(x, factor, return_weights=True)
    fine = cpu(flt.apply(x))
    assert np.array_equal(np.isnan(fine) & (w > 0), np.isnan(f) & (w > 0))      # the gaps are NaN in the fine result
    got, gw = cpu(got), cpu(gw)
    assert np.isnan(got[:, 7, 10]).all() and (gw[:, 7, 10] == 0).all()
    within_bound(got, fine, w, factor, (kind, "gaps"))
    # ... which is the mean over the wet cells that are not gaps
    present = np.where(np.isnan(f), 0.0, 1.0) * w
    within_bound(got, np.where(np.isnan(f), 0.0, fine), present, factor, (kind, "gaps, by hand"))
    wsum_within_bound(gw, fine, w, factor, (kind, "gaps"))
    assert same_bits(got, flt.apply_coarsened(f, factor)), (kind, "numpy in and a device tensor in differ")


def level_masks(shape, nlev=3):
    m = np.stack([T.land_mask(shape)] * nlev)
    for k in range(nlev):      # every level loses other cells: a strip that grows with depth and a patch of its own
        m[k, 50:50 + 6 * (k + 1), 90:150] = 0
        m[k, 70 + 8 * k:76 + 8 * k, 20 * k:20 * k + 30] = 0
    return m


def test_every_level_is_weighted_with_its_own_mask(monkeypatch):
    import torch
    kind, shape, factor = "IRREGULAR_WITH_LAND", SMALL, (8, 10)
    gv = grid_vars(kind, shape)
    gv["wet_mask"] = level_masks(shape)
    f = fields(shape, 6, 900).reshape(2, 3, *shape)
    w = coarsen.default_weights(GridType[kind], gv)
    assert w.shape == (3,) + shape
    results = {}
    for stack in ("1", "0"):
        monkeypatch.setenv("GCMF_STACK_LEVELS", stack)
        flt = make_filter(kind, {k: v.copy() for k, v in gv.items()})
        x = torch.from_numpy(f).cuda()
        got, gw = flt.apply_coarsened(x, factor, return_weights=True)
        fine = cpu(flt.apply(x))
        within_bound(cpu(got), fine, w, factor, ("levels, GCMF_STACK_LEVELS=" + stack))
        wsum_within_bound(cpu(gw), fine, w, factor, ("levels, GCMF_STACK_LEVELS=" + stack))
        assert same_bits(cpu(got), flt.apply_coarsened(f, factor)), "numpy in and a device tensor in differ"
        results[stack] = (cpu(got), fine)
    # the two routes: the same to the bound
    a, b = results["1"][0], results["0"][0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    lim = bound_of(results["1"][1], w, factor)
    ok = ~np.isnan(a)
    print("levels: stacked against per-level, worst |a - b| / bound", float((np.abs(a - b)[ok] / lim[ok]).max()))
    assert np.all(np.abs(a - b)[ok] <= lim[ok])
    # level 0's weights on level 2 would miss by more than 100 bounds: the mask is one that tells
    fine2 = results["1"][1][:, 2]
    wrong, _ = coarsen.block_means(fine2, w[0], factor)
    right, _ = coarsen.block_means(fine2, w[2], factor)
    both = ~np.isnan(wrong) & ~np.isnan(right)
    assert (np.abs(wrong - right)[both] > 100 * bound_of(fine2, w[2], factor)[both]).any()
    assert not np.array_equal(np.isnan(wrong), np.isnan(right))


def test_explicit_weights_replace_the_grids_own():
    import torch
    kind, shape, factor = "IRREGULAR_WITH_LAND", SMALL, (8, 10)
    gv, f, _, w = case(kind, shape)
    flt = make_filter(kind, gv)
    x = torch.from_numpy(f[:3]).cuda()
    fine = cpu(flt.apply(x))
    default = cpu(flt.apply_coarsened(x, factor))
    ones = np.ones(shape)
    got = cpu(flt.apply_coarsened(x, factor, weights=ones))
    within_bound(got, fine, ones, factor, "all ones")      # land counts now: no NaN block, other values
    assert not np.isnan(got).any() and np.isnan(default).any() and not np.array_equal(got[~np.isnan(default)], default[~np.isnan(default)])
    holes = w * (T.random_field(shape, 41) < 0.6)
    got, gw = flt.apply_coarsened(x, factor, weights=holes, return_weights=True)
    within_bound(cpu(got), fine, holes, factor, "weights with zeros")
    wsum_within_bound(cpu(gw), fine, holes, factor, "weights with zeros")
    as_tensor = cpu(flt.apply_coarsened(x, factor, weights=torch.from_numpy(holes).cuda()))
    assert same_bits(as_tensor, cpu(got))
    assert same_bits(cpu(flt.apply_coarsened(x, factor)), default), "the grid's own weights did not come back"
    with pytest.raises(ValueError, match="spatial shape|weights have shape"):
        flt.apply_coarsened(x, factor, weights=np.ones((8, 10)))


@pytest.mark.parametrize("kind,dt,evaluation", [("REGULAR_WITH_LAND", "f4", "auto"), ("IRREGULAR_WITH_LAND", "f4", "backward"),
                                                ("IRREGULAR_WITH_LAND", "f8", "reference"), ("MOM5T", "f4", "reference")])
def test_float32_plans_and_the_other_evaluations_carry_over(kind, dt, evaluation):
    """A float32 field on float32 grid variables runs a float32 plan, whose fine result is float64 (as apply's): so are the coarse
    planes; `evaluation` selects the schedule exactly as for apply."""
    import torch
    shape, factor = SMALL, (3, 5)
    gv = {k: v.astype(dt) for k, v in grid_vars(kind, shape).items()}
    flt = make_filter(kind, gv, evaluation=evaluation)
    f = fields(shape, 3, 600).astype(dt)
    x = torch.from_numpy(f).cuda()
    fine = flt.apply(x)
    assert fine.dtype == torch.float64
    w = coarsen.default_weights(GridType[kind], gv)
    got, gw = flt.apply_coarsened(x, factor, return_weights=True)
    assert got.dtype == torch.float64 and gw.dtype == torch.float64
    within_bound(cpu(got), cpu(fine), w, factor, (kind, dt, evaluation))
    wsum_within_bound(cpu(gw), cpu(fine), w, factor, (kind, dt, evaluation))
    host = flt.apply_coarsened(f, factor)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and same_bits(host, cpu(got))
    tensor = flt.apply_coarsened(torch.from_numpy(f), factor)      # a host tensor in, a host tensor out
    assert isinstance(tensor, torch.Tensor) and not tensor.is_cuda and same_bits(tensor.numpy(), host)


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------------
def _status(fn, *a, **k):
    try:
        fn(*a, **k)
    except _lib.GcmfError as e:
        return e.status, e.message
    return _lib.OK, ""


def test_c_abi_refusals_write_nothing():
    import torch
    kind, shape = "IRREGULAR_WITH_LAND", SMALL
    ny, nx = shape
    gv, f, _, w = case(kind, shape)
    p, c = poly(kind, gv)
    plan = raw_plan(kind, gv, shape)
    x = torch.from_numpy(f[:2]).cuda()
    out = torch.full((2, 2, ny // 8, nx // 10), POISON, dtype=torch.float64, device="cuda")
    src, dst, ws = x.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def refused(pl, status, why, ins, outs, n, fy, fx, **k):
        st, msg = _status(pl.apply_coarsen, p, c, ins, outs, n, fy, fx, device_ptrs=True, stream=stream, **k)
        assert st == status and "gcmf_apply_coarsen" in msg and why in msg, (why, st, msg)

    bad, no = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    refused(plan, bad, "`fy`", [src], [dst], 2, 0, 10)
    refused(plan, bad, "`fx`", [src], [dst], 2, 8, -1)
    refused(plan, bad, "`fy` = 7 must be positive and divide ny = 96", [src], [dst], 2, 7, 10)
    refused(plan, bad, "`fx` = 7 must be positive and divide nx = 160", [src], [dst], 2, 8, 7)
    refused(plan, bad, "`in`", [None], [dst], 2, 8, 10)
    refused(plan, bad, "`out`", [src], [None], 2, 8, 10)
    refused(plan, bad, "`wsum`", [src], [dst], 2, 8, 10, wsums=[None])
    refused(plan, bad, "`nbatch`", [src], [dst], -1, 8, 10)
    refused(plan, bad, "`out` must not overlap `in`", [src], [src + 8 * ny * nx], 2, 8, 10)
    refused(plan, bad, "`wsum` must not overlap `in`", [src], [dst], 2, 8, 10, wsums=[src + 16])
    refused(plan, bad, "`wsum` must not overlap `out`", [src], [dst], 2, 8, 10, wsums=[dst + 8])
    refused(plan, no, "GCMF_OUT_F32", [src], [dst], 2, 8, 10, flags=_lib.OUT_F32)
    slab = raw_plan(kind, gv, shape, row_begin=0, row_end=ny // 2, halo=9)
    refused(slab, no, "row slab", [src], [dst], 2, 8, 10)
    slab.close()
    ring = raw_plan(kind, gv, shape, self_ring=True, halo=9)
    refused(ring, no, "GCMF_PLAN_SELF_RING", [src], [dst], 2, 8, 10)
    ring.close()
    vg = T.vector_grid_vars("VECTOR_C_GRID", shape)
    vec = raw_plan("VECTOR_C_GRID", vg, shape)
    refused(vec, no, "ncomp == 2", [src, src], [dst, dst], 2, 8, 10)
    vec.close()
    st, msg = _status(plan.set_coarsen_weights, w, 0)
    assert st == bad and "gcmf_coarsen_weights" in msg and "`nlev`" in msg, (st, msg)
    # nbatch = 0 is fine and writes nothing
    plan.apply_coarsen(p, c, [src], [dst], 0, 8, 10, wsums=[ws], device_ptrs=True, stream=stream)
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused call wrote to `out`"
    plan.close()


def test_c_abi_weights_wsum_and_the_launch_count():
    import torch
    kind, shape, factor = "IRREGULAR_WITH_LAND", SMALL, (8, 10)
    ny, nx = shape
    gv, f, _, w = case(kind, shape)
    p, c = poly(kind, gv)
    plan = raw_plan(kind, gv, shape)
    x = torch.from_numpy(f[:3]).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    fine_t = torch.empty_like(x)
    plan.set_timing(True)
    plan.last_kernel()
    plan.apply(p, c, [x.data_ptr()], [fine_t.data_ptr()], 3, device_ptrs=True, stream=stream)
    torch.cuda.synchronize()
    _, launches = plan.last_timing()
    marching, path = plan.last_kernel(), plan.last_path()
    fine = cpu(fine_t)

    def call(wsum=True):
        out = torch.full((2, 3, ny // 8, nx // 10), POISON, dtype=torch.float64, device="cuda")
        plan.apply_coarsen(p, c, [x.data_ptr()], [out[0].data_ptr()], 3, *factor, wsums=[out[1].data_ptr()] if wsum else None, device_ptrs=True,
                           stream=stream)
        torch.cuda.synchronize()
        return cpu(out)

    # a new plan: every weight is 1
    ones = call()
    within_bound(ones[0], fine, None, factor, "no weights set")
    assert np.array_equal(ones[1], np.full_like(ones[1], 80.0))
    # the launch count is the schedule's and one more; the kernel named is still the marching one, the path the same
    _, n = plan.last_timing()
    assert n == launches + 1, (n, launches)
    assert plan.last_kernel() == marching and marching.startswith("gcmf::k_") and "k_prepare" not in marching
    assert plan.last_path() == path
    # wsum = NULL: the same coarse planes, nothing else written
    lone = call(wsum=False)
    assert same_bits(lone[0], ones[0]) and (lone[1] == POISON).all()
    # host weights, replaced by device weights, dropped again
    plan.set_coarsen_weights(w, 1)
    own = call()
    within_bound(own[0], fine, w, factor, "host weights")
    wsum_within_bound(own[1], fine, w, factor, "host weights")
    other = w * T.random_field(shape, 78)
    wt = torch.from_numpy(other).cuda()
    torch.cuda.synchronize()
    plan.set_coarsen_weights(wt.data_ptr(), 1, device_ptrs=True)
    del wt      # (copied: the plan owns its planes)
    repl = call()
    within_bound(repl[0], fine, other, factor, "device weights")
    plan.set_coarsen_weights(other, 1)
    assert same_bits(call(), repl), "host and device weight planes differ"
    plan.set_coarsen_weights(None)
    assert same_bits(call(), ones), "dropping the weights did not bring weight 1 back"
    plan.close()


# ---- 5. the path is apply's -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("IRREGULAR_WITH_LAND", SMALL), ("IRREGULAR_WITH_LAND", BLOCKED), ("TRIPOLAR_POP_WITH_LAND", BLOCKED)],
                         ids=["irregular-96x160", "irregular-200x520", "pop-200x520"])
def test_the_fine_path_is_the_one_apply_takes(kind, shape):
    import torch
    gv, f, _, _ = case(kind, shape)
    flt = make_filter(kind, gv)
    x = torch.from_numpy(f[:1]).cuda()
    plan = ALL_KERNELS[GridType[kind]](**gv)._plan(_lib.F64, shape)      # the cached plan the Filter runs on
    plan.last_kernel()
    flt.apply(x)
    path, marching = flt.last_path, plan.last_kernel()
    assert path is not None and marching.startswith("gcmf::k_")
    other = make_filter(kind, gv)
    other.apply_coarsened(x, (5, 8) if shape == BLOCKED else (3, 5))
    assert other.last_path == path and plan.last_kernel() == marching
