"""Gappy fields on the flux-form grid types: ``Filter(nan_mask="auto")`` / ``GCMF_FACES_FROM_NAN`` on IRREGULAR_WITH_LAND, MOM5U, MOM5T.

The contract: batch entry b is filtered with m_b = wet_mask * [field_b is not NaN] -- the reference's ``filter_func`` with ``wet_mask``
replaced by m_b (the oracle called once per entry) -- and the result has the bits of the stacked plan built from the explicit masks.
Fields: ``gappy_stack`` of tests/test_gpu_nan_mask.py (15 % random gaps plus blobs, different per entry) on (96, 160) and (200, 520).
Gates are those of tests/test_gpu_level_stack.py: NaN pattern equal to the input's, rel_err <= 1e-11 against the oracle.

The polynomials of 24, 63 and 20 steps are cut into launches of (8 8 8), (9 x 7) and (8 7 5) levels on these grids; a fourth of 14 steps
(8 6) is filtered as well so that every depth from 5 to 9 occurs -- test_the_polynomials_run_every_depth_from_5_to_9 reads the cuts."""
import functools
import threading

import numpy as np
import pytest

from gcm_filters_amd import GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
from oracle import gcmf_oracle as O
from test_gpu_level_stack import check, make_filter
from test_gpu_nan_mask import gappy_stack

pytestmark = pytest.mark.gpu

KINDS = ["IRREGULAR_WITH_LAND", "MOM5U", "MOM5T"]
SMALL, BLOCKED, RAGGED = (96, 160), (200, 520), (64, 102)
N_STEPS = [24, 63, 20, 14]
FLAG = "GCMF_FACES_FROM_NAN"


@functools.lru_cache(maxsize=None)
def grid_vars(kind, shape):
    gv = T.scalar_grid_vars(kind, shape)
    if kind == "IRREGULAR_WITH_LAND":
        gv["kappa_w"] = T.smooth_kappa(shape, 11)
    return gv


def auto_filter(kind, gv, n_steps, **kw):
    kw.setdefault("nan_mask", "auto")
    return make_filter(kind, gv, n_steps, **kw)


def oracle(flt, kind, stack, gv):
    """The reference's filter_func per entry, wet_mask replaced by wet_mask * notnull(entry); the polynomial is the Filter's own."""
    fs = flt.filter_spec
    spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
    flat = stack.reshape((-1,) + stack.shape[-2:])
    gv = {k: np.asarray(v, dtype=np.float64) for k, v in gv.items()}
    wm = np.broadcast_to(gv["wet_mask"], stack.shape[:-2] + gv["wet_mask"].shape[-2:]).reshape((-1,) + stack.shape[-2:]) \
        if gv["wet_mask"].ndim > 2 else [gv["wet_mask"]] * len(flat)
    with np.errstate(all="ignore"):
        res = [O.filter_func(spec, kind, np.asarray(f, dtype=np.float64), {**gv, "wet_mask": m * ~np.isnan(f)}) for f, m in zip(flat, wm)]
    return np.stack(res).reshape(stack.shape)


def plan_of(kind, gv, shape):
    return ALL_KERNELS[GridType[kind]](**gv)._plan(_lib.F64, shape)


def explicit(kind, gv, stack, flt, stacked):
    """The routes that existed before the flag: wet_mask(n, y, x) = wet_mask * notnull(stack) as a grid variable -- one stacked plan, or one
    plan and one call per entry."""
    m = gv["wet_mask"] * ~np.isnan(stack)
    lap = ALL_KERNELS[GridType[kind]](**{**gv, "wet_mask": m.astype(np.float64)}, _stack_levels=stacked)
    assert lap._stacked == stacked
    return lap._run([stack], spec=flt.filter_spec)[0]


@functools.lru_cache(maxsize=None)
def _case(kind, shape, nb, n_steps):
    """(stack, oracle) of a parity case: computed once, shared by the tests that need it and left unchanged."""
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, nb, seed=KINDS.index(kind) + 3 * nb)
    stack.setflags(write=False)
    want = oracle(auto_filter(kind, gv, n_steps), kind, stack, gv)
    want.setflags(write=False)
    return stack, want


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("n_steps", N_STEPS)
@pytest.mark.parametrize("nb", [1, 3, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_parity(kind, nb, n_steps, shape):
    import torch
    gv = grid_vars(kind, shape)
    stack, want = _case(kind, shape, nb, n_steps)
    flt = auto_filter(kind, gv, n_steps)
    plan = plan_of(kind, gv, shape)
    cut = plan.clenshaw_cut(n_steps, nb)
    plan.last_kernel()
    got = flt.apply(stack)                                        # a numpy array
    ran, geom = plan.last_kernel(), plan.last_kernel_geometry()
    assert flt.last_path == "strips"
    assert np.array_equal(np.isnan(got), np.isnan(stack))         # NaN exactly where the input is NaN
    check(got, want, (kind, nb, n_steps, shape, ran, cut))
    dev = flt.apply(torch.from_numpy(stack.copy()).cuda())        # a device tensor
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and flt.last_path == "strips"
    assert np.array_equal(dev.cpu().numpy(), got, equal_nan=True)
    if shape == BLOCKED:
        assert ran.startswith("gcmf::k_ringc<double"), ran
        assert geom.get("levels") is not None and geom["grid"].endswith(f"x{geom['levels']}"), geom    # a stacked plan's launch: the entries are its levels


def test_the_polynomials_run_every_depth_from_5_to_9():
    seen = set()
    for shape in (SMALL, BLOCKED):
        plan = plan_of("IRREGULAR_WITH_LAND", grid_vars("IRREGULAR_WITH_LAND", shape), shape)
        for nb in (3, 17):       # (a lone field on an ordinary plan may be cut shallower: the flagged call is a stacked plan's, never that)
            for n in N_STEPS:
                seen |= set(plan.clenshaw_cut(n, nb))
    assert seen == {5, 6, 7, 8, 9}, seen


# ---- 2. the same bits as the routes through explicit masks -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_as_the_explicit_masks(kind):
    shape, nb, n_steps = BLOCKED, 5, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, nb, seed=40 + KINDS.index(kind))
    flt = auto_filter(kind, gv, n_steps)
    fast = flt.apply(stack)
    for stacked in (True, False):
        slow = explicit(kind, gv, stack, flt, stacked)
        assert fast.dtype == slow.dtype and np.array_equal(fast, slow, equal_nan=True), (kind, stacked)


# ---- 3. the scratch bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_however_the_scratch_bound_cuts_the_batch(kind, shape):
    """25 bytes per cell and entry: 1 MiB holds two entries of (96, 160) and none of (200, 520), so five entries go in three launches
    (2 2 1) or five; the default bound takes them in one."""
    import torch
    nb, n_steps = 5, 20
    gv = grid_vars(kind, shape)
    dev = torch.from_numpy(gappy_stack(shape, nb, seed=50 + KINDS.index(kind))).cuda()
    flt = auto_filter(kind, gv, n_steps)
    plan = plan_of(kind, gv, shape)
    plan.last_kernel()
    whole = flt.apply(dev).cpu().numpy()
    plan.last_kernel()
    assert plan.last_kernel_geometry()["grid"].endswith("x5")
    try:
        plan.set_option("gap_scratch_mb", 1)
        plan.last_kernel()
        cut = flt.apply(dev).cpu().numpy()
        plan.last_kernel()
        assert plan.last_kernel_geometry()["grid"].endswith("x1")       # the last launch of (2 2 1) or (1 1 1 1 1)
    finally:
        plan.set_option("gap_scratch_mb", 4096)
    assert np.array_equal(cut, whole, equal_nan=True)


# ---- 4. the streamed host path ----------------------------------------------------------------------------------------------------
def test_host_batch_streamed_in_chunks(monkeypatch):
    """A host batch cut into chunks of two entries (seven entries: four chunks): every chunk folds its own entries' planes."""
    import torch
    kind, shape, nb, n_steps = "IRREGULAR_WITH_LAND", SMALL, 7, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, nb, seed=91)
    want = auto_filter(kind, gv, n_steps).apply(torch.from_numpy(stack).cuda()).cpu().numpy()      # one launch, device-resident
    clear_plan_cache()
    monkeypatch.setenv("GCMF_HOST_CHUNK_MB", str(2.5 * shape[0] * shape[1] * 8 / 2**20))
    try:
        flt = auto_filter(kind, gv, n_steps)
        got = flt.apply(stack)
        plan = plan_of(kind, gv, shape)
        plan.last_kernel()
        assert plan.last_kernel_geometry()["grid"].endswith("x1")       # the last chunk: one entry
    finally:
        clear_plan_cache()
    assert np.array_equal(got, want, equal_nan=True)
    check(got, oracle(flt, kind, stack, gv), (kind, "host chunks"))


# ---- 5. hand-drawn gaps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("kind", KINDS)
def test_hand_drawn_gaps(kind, shape):
    ny, nx = shape
    n_steps = 24
    gv = grid_vars(kind, shape)
    wet = gv["wet_mask"] == 1
    stack = np.stack([T.random_field(shape, 300 + b) for b in range(4)])
    stack[0, 0, [0, 5, nx // 2, nx - 1]] = np.nan                    # row 0, row ny - 1, column 0, column nx - 1: the wrap applies
    stack[0, ny - 1, [0, 7, nx - 1]] = np.nan
    stack[0, [1, ny // 3, ny - 2], 0] = np.nan
    stack[0, [2, ny // 2, ny - 3], nx - 1] = np.nan
    coast = wet & ~(np.roll(wet, 1, 0) & np.roll(wet, -1, 0) & np.roll(wet, 1, 1) & np.roll(wet, -1, 1))
    cj, ci = np.nonzero(coast)
    assert len(cj) > 20
    stack[1, cj[::3], ci[::3]] = np.nan                               # gaps touching land
    inner = wet & np.roll(wet, 1, 0) & np.roll(wet, -1, 0) & np.roll(wet, 1, 1) & np.roll(wet, -1, 1)
    inner[:2] = inner[-2:] = False
    inner[:, :2] = inner[:, -2:] = False
    jj, ii = np.argwhere(inner)[len(np.argwhere(inner)) // 2]         # a wet cell enclosed by gaps
    for dj, di in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        stack[2, jj + dj, ii + di] = np.nan
    stack[3] = np.nan                                                 # an entry that is all NaN
    flt = auto_filter(kind, gv, n_steps)
    got = flt.apply(stack)
    assert np.array_equal(np.isnan(got), np.isnan(stack))
    check(got, oracle(flt, kind, stack, gv), (kind, shape, "hand-drawn"))
    p = np.asarray(flt.filter_spec.p)                                 # its value passes through: sum_k p_k (-1)^k f, as on land
    alone = float(np.sum(p * (-1.0) ** np.arange(len(p))))
    assert abs(got[2, jj, ii] - alone * stack[2, jj, ii]) <= 1e-12 * abs(stack[2, jj, ii])


@pytest.mark.parametrize("kind", KINDS)
def test_inf_in_a_wet_cell_is_data_not_a_gap(kind):
    """+-inf in wet cells: the cell keeps its faces (only NaN is a gap).  Against the explicit-mask route, for bits."""
    shape, nb, n_steps = BLOCKED, 3, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, nb, seed=95)
    wet = np.argwhere((gv["wet_mask"] == 1) & ~np.isnan(stack).any(axis=0))
    (j0, i0), (j1, i1) = wet[len(wet) // 5], wet[len(wet) // 2]
    stack[0, j0, i0] = np.inf
    stack[1, j1, i1] = -np.inf
    flt = auto_filter(kind, gv, n_steps)
    with np.errstate(all="ignore"):
        got = flt.apply(stack)
        want = explicit(kind, gv, stack, flt, True)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[0, j0, i0 + 1]) or np.isinf(got[0, j0, i0 + 1])      # it spread: the face east of the cell is open
    assert np.array_equal(np.isnan(got[2]), np.isnan(stack[2]))


# ---- 6. it is really on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_gaps_are_land_not_zeros(kind):
    shape, n_steps = SMALL, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 3, seed=7)
    on = auto_filter(kind, gv, n_steps).apply(stack)
    off = auto_filter(kind, gv, n_steps, nan_mask=False).apply(stack)
    assert np.array_equal(np.isnan(on), np.isnan(off))
    gap = np.isnan(stack)
    near = (np.roll(gap, 1, -1) | np.roll(gap, -1, -1) | np.roll(gap, 1, -2) | np.roll(gap, -1, -2)) & ~gap & (gv["wet_mask"] == 1)
    amp = np.nanmax(stack) - np.nanmin(stack)
    diff = np.abs(on - off)[near].max() / amp
    print(f"{kind}: largest difference next to gaps {diff:.3f} of the field's amplitude")
    assert diff > 0.1, diff
    full = np.stack([T.random_field(shape, 77 + b) for b in range(3)])       # no NaN: nothing to treat differently
    assert np.array_equal(auto_filter(kind, gv, n_steps).apply(full), auto_filter(kind, gv, n_steps, nan_mask=False).apply(full))


# ---- 7. the plan is left as it was ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_flagged_and_unflagged_calls_share_a_plan(kind):
    import torch
    shape, n_steps = BLOCKED, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 3, seed=11)
    on, off = auto_filter(kind, gv, n_steps), auto_filter(kind, gv, n_steps, nan_mask=False)
    plan = plan_of(kind, gv, shape)
    want_off = off.apply(stack)                      # before any flagged call
    lone_off = off.apply(stack[1])                   # (a lone field: the zipped strips and the wet-row table)
    want_on = on.apply(stack)
    assert not np.array_equal(want_on, want_off, equal_nan=True)
    assert np.array_equal(off.apply(stack), want_off, equal_nan=True) and np.array_equal(off.apply(stack[1]), lone_off, equal_nan=True)
    x = torch.from_numpy(stack).cuda()
    y = torch.empty_like(x)
    with pytest.raises(_lib.GcmfError) as e:         # refused INSIDE the call, with the entries' planes in place: three steps have no backward cut
        plan.apply(np.array([0.5, -0.3, 0.1, 0.05]), 0.2, [x.data_ptr()], [y.data_ptr()], 3, device_ptrs=True, faces_from_nan=True)
    assert e.value.status == _lib.ERR_UNSUPPORTED and FLAG in e.value.message and "no backward cut" in e.value.message
    assert plan.levels == 1
    for _ in range(2):
        assert np.array_equal(off.apply(stack), want_off, equal_nan=True)
        assert np.array_equal(off.apply(stack[1]), lone_off, equal_nan=True)
        assert np.array_equal(on.apply(stack[1]), want_on[1], equal_nan=True)
        assert np.array_equal(on.apply(stack), want_on, equal_nan=True)
    bad = []

    def work(flt, want):
        for _ in range(6):
            if not np.array_equal(flt.apply(stack), want, equal_nan=True):
                bad.append(flt.nan_mask)
    threads = [threading.Thread(target=work, args=a) for a in ((on, want_on), (off, want_off))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(_lib.GcmfError) as e:
        call()
    assert e.value.status == _lib.ERR_UNSUPPORTED, e.value
    assert FLAG in e.value.message, e.value.message
    for kind in KINDS:
        assert kind in e.value.message, e.value.message
    return e.value.message


def _flagged(plan, shape, nb=1, dt="f8", **kw):
    import torch

    def call():
        x = torch.rand((nb,) + tuple(shape), dtype=torch.float64 if dt == "f8" else torch.float32, device="cuda")
        y = torch.empty((nb,) + tuple(shape), dtype=torch.float64, device="cuda")
        plan.apply(np.array([0.5, -0.3, 0.1, 0.05, 0.02, 0.01]), 0.2, [x.data_ptr()], [y.data_ptr()], nb, device_ptrs=True,
                   faces_from_nan=True, **kw)
        torch.cuda.synchronize()
    return call


def _make_plan(kind, shape, dt=_lib.F64, **kw):
    gv = T.scalar_grid_vars(kind, shape)
    names = ALL_KERNELS[GridType[kind]].required_grid_args()
    return _lib.Plan(GridType[kind].value, dt, *shape, [gv[k].astype(_lib.np_dtype(dt)) for k in names], **kw)


def test_c_abi_refusals():
    import ctypes as C
    import torch
    shape = (64, 96)
    for kind in ("REGULAR", "REGULAR_WITH_LAND", "TRIPOLAR_POP_WITH_LAND"):       # any other grid type
        plan = _make_plan(kind, shape)
        try:
            assert "another grid type" in _refused(_flagged(plan, shape))
        finally:
            plan.close()
    plan = _make_plan("MOM5U", shape, _lib.F32)                                    # f32 plans
    try:
        assert "f32" in _refused(_flagged(plan, shape, dt="f4"))
    finally:
        plan.close()
    slab = _make_plan("MOM5T", shape, row_begin=16, row_end=48, halo=8)            # row slabs
    try:
        assert "row slab" in _refused(_flagged(slab, (slab.rows_alloc, shape[1])))
    finally:
        slab.close()
    gv = T.scalar_grid_vars("IRREGULAR_WITH_LAND", shape)                          # stacked plans
    names = ALL_KERNELS[GridType.IRREGULAR_WITH_LAND].required_grid_args()
    planes = [np.stack([gv[k], gv[k]]) if k == "wet_mask" else gv[k] for k in names]
    stacked = _lib.Plan.create_levels(GridType.IRREGULAR_WITH_LAND.value, _lib.F64, *shape, planes, [2 if k == "wet_mask" else 1 for k in names], 2)
    try:
        assert "stacked" in _refused(_flagged(stacked, shape, nb=2))
    finally:
        stacked.close()
    plan = _make_plan("IRREGULAR_WITH_LAND", shape)
    try:
        assert "GCMF_FORWARD_RECURRENCE" in _refused(_flagged(plan, shape, forward=True))       # combined with the other flags
        assert "GCMF_MASK_FROM_NAN" in _refused(_flagged(plan, shape, mask_from_nan=True))
        x = torch.rand((1,) + shape, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        assert "no backward cut" in _refused(lambda: plan.apply(np.array([0.5, -0.3, 0.1]), 0.2, [x.data_ptr()], [y.data_ptr()], 1,
                                                                device_ptrs=True, faces_from_nan=True))
        lib = _lib.load()
        flags = _lib.DEVICE_PTRS | _lib.FACES_FROM_NAN
        px, py, pz = _lib._ptr_array([x.data_ptr()]), _lib._ptr_array([y.data_ptr()]), _lib._ptr_array([None])
        pk = (C.c_double * 8)(*([0.1] * 8))
        assert "gcmf_laplacian" in _refused(lambda: _lib.check(lib.gcmf_laplacian(plan._h, px, py, 1, flags, None)))
        # the building blocks and the slab drivers: refused before any argument is looked at
        _refused(lambda: _lib.check(lib.gcmf_cheb_step(plan._h, px, pz, pz, py, py, 0.5, 0.1, 0.2, _lib.STEP_FIRST, flags, 1, 0, shape[0], None)))
        _refused(lambda: _lib.check(lib.gcmf_cheb_multi(plan._h, None, None, None, None, None, None, pk, 5, 0.5, 0.2, _lib.STEP_FIRST, flags, 1, 0,
                                                        shape[0], None)))
        _refused(lambda: _lib.check(lib.gcmf_cheb_multi_vec(plan._h, px, pz, py, py, pz, py, pk, 5, 0.5, 0.2, _lib.STEP_FIRST, flags, 1, 0,
                                                            shape[0], None)))
        _refused(lambda: _lib.check(lib.gcmf_land_fix(plan._h, pk, 5, 0.2, px, py, 1, flags, None)))
        _refused(lambda: _lib.check(lib.gcmf_slab_apply_backward(plan._h, None, None, -1, -1, pk, 5, 0.2, (C.c_int * 1)(5), 1, None, pz, None, 1, 0, 0,
                                                                 flags, None)))
        _refused(lambda: _lib.check(lib.gcmf_slab_apply_backward_vec(plan._h, None, None, -1, -1, pk, 5, 0.2, px, pz, py, 1, 0, flags, None)))
    finally:
        plan.close()
    with pytest.raises(ValueError, match="IRREGULAR_WITH_LAND, MOM5U, MOM5T"):        # ... and the Python driver, one Laplacian
        ALL_KERNELS[GridType.MOM5U](**T.scalar_grid_vars("MOM5U", shape))._run([np.zeros(shape)], faces_from_nan=True)


# ---- 9. the fallbacks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fallback_ragged_rows(kind):
    """nx % 4 != 0: no land fix-up, no backward cut -- the explicit masks as grid variables with a level axis."""
    shape, n_steps = RAGGED, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 3, seed=61)
    flt = auto_filter(kind, gv, n_steps)
    got = flt.apply(stack)
    check(got, oracle(flt, kind, stack, gv), (kind, shape, "nx % 4 != 0"))
    one = flt.apply(stack[1])
    assert np.array_equal(one, got[1], equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_reference_evaluation_and_float32(kind):
    shape, n_steps = SMALL, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 3, seed=63)
    flt = auto_filter(kind, gv, n_steps, evaluation="reference")
    check(flt.apply(stack), oracle(flt, kind, stack, gv), (kind, "reference"))
    gv32 = {k: v.astype("f4") for k, v in gv.items()}
    s32 = stack.astype("f4")
    f32 = auto_filter(kind, gv32, n_steps)
    got = f32.apply(s32)
    want = oracle(f32, kind, s32, gv32)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(s32))
    from test_gpu_parity import RTOL_F32, rel_err
    err = rel_err(got, want)
    print(f"{kind} float32: rel_err {err:.3e}")
    assert err <= RTOL_F32, err


def test_fallback_leaves_no_plan_in_the_cache():
    from gcm_filters_amd.kernels import PLAN_CACHE
    kind, shape = "MOM5T", RAGGED
    gv = grid_vars(kind, shape)
    flt = auto_filter(kind, gv, 24)
    flt.apply(gappy_stack(shape, 2, seed=65))
    before = len(PLAN_CACHE._d)
    flt.apply(gappy_stack(shape, 3, seed=66))
    assert len(PLAN_CACHE._d) == before


def test_grid_variables_with_a_level_axis():
    """kappa_w(level, y, x): the per-level plans run the flagged call, each on its own entries."""
    kind, shape, n_steps, nlev = "IRREGULAR_WITH_LAND", SMALL, 24, 3
    gv = dict(grid_vars(kind, shape))
    gv["kappa_w"] = np.stack([T.smooth_kappa(shape, 21 + l) for l in range(nlev)])
    stack = gappy_stack(shape, 2 * nlev, seed=31).reshape((2, nlev) + shape)
    flt = auto_filter(kind, gv, n_steps)
    got = flt.apply(stack)
    fs = flt.filter_spec
    spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
    with np.errstate(all="ignore"):
        want = np.asarray([[O.filter_func(spec, kind, stack[a, l], {**gv, "kappa_w": gv["kappa_w"][l],
                                                                    "wet_mask": gv["wet_mask"] * ~np.isnan(stack[a, l])})
                            for l in range(nlev)] for a in range(2)])
    check(got, want, (kind, "kappa_w(level, y, x)"))


def test_xarray_front_door(monkeypatch):
    from conftest import xarray_backend
    xr = xarray_backend("model", monkeypatch)
    kind, shape, n_steps = "MOM5U", SMALL, 24
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 4, seed=51)
    gvx = {k: xr.DataArray(v, dims=["y", "x"]) for k, v in gv.items()}
    flt = auto_filter(kind, gvx, n_steps)
    out = flt.apply(xr.DataArray(stack, dims=["time", "y", "x"]), dims=["y", "x"])
    assert out.dims == ("time", "y", "x")
    check(out.data, oracle(flt, kind, stack, gv), (kind, "xarray"))
