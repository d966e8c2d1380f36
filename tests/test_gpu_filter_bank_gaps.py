"""``FilterBank(nan_mask="auto")`` on float64 IRREGULAR_WITH_LAND / MOM5U / MOM5T: gappy fields at many scales as ONE batch
(``gcmf_apply_bank_gaps``) -- every 2-D slice filtered with ``wet_mask * notnull(slice)`` at every scale, its face coefficients folded
once per slice and call (``k_pre_isolated``'s gap form), the launches ``k_ringc`` / ``k_land_fix`` in the instantiation that knows both the
polynomial of an entry and the planes of its field.

The contract: ``bank.apply(f)[j]`` is ``bank.filters[j].apply(f)`` (``Filter(nan_mask="auto")``) bit for bit, NaN exactly where ``f`` is NaN
(a gap is land in its own slice's mask; the plan's land cells keep their own polynomial, as in every filter here), and that is the reference's ``filter_func`` per scale and slice with the slice's own mask (the oracle of
tests/test_gpu_gap_fold.py).  Shapes, fields and gates are those of the bank and gap tests: (96, 160) and (200, 520), ``gappy_stack``,
identical NaN pattern and rel_err <= 1e-11."""
import functools

import numpy as np
import pytest

from gcm_filters_amd import FilterBank, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from test_gpu_filter_bank import BLOCKED, FIVE, KINDS, SMALL, THREE, check, host, loop_of, make_bank
from test_gpu_gap_fold import grid_vars, oracle, plan_of
from test_gpu_nan_mask import gappy_stack
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

CUTS = {24: [8, 8, 8], 14: [8, 6], 63: [9] * 7, 20: [8, 7, 5]}


def gaps_bank(kind, shape, n_steps, scales=THREE, gv=None, nan_mask="auto", **kw):
    return make_bank(kind, shape, n_steps, scales, gv=grid_vars(kind, shape) if gv is None else gv, nan_mask=nan_mask, **kw)


def oracle_of(bank, kind, stack, gv):
    return np.stack([oracle(f, kind, stack, gv) for f in bank.filters])


@functools.lru_cache(maxsize=None)
def _case(kind, shape, n_steps, scales):
    """(three gappy fields, the oracle per scale and field): computed once, shared, left unchanged (one field: the first of the three)."""
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 3, seed=40 + KINDS.index(kind))
    stack.setflags(write=False)
    want = oracle_of(gaps_bank(kind, shape, n_steps, scales), kind, stack, gv)
    want.setflags(write=False)
    return stack, want


# ---- 1. oracle parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("nfield", [1, 3])
@pytest.mark.parametrize("n_steps, scales", [(24, THREE), (14, THREE), (63, THREE), (20, THREE), (24, FIVE), (63, FIVE)])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_parity(kind, n_steps, scales, nfield, shape):
    gv = grid_vars(kind, shape)
    bank = gaps_bank(kind, shape, n_steps, scales)
    plan = plan_of(kind, gv, shape)
    M = len(scales)
    cut = plan.bank_cut(n_steps, M * nfield)
    assert cut == CUTS[n_steps], cut
    stack, want = _case(kind, shape, n_steps, scales)
    stack, want = np.array(stack[:nfield]), want[:, :nfield]     # (a writable copy: the shared case stays read-only)
    plan.last_kernel()
    got = bank.apply(stack)
    ran, geom = plan.last_kernel(), plan.last_kernel_geometry()
    assert bank.last_route == "bank" and bank.last_path == "strips"
    assert isinstance(got, np.ndarray) and got.shape == (M, nfield) + shape and got.dtype == np.float64
    assert ran.startswith(f"gcmf::k_ringc<double, 2, {max(cut)}, "), (ran, cut)
    assert list(geom)[-2:] == ["levels", "bank"] and geom["levels"] == nfield and geom["bank"] == M, geom
    assert geom["grid"].endswith(f"x{M * nfield}"), geom
    assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(stack), got.shape))
    check(got, want, (kind, n_steps, scales, nfield, shape, ran, cut))


def test_the_polynomials_run_every_depth_from_5_to_9():
    assert {s for c in CUTS.values() for s in c} == {5, 6, 7, 8, 9}


# ---- 2. the bits of the loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "numpy"])
@pytest.mark.parametrize("n_steps", [24, 63])
@pytest.mark.parametrize("kind", KINDS)
def test_the_bits_of_the_loop(monkeypatch, kind, n_steps, where):
    import torch
    shape = BLOCKED
    bank = gaps_bank(kind, shape, n_steps)
    stack = gappy_stack(shape, 3, seed=50 + KINDS.index(kind))
    x = torch.from_numpy(stack).cuda() if where == "device" else stack
    got = bank.apply(x)
    assert bank.last_route == "bank"
    assert (torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64) if where == "device" else isinstance(got, np.ndarray)
    assert tuple(got.shape) == (3, 3) + shape
    want = loop_of(bank, x)                     # [f.apply(stack) for f in bank.filters]: Filter(nan_mask="auto")
    assert np.array_equal(host(got), want, equal_nan=True), rel_err(host(got), want)
    monkeypatch.setenv("GCMF_FILTER_BANK", "0")
    slow = bank.apply(x)
    assert bank.last_route == "loop"
    assert np.array_equal(host(slow), host(got), equal_nan=True)
    monkeypatch.setenv("GCMF_FILTER_BANK", "1")
    assert np.array_equal(host(bank.apply(x)), host(got), equal_nan=True) and bank.last_route == "bank"


# ---- 3. NaN on the plan's land only --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nans_on_land_only_give_the_unmasked_bank(kind):
    shape = BLOCKED
    gv = grid_vars(kind, shape)
    f = np.stack([T.random_field(shape, 810 + b) for b in range(2)])
    land = gv["wet_mask"] == 0
    f[0][land] = np.nan
    f[1, 0, :] = np.nan                              # (the fixture's land row; the other land cells keep finite values)
    assert land[0].all() and not np.isnan(f[:, ~land]).any()
    on, off = gaps_bank(kind, shape, 24), gaps_bank(kind, shape, 24, nan_mask=False)
    got, want = on.apply(f), off.apply(f)
    assert on.last_route == "bank" and off.last_route == "bank"
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)


# ---- 4. coastline edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("kind", KINDS)
def test_gaps_on_the_edges_of_the_grid(kind, shape):
    ny, nx = shape
    gv = grid_vars(kind, shape)
    stack = np.stack([T.random_field(shape, 820 + b) for b in range(4)])
    for j in (0, ny - 1):                                     # the four corners
        for i in (0, nx - 1):
            stack[0, j, i] = np.nan
    stack[0, 0, [5, nx // 2, nx - 7]] = np.nan                # rows 0 and ny - 1
    stack[0, ny - 1, [7, nx // 3, nx - 5]] = np.nan
    stack[0, [1, ny // 3, ny - 2], 0] = np.nan                # columns 0 and nx - 1: the wrap in x
    stack[0, [2, ny // 2, ny - 3], nx - 1] = np.nan
    stack[1] = np.nan                                         # all NaN
    stack[3] = gappy_stack(shape, 1, seed=83)[0]              # (stack[2]: no gaps, beside gappy ones)
    bank = gaps_bank(kind, shape, 20)
    got = bank.apply(stack)
    assert bank.last_route == "bank"
    assert np.isnan(got[:, 1]).all()
    assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(stack), got.shape))
    want = loop_of(bank, stack)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    check(got, oracle_of(bank, kind, stack, gv), (kind, shape, "edges"))


# ---- 5. cuts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [4, 2], ids=["4-entries", "2-entries"])
def test_sweeps_longer_than_the_bound_are_cut(monkeypatch, bound):
    """Five scales x three fields with at most four entries per call (one scale and all fields each) and at most two (a scale's fields in
    two calls): over the scales, then over the fields."""
    import torch
    kind, shape = "MOM5U", SMALL
    bank = gaps_bank(kind, shape, 14, FIVE)
    x = torch.from_numpy(gappy_stack(shape, 3, seed=84)).cuda()
    whole = host(bank.apply(x))
    assert bank.last_route == "bank"
    calls = []
    orig = _lib.Plan.apply_bank
    monkeypatch.setattr(_lib.Plan, "apply_bank",
                        lambda self, p, c, s, o, n, **k: calls.append((len(p), n, k.get("faces_from_nan"))) or orig(self, p, c, s, o, n, **k))
    monkeypatch.setenv("GCMF_BANK_ENTRIES", str(bound))
    got = host(bank.apply(x))
    assert bank.last_route == "bank"
    assert calls == ([(1, 3, True)] * 5 if bound == 4 else [(1, 2, True), (1, 1, True)] * 5), calls
    assert np.array_equal(got, whole, equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_when_the_scratch_bound_cuts_the_fields(kind):
    """(200, 520): the planes of one field take 25 x 104 000 bytes = 2.6 MB, so a bound of 1 MiB runs one field at a time -- every
    polynomial for each -- and 6 MiB runs two and one."""
    import torch
    shape = BLOCKED
    gv = grid_vars(kind, shape)
    plan = plan_of(kind, gv, shape)
    bank = gaps_bank(kind, shape, 20)
    x = torch.from_numpy(gappy_stack(shape, 3, seed=85)).cuda()
    whole = host(bank.apply(x))
    assert bank.last_route == "bank" and plan.last_kernel_geometry()["levels"] == 3
    try:
        for mb, levels in ((1, 1), (6, 2)):
            plan.set_option("gap_scratch_mb", mb)
            plan.last_kernel()
            got = host(bank.apply(x))
            geom = plan.last_kernel_geometry()
            assert bank.last_route == "bank" and geom["bank"] == 1 and geom["levels"] in (levels, 1), (mb, geom)
            assert np.array_equal(got, whole, equal_nan=True), (mb, rel_err(got, whole))
    finally:
        plan.set_option("gap_scratch_mb", 4096)
    assert np.array_equal(host(bank.apply(x)), whole, equal_nan=True)


# ---- 6. the plan is put back -----------------------------------------------------------------------------------------------------------
def _status(fn, *a, **k):
    try:
        fn(*a, **k)
    except _lib.GcmfError as e:
        return e.status, e.message
    return _lib.OK, ""


@pytest.mark.parametrize("kind", KINDS)
def test_the_plan_is_put_back(kind):
    import torch
    shape = BLOCKED
    gv = grid_vars(kind, shape)
    plan = plan_of(kind, gv, shape)
    bank = gaps_bank(kind, shape, 24)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    spec = bank.filter_specs[0]
    c = 2 / spec.s_max
    f = torch.from_numpy(gappy_stack(shape, 2, seed=86)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def three_calls():
        plain, flagged = (torch.empty((2,) + shape, dtype=torch.float64, device="cuda") for _ in range(2))
        banked = torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda")
        plan.apply(P[1], c, [f.data_ptr()], [plain.data_ptr()], 2, device_ptrs=True, stream=stream)
        assert "levels" not in plan.last_kernel_geometry() and "bank" not in plan.last_kernel_geometry()
        plan.apply(P[1], c, [f.data_ptr()], [flagged.data_ptr()], 2, device_ptrs=True, stream=stream, faces_from_nan=True)
        plan.apply_bank(P, c, f.data_ptr(), banked.data_ptr(), 2, stream=stream)
        geom = plan.last_kernel_geometry()
        assert geom["bank"] == 3 and "levels" not in geom, geom
        return [t.cpu().numpy() for t in (plain, flagged, banked)]

    before = three_calls()
    assert not np.array_equal(before[0], before[1], equal_nan=True)
    out = torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda")
    plan.apply_bank(P, c, f.data_ptr(), out.data_ptr(), 2, stream=stream, faces_from_nan=True)
    assert plan.levels == 1 and plan.last_path() == "strips"
    got = out.cpu().numpy()
    for j in range(3):          # the C ABI's contract: gcmf_apply with the flag, one polynomial and one field at a time
        for i in range(2):
            one = torch.empty(shape, dtype=torch.float64, device="cuda")
            plan.apply(P[j], c, [f[i].data_ptr()], [one.data_ptr()], 1, device_ptrs=True, stream=stream, faces_from_nan=True)
            assert np.array_equal(got[j, i], one.cpu().numpy(), equal_nan=True), (j, i)
    assert np.array_equal(got[1], before[1], equal_nan=True)
    for a, b in zip(before, three_calls()):
        assert np.array_equal(a, b, equal_nan=True)
    # ... and after a refused one: three steps have no backward cut
    st, msg = _status(plan.apply_bank, P[:, :4], c, f.data_ptr(), out.data_ptr(), 2, stream=stream, faces_from_nan=True)
    assert st == _lib.ERR_UNSUPPORTED and "gcmf_apply_bank_gaps" in msg and "no backward cut" in msg, (st, msg)
    assert plan.levels == 1
    for a, b in zip(before, three_calls()):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 7. the fallbacks keep the contract -------------------------------------------------------------------------------------------------
def test_fallbacks_keep_the_contract():
    kind = "IRREGULAR_WITH_LAND"
    shape = SMALL
    gv = grid_vars(kind, shape)
    stack = gappy_stack(shape, 2, seed=87)

    def looped(bank, f):
        got = bank.apply(f)
        assert bank.last_route == "loop", bank
        want = loop_of(bank, f)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
        return got

    # nx % 4 != 0
    odd = (64, 102)
    godd = grid_vars(kind, odd)
    sodd = gappy_stack(odd, 2, seed=88)
    bank = gaps_bank(kind, odd, 24, gv=godd)
    got = looped(bank, sodd)
    assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(sodd), got.shape))
    check(got, oracle_of(bank, kind, sodd, godd), "nx % 4 != 0")
    # float32 grids
    g32 = {k: v.astype("f4") for k, v in gv.items()}
    bank = gaps_bank(kind, shape, 24, gv=g32)
    got = looped(bank, stack.astype("f4"))
    assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(stack), got.shape))
    # the forward recurrence
    bank = gaps_bank(kind, shape, 24, evaluation="reference")
    check(looped(bank, stack), oracle_of(bank, kind, stack, gv), "evaluation=reference")
    # one scale
    bank = gaps_bank(kind, shape, 24, (3.0,))
    check(looped(bank, stack), oracle_of(bank, kind, stack, gv), "one scale")
    # wet_mask with a leading axis
    g3 = dict(gv, wet_mask=np.stack([gv["wet_mask"]] * 2))
    g3["wet_mask"][1, 60:64, 100:110] = 0
    bank = gaps_bank(kind, shape, 24, gv=g3)
    check(looped(bank, stack), oracle_of(bank, kind, stack, g3), "a level axis")
    # a land-mask kind: True and "auto" both run the filters, which carry nan_mask
    g = T.scalar_grid_vars("REGULAR_WITH_LAND", shape)
    for value in (True, "auto"):
        bank = FilterBank(filter_scales=[2.0, 3.0, 4.5], dx_min=1.0, n_steps=24, grid_type=GridType.REGULAR_WITH_LAND, grid_vars=g,
                          nan_mask=value)
        got = looped(bank, stack)
        assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(stack), got.shape))
        off = FilterBank(filter_scales=[2.0, 3.0, 4.5], dx_min=1.0, n_steps=24, grid_type=GridType.REGULAR_WITH_LAND, grid_vars=g)
        assert not np.array_equal(got, off.apply(stack), equal_nan=True)


# ---- 8. the C ABI's refusals -------------------------------------------------------------------------------------------------------------
def _planes(kind, gv, dt="f8"):
    return [np.ascontiguousarray(gv[k], dtype=dt) for k in ALL_KERNELS[GridType[kind]].required_grid_args()]


def test_c_abi_refusals(monkeypatch):
    import torch
    kind, shape = "IRREGULAR_WITH_LAND", SMALL
    ny, nx = shape
    gv = grid_vars(kind, shape)
    plan = plan_of(kind, gv, shape)
    bank = gaps_bank(kind, shape, 24)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    c = 2 / bank.filter_specs[0].s_max
    f = torch.from_numpy(gappy_stack(shape, 2, seed=89)).cuda()
    out = torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda")
    src, dst = f.data_ptr(), out.data_ptr()

    def refused(pl, why, *a, status=_lib.ERR_UNSUPPORTED, **k):
        st, msg = _status(pl.apply_bank, *a, faces_from_nan=True, **k)
        assert st == status and "gcmf_apply_bank_gaps" in msg and why in msg, (why, st, msg)

    for other_kind, why in (("TRIPOLAR_POP_WITH_LAND", "TRIPOLAR_POP_WITH_LAND"), ("REGULAR_WITH_LAND", "another grid type"),
                            ("REGULAR", "another grid type")):
        g = T.scalar_grid_vars(other_kind, shape)
        other = _lib.Plan(GridType[other_kind].value, _lib.F64, ny, nx, _planes(other_kind, g))
        refused(other, why, P, c, src, dst, 2)
        other.close()
    f32 = _lib.Plan(GridType[kind].value, _lib.F32, ny, nx, _planes(kind, gv, "f4"))
    refused(f32, "an f32 plan", P, c, src, dst, 2)
    f32.close()
    lev = [np.stack([a] * 2) if k == 0 else a for k, a in enumerate(_planes(kind, gv))]
    stacked = _lib.Plan.create_levels(GridType[kind].value, _lib.F64, ny, nx, lev, [2] + [1] * (len(lev) - 1), 2)
    refused(stacked, "a stacked plan", P, c, src, dst, 2)
    stacked.close()
    slab = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv), row_begin=0, row_end=ny // 2, halo=9)
    refused(slab, "a row slab", P, c, src, dst, 2)
    slab.close()
    ring = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv), self_ring=True, halo=9)
    refused(ring, "GCMF_PLAN_SELF_RING", P, c, src, dst, 2)
    ring.close()
    refused(plan, "host pointers", P, c, src, dst, 2, device_ptrs=False)
    for flag, name in [(_lib.FORWARD_RECURRENCE, "GCMF_FORWARD_RECURRENCE"), (_lib.MASK_FROM_NAN, "GCMF_MASK_FROM_NAN"), (_lib.OUT_F32, "GCMF_OUT_F32")]:
        refused(plan, name, P, c, src, dst, 2, flags=flag)
    # a polynomial for which gcmf_bank_cut returns 0
    assert plan.bank_cut(4, 6) == [] and plan.bank_cut(24, 6) == [8, 8, 8]
    refused(plan, "gcmf_bank_cut returns 0", P[:, :5], c, src, dst, 2)
    monkeypatch.setenv("GCMF_CLENSHAW", "0")
    off = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv))
    monkeypatch.delenv("GCMF_CLENSHAW")
    assert off.bank_cut(24, 6) == []
    refused(off, "gcmf_bank_cut returns 0", P, c, src, dst, 2)
    off.close()
    odd = (ny, nx + 2)
    godd = T.scalar_grid_vars(kind, odd)
    podd = _lib.Plan(GridType[kind].value, _lib.F64, odd[0], odd[1], _planes(kind, godd))
    fo = torch.zeros((2,) + odd, dtype=torch.float64, device="cuda")
    oo = torch.empty((3, 2) + odd, dtype=torch.float64, device="cuda")
    refused(podd, "not a multiple of 4", P, c, fo.data_ptr(), oo.data_ptr(), 2)
    podd.close()
    # invalid arguments, as gcmf_apply_bank
    inv = dict(status=_lib.ERR_INVALID_ARG)
    refused(plan, "at least one polynomial", P[:0], c, src, dst, 2, **inv)
    refused(plan, "at least one step", P[:, :1], c, src, dst, 2, **inv)
    refused(plan, "null", P, c, 0, dst, 2, **inv)
    refused(plan, "null", P, c, src, 0, 2, **inv)
    refused(plan, "must not overlap", P, c, src, src, 2, **inv)
    refused(plan, "must not overlap", P, c, dst + 8 * ny * nx * 5, dst, 2, **inv)      # the input inside the output
    refused(plan, "must not overlap", P, c, src, src + 8 * ny * nx, 2, **inv)          # the output begins inside the input
    assert _status(plan.apply_bank, P, c, src, dst, 0, faces_from_nan=True) == (_lib.OK, "")
    # gcmf_apply_bank itself keeps refusing the flag
    st, msg = _status(plan.apply_bank, P, c, src, dst, 2, flags=_lib.FACES_FROM_NAN)
    assert st == _lib.ERR_UNSUPPORTED and "GCMF_FACES_FROM_NAN" in msg
    torch.cuda.synchronize()
    # ... and a real call counts its launches: the fold and three strip launches (+ k_land_fix, not counted)
    plan.apply_bank(P, c, src, dst, 2, faces_from_nan=True)
    assert plan.last_path() == "strips" and plan.last_timing()[1] == 4


# ---- 9. xarray -----------------------------------------------------------------------------------------------------------------------------
def test_xarray_dataarray(monkeypatch):
    from conftest import xarray_backend
    xr = xarray_backend("model", monkeypatch)
    kind, shape = "MOM5U", SMALL
    gv = grid_vars(kind, shape)
    gvx = {k: xr.DataArray(v, dims=["y", "x"]) for k, v in gv.items()}
    bank = gaps_bank(kind, shape, 24, gv=gvx)
    f = gappy_stack(shape, 3, seed=90)
    out = bank.apply(xr.DataArray(f, dims=["time", "y", "x"]), dims=["y", "x"])
    assert bank.last_route == "bank"
    assert tuple(out.dims) == ("time", "filter_scale", "y", "x") and out.data.shape == (3, 3) + shape
    want = loop_of(gaps_bank(kind, shape, 24), f)
    assert np.array_equal(np.moveaxis(np.asarray(out.data), 1, 0), want, equal_nan=True)
