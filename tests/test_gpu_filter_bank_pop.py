"""``FilterBank`` on TRIPOLAR_POP_WITH_LAND: the scales of a sweep as ONE batch of the backward evaluation with a polynomial per entry
(``gcmf_apply_bank``) on the grid with the tripole seam.  The plain strips (``k_ringc``'s per-entry form) stop S rows below the seam; its rows
are advanced by ``k_fold_band``'s per-entry form -- entry e of a launch is polynomial e / nfield on field e % nfield, coefficients from the
table the strips read -- after every strip launch (1024 threads per tile) or beside it (256), in launches of 5 .. 8 levels.

The contract is FilterBank's: ``bank.apply(f)[j]`` has the bits of ``bank.filters[j].apply(f)`` and is the reference's ``filter_func`` with
scale j's polynomial (identical NaN pattern, rel_err <= 1e-11 against the oracle, once per scale).  Shapes:
  (96, 160)   two strip windows that wrap, five mirrored band window pairs that fit exactly, the band after the strips; the lone-field loop
              runs the band too (nx < 256)
  (96, 168)   nx / 2 no multiple of the band's 16 useful columns: a partial last window pair
  (200, 520)  several windows and strips; the lone-field loop runs the zipped fold strips, so bit equality ties the two seam implementations
              together per scale
  (ny, 64)    the shortest grid ``plan.bank_cut`` offers a bank on, found from bank_cut; one row fewer has none
Whether a bank is the DEFAULT on this grid type is a measured decision (filter._bank_by_default); these tests ask for it with
GCMF_FILTER_BANK=1, the last one also reads the default."""
import functools

import numpy as np
import pytest

from gcm_filters_amd import GridType, _lib, testing as T
from gcm_filters_amd.filter import _bank_by_default
from test_gpu_filter_bank import (FIVE, THREE, _oracle, _planes, _status, check, field_for, grid_vars, host, loop_of, make_bank, oracle_of,
                                  plan_of)
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

KIND = "TRIPOLAR_POP_WITH_LAND"
SMALL, PARTIAL, BLOCKED = (96, 160), (96, 168), (200, 520)
BAND_SEQ_CELLS = 3000000      # the plan option's default (csrc/gcmf_internal.hpp)


@pytest.fixture(autouse=True)
def ask_for_the_bank(monkeypatch):
    monkeypatch.setenv("GCMF_FILTER_BANK", "1")


def band_launches(cut):
    """advance_multi counts one k_fold_band launch per strip launch on the seam's plan (beside it or after it)."""
    return 2 * len(cut)


# ---- 1. oracle parity and the bits of the loop, per scale --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, PARTIAL, BLOCKED], ids=["96x160", "96x168", "200x520"])
@pytest.mark.parametrize("n_steps, scales", [(24, THREE), (14, THREE), (20, THREE), (63, THREE), (24, FIVE), (14, FIVE), (20, FIVE), (63, FIVE)])
def test_oracle_parity_and_loop_bits_per_scale(n_steps, scales, shape):
    gv = grid_vars(KIND, shape)
    bank = make_bank(KIND, shape, n_steps, scales)
    plan = plan_of(KIND, shape)
    M = len(scales)
    cut = plan.bank_cut(n_steps, M)
    assert cut and sum(cut) == n_steps and all(5 <= s <= 8 for s in cut), cut      # k_fold_band stops at eight levels
    f = field_for(shape)
    plan.last_kernel()
    got = bank.apply(f)
    ran, geom, launches = plan.last_kernel(), plan.last_kernel_geometry(), plan.last_timing()[1]
    assert bank.last_route == "bank" and bank.last_path == "strips"
    assert plan.bank_cut(n_steps, M) == cut                                         # the same answer outside and after a call
    assert isinstance(got, np.ndarray) and got.shape == (M,) + shape and got.dtype == np.float64
    assert ran.startswith(f"gcmf::k_ringc<double, 2, {max(cut)}, "), (ran, cut)
    assert list(geom)[-1] == "bank" and geom["bank"] == M and geom["grid"].endswith(f"x{M}"), geom
    assert geom["rows"] == shape[0] - max(cut), geom                                # the strips stop below the band
    assert launches == band_launches(cut), (launches, cut)
    want = np.stack([_oracle(KIND, shape, n_steps, s, 700) for s in scales])
    check(got, want, (KIND, n_steps, scales, shape, ran, cut))
    land = gv["wet_mask"] == 0
    land[0, :] = False
    assert land.sum() > 100 and np.isfinite(got[:, land]).all()
    check(got[:, land], want[:, land], (KIND, n_steps, shape, "land"))
    for j in range(1, M):
        assert not np.array_equal(got[j][land], got[0][land]), j
    loop = loop_of(bank, f)
    assert np.array_equal(got, loop, equal_nan=True), rel_err(got, loop)


def test_the_loop_on_the_wide_grid_runs_the_zipped_fold_strips():
    """... so that the bit equality above compares k_fold_band's per-entry form with the seam inside k_ringcz, and on the narrow grids with
    the ordinary k_fold_band."""
    import torch
    for shape, seam_inside in ((BLOCKED, True), (SMALL, False)):
        bank = make_bank(KIND, shape, 24)
        plan = plan_of(KIND, shape)
        f = torch.from_numpy(field_for(shape)).cuda()
        plan.last_kernel()
        bank.filters[0].apply(f)
        if bank.filters[0].last_path == "strips":      # (the on-chip kernel may take a grid this small: the same bits, another route)
            ran, geom, launches = plan.last_kernel(), plan.last_kernel_geometry(), plan.last_timing()[1]
            cut = plan.clenshaw_cut(24, 1)
            assert "bank" not in geom
            # the strips own every row and no band launch ran / they stop below the band and one band launch ran per strip launch
            assert geom["rows"] == (shape[0] if seam_inside else shape[0] - max(cut)), (shape, ran, geom, cut)
            assert launches == (len(cut) if seam_inside else 2 * len(cut)), (shape, launches, cut)
            assert ("k_ringcz<" in ran) or not seam_inside, ran


# ---- 2. first launches of 5, 6, 7 levels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smax", [5, 6, 7])
def test_first_launches_of_every_depth(smax):
    import torch
    shape = BLOCKED
    bank = make_bank(KIND, shape, 5 * smax)
    plan = plan_of(KIND, shape)
    f = torch.from_numpy(field_for(shape)).cuda()
    want = bank.apply(f).cpu().numpy()
    assert bank.last_route == "bank"
    try:
        plan.set_option("ringc_smax", smax)
        assert plan.bank_cut(5 * smax, 3) == [smax] * 5
        plan.last_kernel()
        got = bank.apply(f).cpu().numpy()
        assert bank.last_route == "bank" and plan.last_kernel().startswith(f"gcmf::k_ringc<double, 2, {smax}, "), smax
        assert plan.last_timing()[1] == band_launches([smax] * 5)
    finally:
        plan.set_option("ringc_smax", 0)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    assert np.array_equal(want, loop_of(bank, f), equal_nan=True)


# ---- 3. the band beside the launch (256 threads per tile) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [24, 20])
def test_the_band_beside_the_launch(n_steps):
    import torch
    shape = BLOCKED
    bank = make_bank(KIND, shape, n_steps, FIVE)
    plan = plan_of(KIND, shape)
    f = torch.from_numpy(field_for(shape, 705, (2,))).cuda()
    want = bank.apply(f).cpu().numpy()                  # the default: 10 x 200 x 520 cells, the band after the strips
    try:
        plan.set_option("band_seq_cells", 0)
        got = bank.apply(f).cpu().numpy()
        assert bank.last_route == "bank" and plan.last_timing()[1] == band_launches(plan.bank_cut(n_steps, 10))
    finally:
        plan.set_option("band_seq_cells", BAND_SEQ_CELLS)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    assert np.array_equal(got, loop_of(bank, f), equal_nan=True)


# ---- 4. leading axes: entry -> (polynomial, field) inside the band ------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [(), (2,), (2, 3)], ids=["1", "2", "2x3"])
@pytest.mark.parametrize("where", ["device", "numpy"])
def test_leading_axes(where, lead):
    import torch
    shape = PARTIAL
    bank = make_bank(KIND, shape, 20, FIVE)
    f = field_for(shape, 710, lead)                     # (every slice from its own seed: a swapped index shows)
    x = torch.from_numpy(f).cuda() if where == "device" else f
    plan_of(KIND, shape).last_kernel()
    got = bank.apply(x)
    assert bank.last_route == "bank"
    assert (torch.is_tensor(got) and got.is_cuda) if where == "device" else isinstance(got, np.ndarray)
    assert tuple(got.shape) == (5,) + tuple(lead) + shape
    assert plan_of(KIND, shape).last_kernel_geometry()["grid"].endswith(f"x{5 * max(1, int(np.prod(lead, dtype=int)))}")
    want = loop_of(bank, x)
    assert np.array_equal(host(got), want, equal_nan=True), rel_err(host(got), want)
    top = host(got)[..., -8:, :]                        # the band's rows differ between scales and between fields
    assert not np.array_equal(top[0], top[1], equal_nan=True)
    if lead:
        flat = top.reshape((5, -1) + top.shape[-2:])
        assert not np.array_equal(flat[:, 0], flat[:, 1], equal_nan=True)


# ---- 5. GCMF_BANK_ENTRIES: ent0 inside the band --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [4, 2], ids=["4-entries", "2-entries"])
def test_sweeps_longer_than_the_bound_are_cut(monkeypatch, bound):
    import torch
    shape = SMALL
    bank = make_bank(KIND, shape, 14, FIVE)
    x = torch.from_numpy(field_for(shape, 730, (3,))).cuda()
    whole = host(bank.apply(x))
    calls = []
    cls = _lib.Plan
    orig = cls.apply_bank
    monkeypatch.setattr(cls, "apply_bank", lambda self, p, c, s, o, n, **k: calls.append((len(p), n)) or orig(self, p, c, s, o, n, **k))
    monkeypatch.setenv("GCMF_BANK_ENTRIES", str(bound))
    got = host(bank.apply(x))
    assert bank.last_route == "bank"
    assert calls == ([(1, 3)] * 5 if bound == 4 else [(1, 2), (1, 1)] * 5), calls
    assert np.array_equal(got, whole, equal_nan=True)
    assert np.array_equal(got, loop_of(bank, x), equal_nan=True)


def test_entries_keep_their_place_in_one_call_of_several_polynomials():
    """ent0 = 0 and nfield = 3: entry e of the band is polynomial e // 3 on field e % 3 (the C ABI directly, against gcmf_apply per entry)."""
    import torch
    shape = SMALL
    plan = plan_of(KIND, shape)
    bank = make_bank(KIND, shape, 14, FIVE)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    c = 2 / bank.filter_specs[0].s_max
    f = torch.from_numpy(field_for(shape, 735, (3,))).cuda()
    out = torch.empty((5, 3) + shape, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    plan.apply_bank(P, c, f.data_ptr(), out.data_ptr(), 3, stream=stream)
    one = torch.empty(shape, dtype=torch.float64, device="cuda")
    for j in range(5):
        for i in range(3):
            plan.apply(P[j], c, [f[i].data_ptr()], [one.data_ptr()], 1, device_ptrs=True, stream=stream)
            assert np.array_equal(out[j, i].cpu().numpy(), one.cpu().numpy(), equal_nan=True), (j, i)


# ---- 6. non-finite values in the band ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
def test_nan_in_the_band(shape):
    """A NaN in a wet cell of the top row, one beside the mirror image of that column (the fold's other side), one just below the band of
    an eight-level launch: NaN exactly there, finite neighbours, the bits of the loop, the oracle's values."""
    import torch
    n_steps = 24
    ny, nx = shape
    gv = grid_vars(KIND, shape)
    bank = make_bank(KIND, shape, n_steps)
    f = field_for(shape, 720, (2,))
    a, b, below = (ny - 1, 20), (ny - 1, nx - 1 - 20 + 1), (ny - 9, 3 * nx // 4)
    for j, i in (a, b, below):
        assert gv["wet_mask"][j, i] == 1
        f[1, j, i] = np.nan
    x = torch.from_numpy(f).cuda()
    got = bank.apply(x).cpu().numpy()
    assert bank.last_route == "bank"
    want = loop_of(bank, x)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    nan = np.isnan(got[:, 1])
    expect = np.zeros(shape, dtype=bool)
    expect[0, :] = True                                 # (field_for: NaN on the land row)
    for j, i in (a, b, below):
        expect[j, i] = True
    assert (nan == expect[None]).all()
    for j, i in (a, b, below):
        assert np.isfinite(got[:, 1, j - 1, i]).all() and np.isfinite(got[:, 1, j, i - 1]).all() and np.isfinite(got[:, 1, j, i + 1]).all()
    assert np.isfinite(got[:, 1, ny - 1, nx - 1 - 20]).all()      # the fold partner of `a`
    assert np.isfinite(got[:, 0, 1:, :]).all()                    # the other field of the call
    check(got, oracle_of(bank, KIND, f, gv), ("non-finite values in the band", shape))


# ---- 7. land on the seam, finite values on land -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fold_grid(shape):
    gv = dict(T.scalar_grid_vars(KIND, shape))
    gv["wet_mask"] = T.coastline("fold", shape, seed=5, tripolar=True)
    return gv


@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
def test_land_on_the_seam(shape):
    ny = shape[0]
    gv = fold_grid(shape)
    bank = make_bank(KIND, shape, 24, gv=gv)
    plan = plan_of(KIND, shape, gv)
    assert plan.bank_cut(24, 6) == [8, 8, 8]
    f = np.stack([T.random_field(shape, 780 + k) for k in range(2)])       # finite everywhere, land included
    got = bank.apply(f)
    assert bank.last_route == "bank" and np.isfinite(got).all()
    land = gv["wet_mask"] == 0
    assert land[ny - 1].sum() >= 7 and land[ny - 8:].sum() >= 20 and land[: ny - 8].sum() >= shape[1]
    want = oracle_of(bank, KIND, f, gv)
    check(got, want, ("land on the seam", shape))
    check(got[:, :, land], want[:, :, land], ("land on the seam: the land cells' own polynomial", shape))
    for j in range(1, 3):
        assert not np.array_equal(got[j][:, land], got[0][:, land]), j
    assert np.array_equal(got, loop_of(bank, f), equal_nan=True)


# ---- the shortest grid ---------------------------------------------------------------------------------------------------------------------
def test_the_shortest_grid():
    """rows >= 3 S + 2 on the seam's plan (multi_supported): found from bank_cut, not written down here."""
    nx, n_steps = 64, 24
    shortest = None
    for ny in range(16, 48):
        if plan_of(KIND, (ny, nx)).bank_cut(n_steps, 3):
            shortest = ny
            break
    assert shortest is not None and shortest > 16
    for ny, route in ((shortest, "bank"), (shortest - 1, "loop")):
        shape = (ny, nx)
        plan = plan_of(KIND, shape)
        cut = plan.bank_cut(n_steps, 3)
        assert bool(cut) == (route == "bank"), (ny, cut)
        bank = make_bank(KIND, shape, n_steps)
        f = field_for(shape, 790, (2,))
        got = bank.apply(f)
        assert bank.last_route == route, (ny, bank.last_route)
        if cut:
            assert sum(cut) == n_steps and all(5 <= s <= 8 for s in cut) and plan.last_timing()[1] == band_launches(cut)
        assert np.array_equal(got, loop_of(bank, f), equal_nan=True)
        check(got, oracle_of(bank, KIND, f, grid_vars(KIND, shape)), ("the shortest grid", shape, route))


# ---- 8. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_c_abi(monkeypatch):
    import torch
    shape = BLOCKED          # (wide enough for the lone field's zipped fold strips)
    ny, nx = shape
    gv = grid_vars(KIND, shape)
    plan = plan_of(KIND, shape)
    bank = make_bank(KIND, shape, 63)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    c = 2 / bank.filter_specs[0].s_max
    f = torch.from_numpy(field_for(shape, 750, (2,))).cuda()
    out = torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda")
    src, dst = f.data_ptr(), out.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    before = torch.empty(shape, dtype=torch.float64, device="cuda")
    plan.last_kernel()
    plan.apply(P[1], c, [f[0].data_ptr()], [before.data_ptr()], 1, device_ptrs=True, stream=stream)
    lone_kernel, lone_cut = plan.last_kernel(), plan.clenshaw_cut(63, 1)
    assert lone_kernel.startswith("gcmf::k_ringcz<double, ") and sum(lone_cut) == 63, (lone_kernel, lone_cut)     # the zipped fold strips

    def refused(pl, why, *a, status=_lib.ERR_UNSUPPORTED, **k):
        st, msg = _status(pl.apply_bank, *a, **k)
        assert st == status and "gcmf_apply_bank" in msg and why in msg, (why, st, msg)

    gt = GridType[KIND].value
    f32 = _lib.Plan(gt, _lib.F32, ny, nx, _planes(KIND, gv, "f4"))
    refused(f32, "an f32 plan", P, c, src, dst, 2)
    assert f32.bank_cut(63, 6) == []
    f32.close()
    slab = _lib.Plan(gt, _lib.F64, ny, nx, _planes(KIND, gv), row_begin=ny // 2, row_end=ny, halo=9)
    refused(slab, "a row slab", P, c, src, dst, 2)
    assert slab.bank_cut(63, 6) == []
    slab.close()
    # (GCMF_PLAN_SELF_RING: a tripolar grid never gets such a plan -- the refusal is gcmf_plan_create's)
    st, msg = _status(_lib.Plan, gt, _lib.F64, ny, nx, _planes(KIND, gv), self_ring=True, halo=9)
    assert st != _lib.OK and "GCMF_PLAN_SELF_RING" in msg, (st, msg)
    refused(plan, "host pointers", P, c, src, dst, 2, device_ptrs=False)
    for flag, name in [(_lib.FORWARD_RECURRENCE, "GCMF_FORWARD_RECURRENCE"), (_lib.MASK_FROM_NAN, "GCMF_MASK_FROM_NAN"),
                       (_lib.FACES_FROM_NAN, "GCMF_FACES_FROM_NAN"), (_lib.OUT_F32, "GCMF_OUT_F32")]:
        refused(plan, name, P, c, src, dst, 2, flags=flag)
    cut = plan.bank_cut(63, 6)
    assert plan.bank_cut(4, 6) == [] and sum(cut) == 63 and max(cut) == 8 and min(cut) >= 5, cut
    assert plan.bank_cut(9, 6) == []                    # (nine steps are one nine-level launch or none)
    refused(plan, "fewer than five steps", P[:, :5], c, src, dst, 2)
    monkeypatch.setenv("GCMF_CLENSHAW", "0")
    off = _lib.Plan(gt, _lib.F64, ny, nx, _planes(KIND, gv))
    monkeypatch.delenv("GCMF_CLENSHAW")
    assert off.bank_cut(63, 6) == []
    refused(off, "GCMF_CLENSHAW=0", P, c, src, dst, 2)
    off.close()
    torch.cuda.synchronize()
    # a real bank call, then gcmf_apply on the same plan: its usual path and the bits it gave before
    plan.apply_bank(P, c, src, dst, 2, stream=stream)
    assert plan.last_path() == "strips" and plan.last_timing()[1] == band_launches(cut)
    assert plan.last_kernel_geometry()["bank"] == 3
    assert plan.bank_cut(63, 6) == cut and plan.clenshaw_cut(63, 1) == lone_cut
    after = torch.empty(shape, dtype=torch.float64, device="cuda")
    plan.last_kernel()
    plan.apply(P[1], c, [f[0].data_ptr()], [after.data_ptr()], 1, device_ptrs=True, stream=stream)
    assert "bank" not in plan.last_kernel_geometry() and plan.last_kernel() == lone_kernel
    assert np.array_equal(before.cpu().numpy(), after.cpu().numpy(), equal_nan=True)
    assert np.array_equal(out[1, 0].cpu().numpy(), after.cpu().numpy(), equal_nan=True)


def test_nx_no_multiple_of_four_with_land_has_no_bank():
    import torch
    odd = (96, 162)
    godd = T.scalar_grid_vars(KIND, odd)
    podd = _lib.Plan(GridType[KIND].value, _lib.F64, odd[0], odd[1], _planes(KIND, godd))
    assert (godd["wet_mask"] == 0).any() and podd.bank_cut(24, 6) == []
    bank = make_bank(KIND, SMALL, 24)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    fo = torch.zeros((2,) + odd, dtype=torch.float64, device="cuda")
    oo = torch.empty((3, 2) + odd, dtype=torch.float64, device="cuda")
    st, msg = _status(podd.apply_bank, P, 2 / bank.filter_specs[0].s_max, fo.data_ptr(), oo.data_ptr(), 2)
    assert st == _lib.ERR_UNSUPPORTED and "gcmf_apply_bank" in msg and "not a multiple of 4" in msg, (st, msg)
    podd.close()


# ---- 9. the switch --------------------------------------------------------------------------------------------------------------------------
def test_the_switch(monkeypatch):
    shape = SMALL
    f = field_for(shape, 760, (2,))
    bank = make_bank(KIND, shape, 24)
    fast = bank.apply(f)
    assert bank.last_route == "bank"                    # GCMF_FILTER_BANK=1 (the fixture)
    monkeypatch.setenv("GCMF_FILTER_BANK", "0")
    slow = bank.apply(f)
    assert bank.last_route == "loop"
    assert np.array_equal(fast, slow, equal_nan=True)
    monkeypatch.delenv("GCMF_FILTER_BANK")
    dflt = bank.apply(f)
    assert bank.last_route == ("bank" if _bank_by_default(3, shape[0], shape[1], GridType[KIND]) else "loop")
    assert np.array_equal(fast, dflt, equal_nan=True)
    # the seamless kinds keep their default
    assert _bank_by_default(3, shape[0], shape[1], GridType.IRREGULAR_WITH_LAND) and _bank_by_default(3, shape[0], shape[1])
    # the measured default: the bank from the 1-degree POP grid with two scales up to 32 scales at 2400 x 3600, the loop outside
    pop = GridType[KIND]
    assert not _bank_by_default(3, 96, 160, pop) and not _bank_by_default(2, 384, 319, pop) and not _bank_by_default(33, 2400, 3600, pop)
    assert _bank_by_default(2, 384, 320, pop) and _bank_by_default(8, 1080, 1440, pop) and _bank_by_default(32, 2400, 3600, pop)
    shape = (384, 320)
    f = field_for(shape, 765)
    bank = make_bank(KIND, shape, 24)
    got = bank.apply(f)
    assert bank.last_route == "bank"
    assert np.array_equal(got, loop_of(bank, f), equal_nan=True)
