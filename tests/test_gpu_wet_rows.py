"""k_ringcz with its strips cut from the WET ROWS of each window (round 7, csrc/gcmf_ringc_zip.hip: wet_table; option "wet_rows").

A (window, strip) tile whose 128 columns hold only isolated cells marches for nothing: the table of a launch leaves such rows out and
hands their wave slots to the rest.  The march is untouched, so every cell a pair owns gets the bits of the even cut; the cells no pair
owns are isolated and get their result from k_land_fix.  The one permitted difference is the sign of an exact zero, so results are compared
with ``==`` and identical NaN patterns (``np.array_equal(..., equal_nan=True)``), never as integer views.

Each case runs option 2 (whenever eligible) against option 0 (never) on one plan, asserts through ``last_kernel_geometry()`` -- the table
path appends ``units=<pairs>`` (``Plan.last_wet_units()``) -- that the table ran with the number of pairs ``model()`` below gives, or that it
was refused where it has to be (``model()`` restates the launcher's cut in numpy: it pins the geometry, the values rest on ``==`` and the oracle); one treatment of the values on land per mask is also held to the oracle at 1e-12.

Shapes: 192 x 432 (four windows of 108 columns at nine levels) and 97 x 236; n_steps 18 (a first and a later launch of nine levels) and,
for the 112-column windows, 23 as 8 + 8 + 7 (option "ringc_smax" 8)."""
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O

pytestmark = pytest.mark.gpu

GRID = "IRREGULAR_WITH_LAND"
BIG, SMALL = (192, 432), (97, 236)


def model(wet, S):
    """(pairs, tallest strip, twice the most pairs of a window) of the table of a launch of S levels: wet_table's rules (csrc/gcmf_ringc_zip.hip)
    restated in numpy on the wet mask (kappa = 1, periodic in x and y: a cell exchanges with a neighbour iff it is wet and one of its four
    neighbours is).  Not an independent derivation: it pins the geometry a mask must give, so that a change of the cut shows."""
    ny, nx = wet.shape
    opened = (wet == 1) & ~T.closed_in_cells(wet)
    M = 2 * ((S + 1) // 2)
    WI = 128 - 2 * M
    runs = []
    for wx in range((nx + WI - 1) // WI):
        need = opened[:, (wx * WI - M + np.arange(128)) % nx].any(axis=1)
        own = np.zeros(ny, bool)
        for d in range(-(S + 1), S + 2):
            own |= np.roll(need, d)
        r = 0
        while r < ny:
            if not own[r]:
                r += 1
                continue
            e = r
            while e < ny and own[e]:
                e += 1
            runs.append((wx, e - r))
            r = e
    pairs = lambda n, H: max(1, min(n // 4, -(-n // (2 * H))))
    H = 2
    while sum(pairs(n, H) for _, n in runs) > 512:
        H += 1
    per_window, tallest = {}, 0
    for wx, n in runs:
        k = pairs(n, H)
        per_window[wx] = per_window.get(wx, 0) + k
        for p in range(k):
            lo, hi = p * n // k, (p + 1) * n // k
            tallest = max(tallest, (hi - lo) // 2, (hi - lo) - (hi - lo) // 2)
    return sum(per_window.values()), tallest, 2 * max(per_window.values(), default=0)


_CASES = {}


def _case(mask_name, shape, n_steps):
    """Filter, plan, field (finite everywhere) and wet mask of one (mask, shape, n_steps); built once per session."""
    key = (mask_name, shape, n_steps)
    if key not in _CASES:
        f, gv = T.scalar_case(GRID, shape)
        if mask_name == "fixture":
            wet = T.land_mask(shape)
        elif mask_name == "band":
            # a band of land through the middle of the grid and a 1 x 2 lake inside it, in the footprint of window 1 only (one wet cell
            # closed in by land would be isolated itself and need no row): ONE row with anything wet, a run of 2 S + 3 rows
            ny, nx = shape
            wet = np.ones(shape)
            wet[ny // 2 - 36 : ny // 2 + 36, :] = 0
            wet[ny // 2, 150:152] = 1
        else:
            wet = T.coastline(mask_name, shape, seed=7)
        gv = dict(gv, wet_mask=wet)
        dx = T.grid_dx_min(GRID, gv) if O.DIMENSIONAL[GRID] else 1.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=n_steps, filter_shape=FilterShape.TAPER, grid_type=GridType[GRID], grid_vars=gv)
        plan = ALL_KERNELS[GridType[GRID]](**gv)._plan(_lib.F64, shape)
        _CASES[key] = (flt, plan, f, wet, gv)
    return _CASES[key]


_WANT = {}


def _oracle(key, flt, f, gv):
    if key not in _WANT:
        fs = flt.filter_spec
        with np.errstate(all="ignore"):
            _WANT[key] = O.filter_func(O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq), GRID, f, gv)
    return _WANT[key]


def _ab(flt, plan, f, options=(0, 2), smax=0):
    """The filter under each value of "wet_rows": results, and (kernel, geometry) of the deepest launch."""
    outs, ran = [], []
    try:
        plan.set_option("ringc_smax", smax)
        for opt in options:
            plan.set_option("wet_rows", opt)
            plan.last_kernel()
            with np.errstate(all="ignore"):
                outs.append(flt.apply(f))
            ran.append((plan.last_kernel(), plan.last_kernel_geometry()))
    finally:
        plan.set_option("wet_rows", 1)
        plan.set_option("ringc_smax", 0)
    return outs, ran


def _check(mask_name, shape, n_steps, how, smax=0, oracle=False):
    flt, plan, f0, wet, gv = _case(mask_name, shape, n_steps)
    f = T.treat_land(f0, wet, how, seed=3)
    S = 8 if smax == 8 else 9
    assert plan.clenshaw_cut(n_steps) == [9] * (n_steps // 9), plan.clenshaw_cut(n_steps)
    outs, ran = _ab(flt, plan, f, smax=smax)
    units, tallest, nstrips = model(wet, S)
    assert f"k_ringcz<double, {S}, " in ran[0][0] and "units" not in ran[0][1], ran
    assert f"k_ringcz<double, {S}, " in ran[1][0], ran
    g = ran[1][1]
    assert (g.get("units"), g["H"], g["nstrips"]) == (units, tallest, nstrips), (ran, units, tallest, nstrips)
    assert g["nstrips"] % 2 == 0 and g["grid"] == f"{(units + 1) // 2}x1", ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    if oracle:
        want = _oracle((mask_name, shape, n_steps, how), flt, f, gv)
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(outs[1]), np.isnan(want))
        if ok.any():
            assert np.abs(outs[1][ok] - want[ok]).max() <= 1e-12 * np.abs(want[ok]).max()
    return plan, f, ran


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
def test_fixture_mask(how):
    """testing.land_mask at 192 x 432: the ghost columns of windows 0 and 1 reach across the quadrant's edges (the x seam, column 216),
    so every window keeps all its rows here -- the table is the even cut's rows in another order; the quadrant leaves rows out only at
    sizes where whole windows fit inside it (test_policy_takes_the_table_at_baseline_size)."""
    _check("fixture", BIG, 18, how, oracle=(how == "nan"))


def test_fixture_mask_where_windows_fit_inside_the_quadrant():
    """testing.land_mask at 1440 x 2880: windows 1 .. 12 of 27 lie inside the land quadrant and keep only the northern half of their rows
    (and, across the y wrap, rows 0 .. 9), so the table leaves rows out and its strips are shorter than the even cut's (32 rows against
    40).  No oracle at this size: the even cut on the same plan is the reference."""
    shape = (1440, 2880)
    flt, plan, f0, wet, gv = _case("fixture", shape, 18)
    units, tallest, nstrips = model(wet, 9)
    assert (units, tallest, nstrips) == (501, 32, 46)
    outs, ran = _ab(flt, plan, T.treat_land(f0, wet, "mixed", seed=3))
    assert "k_ringcz<double, 9, " in ran[0][0] and (ran[0][1]["H"], ran[0][1]["nstrips"]) == (40, 36) and "units" not in ran[0][1], ran
    assert "k_ringcz<double, 9, " in ran[1][0] and (ran[1][1]["H"], ran[1][1]["nstrips"], ran[1][1].get("units")) == (tallest, nstrips, units), ran
    assert plan.last_wet_units() == units
    assert np.array_equal(outs[0], outs[1], equal_nan=True)


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
@pytest.mark.parametrize("shape,n_steps,smax", [(BIG, 18, 0), (SMALL, 18, 0), (SMALL, 23, 8)])
@pytest.mark.parametrize("name", ["lakes", "all_land", "on_the_cuts", "one_land_cell", "speckle"])
def test_coastlines(name, shape, n_steps, smax, how):
    """`lakes`: short runs, a lake across the x seam and one across the y seam; `all_land`: no pair at all, the whole result is
    k_land_fix's; `one_land_cell` and `speckle` leave no row out, and the policy of option 1 keeps the even cut there."""
    if n_steps == 23:
        flt, plan, f0, wet, gv = _case(name, shape, n_steps)
        try:
            plan.set_option("ringc_smax", 8)
            assert plan.clenshaw_cut(23) == [8, 8, 7]
        finally:
            plan.set_option("ringc_smax", 0)
        f = T.treat_land(f0, wet, how, seed=3)
        outs, ran = _ab(flt, plan, f, smax=8)
        units, tallest, nstrips = model(wet, 8)
        g = ran[1][1]
        assert "k_ringcz<double, 8, " in ran[0][0] and "units" not in ran[0][1], ran
        assert "k_ringcz<double, 8, " in ran[1][0] and (g.get("units"), g["H"], g["nstrips"]) == (units, tallest, nstrips), (ran, units, tallest, nstrips)
        assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    else:
        # (all_land with NaN on all land has no finite cell: the oracle is held on finite values there)
        plan, f, ran = _check(name, shape, n_steps, how, oracle=(how == ("finite" if name == "all_land" else "nan")))
        flt = _case(name, shape, n_steps)[0]
        if name == "all_land":
            assert ran[1][1]["units"] == 0, ran
        if name in ("one_land_cell", "speckle"):
            outs, ran1 = _ab(flt, plan, f, options=(1,))
            assert "k_ringcz<double, 9, " in ran1[0][0] and "units" not in ran1[0][1], ran1


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
def test_land_band_with_a_lake(how):
    """A run of 2 S + 3 = 21 rows in window 1 only, between the two runs every window has."""
    flt, plan, f0, wet, gv = _case("band", BIG, 18)
    with_lake, _, _ = model(wet, 9)
    dry = wet.copy()
    dry[BIG[0] // 2, 150:152] = 0
    assert with_lake == model(dry, 9)[0] + 21 // 4      # (strips of two rows on a grid this small: five pairs for the lake's run)
    _check("band", BIG, 18, how, oracle=(how == "nan"))


def test_redo_pass_next_to_a_runs_end():
    """A NaN and an inf in wet cells on the last rows before the band (the ends of two runs): the workgroups that meet them redo their
    march with nan_to_num -- from the table, with the bits of the even cut."""
    flt, plan, f0, wet, gv = _case("band", BIG, 18)
    f = T.treat_land(f0, wet, "nan")
    ny = BIG[0]
    f[ny // 2 - 37, 150] = np.nan
    f[ny // 2 + 36, 160] = np.inf
    assert wet[ny // 2 - 37, 150] == 1 and wet[ny // 2 + 36, 160] == 1 and wet[ny // 2 - 36, 150] == 0 and wet[ny // 2 + 35, 160] == 0
    outs, ran, redone = [], [], []
    for opt in (0, 2):    # (the counter of redone strips read and reset per option: the table's own pairs must take the redo)
        plan.ring_fallbacks()
        o, r = _ab(flt, plan, f, options=(opt,))
        outs, ran = outs + o, ran + r
        redone.append(plan.ring_fallbacks())
    assert "units" not in ran[0][1] and ran[1][1].get("units") == model(wet, 9)[0], ran
    assert redone[0] > 0 and redone[1] > 0, redone
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    assert np.isnan(outs[1][ny // 2 - 37, 150]) and not np.isnan(outs[1][wet == 1]).all()


def test_work_planes_are_made_finite_after_another_schedule():
    """gcmf_plan::pool_clean.  The one-launch-per-step schedule (multi_s 1: k_scalar_step, no land fix-up) carries the NaN on land through
    every T_k, and its fbar and staged input lie where the blocked schedules keep their third and fourth state plane: after such a call
    all four planes of the pool hold NaN on land -- in cells no pair owns, which every pair's ghost rows read.  (The blocked forward
    schedule would not do: its first launch takes land as zero.)  The next table launch has to fill the planes first.  Three launches
    of nine levels: the ghost rows lie S + 2 rows from the nearest wet row, so a NaN there needs a third launch to reach one.  Without
    the fill the fast march meets the NaN and every pair next to unowned rows takes the nan_to_num redo (or, where the watch does not
    see it, the NaN reaches wet cells): the result must equal a plan's that never ran anything else AND no strip may have been redone.
    Measured once in a build with the hipMemsetAsync taken out: the values still equal (the redo sanitises the ghost cells), 104 strips
    redone per application -- this test fails there on `redone == 0`."""
    flt, plan, f0, wet, gv = _case("band", BIG, 27)
    assert plan.clenshaw_cut(27) == [9, 9, 9]
    f = T.treat_land(f0, wet, "nan")
    gv2 = {k: np.array(v, copy=True) for k, v in gv.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fresh = Filter(filter_scale=flt.filter_scale, dx_min=flt.dx_min, n_steps=27, filter_shape=FilterShape.TAPER, grid_type=GridType[GRID], grid_vars=gv2)
    plan2 = ALL_KERNELS[GridType[GRID]](**gv2)._plan(_lib.F64, BIG)
    assert plan2 is not plan
    try:
        plan2.set_option("wet_rows", 0)
        with np.errstate(all="ignore"):
            want = fresh.apply(f)
    finally:
        plan2.set_option("wet_rows", 1)
    units = model(wet, 9)[0]
    try:
        plan.set_option("wet_rows", 2)
        for _ in range(2):    # (the second round: the flag was set by a table launch, then cleared again)
            with np.errstate(all="ignore"):
                flt.apply(f)              # the work buffer at its full size (it only grows): the planes stay where they are
            assert plan.last_wet_units() == units
            try:
                plan.set_tuning(multi_s=1)
                plan.last_kernel()
                with np.errstate(all="ignore"):
                    dirty = flt.apply(f)
                assert "k_scalar_step" in plan.last_kernel(), plan.last_kernel()
            finally:
                plan.set_tuning(multi_s=8)
            assert np.isnan(dirty[wet == 0]).all()
            plan.ring_fallbacks()
            plan.last_kernel()
            with np.errstate(all="ignore"):
                got = flt.apply(f)
            redone = plan.ring_fallbacks()
            assert "k_ringcz<double, 9, " in plan.last_kernel() and plan.last_wet_units() == units
            same = np.array_equal(got, want, equal_nan=True)
            assert same and redone == 0, (same, redone)
    finally:
        plan.set_option("wet_rows", 1)


def test_batches_keep_the_even_cut():
    """Batches are not taken: the fields of a batch keep today's launches, whatever the option says."""
    flt, plan, f0, wet, gv = _case("fixture", BIG, 18)
    f = T.treat_land(np.stack([f0 + 0.1 * i for i in range(3)]), wet, "mixed", seed=5)
    outs, ran = _ab(flt, plan, f)
    assert "units" not in ran[0][1] and "units" not in ran[1][1], ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True)


def test_policy_takes_the_table_at_baseline_size():
    """Option 1 (the default) on the fixture mask at 2400 x 3600: windows 1 .. 15 keep rows 1190 .. 2399 and, across the y wrap, rows
    0 .. 9; 507 pairs, the tallest strip 67 rows marching 80 instead of 80 marching 92."""
    shape = (2400, 3600)
    flt, plan, f0, wet, gv = _case("fixture", shape, 18)
    assert model(wet, 9) == (507, 67, 36)
    f = T.treat_land(f0, wet, "nan")
    outs, ran = _ab(flt, plan, f, options=(0, 1))
    assert "k_ringcz<double, 9, " in ran[0][0] and (ran[0][1]["H"], ran[0][1]["nstrips"]) == (80, 30) and "units" not in ran[0][1], ran
    assert "k_ringcz<double, 9, " in ran[1][0] and (ran[1][1]["H"], ran[1][1]["nstrips"], ran[1][1].get("units")) == (67, 36, 507), ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True)
