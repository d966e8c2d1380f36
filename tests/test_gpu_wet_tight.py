"""k_ringcz with the TIGHT cut of its wet-row table (round 8, csrc/gcmf_wet_cut.hpp; option "wet_rows" 3 and 4).

The table of round 7 (tests/test_gpu_wet_rows.py, options 1 and 2) widens every run of needed rows by S + 1 rows, counts a row as needed for
the wet cells of a window's ghost columns and pins the window grid at column 0.  The tight cut owns only the rows that a window's OWNED columns
need and shifts the window grid in x; a cell no pair owns can then be the direct neighbour of a wet cell, in y and in x.  The march is the
one it was, so every cell a pair owns gets the bits of the even cut and the rest is k_land_fix's: results are compared with ``==`` and
identical NaN patterns (the sign of an exact zero next to land may differ), never as integer views.

Each case runs option 4 (whenever eligible) against option 0 on one plan and asserts through ``last_kernel_geometry()`` that the table ran
with the (pairs, tallest strip, nstrips, xoff) that tests/wet_tight_model.py -- the shipped rules restated in numpy -- gives for the mask;
one treatment of the values on land per mask is also held to the oracle at 1e-12.

Shapes: 192 x 432 and 97 x 236; n_steps 18 (a first and a later launch of nine levels) and, for the 112-column windows, 23 as 8 + 8 + 7
(option "ringc_smax" 8).  The model picks a nonzero offset for the fixture mask at 97 x 236 with nine levels and at 192 x 432 with eight."""
import warnings

import numpy as np
import pytest
from numpy.random import PCG64, Generator

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O
from tests.wet_tight_model import model

pytestmark = pytest.mark.gpu

GRID = "IRREGULAR_WITH_LAND"
BIG, SMALL = (192, 432), (97, 236)
DEFAULT = 3


def model_r07(wet, S):
    """(pairs, tallest strip, nstrips) of the table of round 7: the model of tests/test_gpu_wet_rows.py, which pins options 1 and 2."""
    from tests.test_gpu_wet_rows import model as m
    return m(wet, S)


def band_mask(shape):
    """A band of land through the middle of the grid and a 1 x 2 lake inside it: one needed row in one window, padded to a run of four."""
    ny, nx = shape
    wet = np.ones(shape)
    wet[ny // 2 - 36 : ny // 2 + 36, :] = 0
    wet[ny // 2, 150:152] = 1
    return wet


_CASES = {}


def _case(mask_name, shape, n_steps):
    """Filter, plan, field (finite everywhere) and wet mask of one (mask, shape, n_steps); built once per session."""
    key = (mask_name, shape, n_steps)
    if key not in _CASES:
        f, gv = T.scalar_case(GRID, shape)
        if mask_name == "fixture":
            wet = T.land_mask(shape)
        elif mask_name == "band":
            wet = band_mask(shape)
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


def _ab(flt, plan, f, options=(0, 4), smax=0):
    """The filter under each value of "wet_rows": results, (kernel, geometry) of the deepest launch, strips redone."""
    outs, ran, redone = [], [], []
    try:
        plan.set_option("ringc_smax", smax)
        for opt in options:
            plan.set_option("wet_rows", opt)
            plan.last_kernel()
            plan.ring_fallbacks()
            with np.errstate(all="ignore"):
                outs.append(flt.apply(f))
            ran.append((plan.last_kernel(), plan.last_kernel_geometry()))
            redone.append(plan.ring_fallbacks())
    finally:
        plan.set_option("wet_rows", DEFAULT)
        plan.set_option("ringc_smax", 0)
    return outs, ran, redone


def _tight(g):
    return g.get("units"), g["H"], g["nstrips"], g.get("xoff")


def _land(f0, wet, how, seed=3):
    """T.LAND_TREATMENTS, and: `garbage` = finite values of any size on land, `zero` = zeros on land."""
    if how == "garbage":
        rng = Generator(PCG64(seed))
        return np.where(wet == 0, 1e30 * rng.standard_normal(wet.shape), f0)
    if how == "zero":
        return np.where(wet == 0, 0.0, f0)
    return T.treat_land(f0, wet, how, seed=seed)


def _check(mask_name, shape, n_steps, how, smax=0, oracle=False):
    flt, plan, f0, wet, gv = _case(mask_name, shape, n_steps)
    f = _land(f0, wet, how)
    S = 8 if smax == 8 else 9
    try:
        plan.set_option("ringc_smax", smax)
        assert plan.clenshaw_cut(n_steps) == ([8, 8, 7] if smax == 8 else [9] * (n_steps // 9)), plan.clenshaw_cut(n_steps)
    finally:
        plan.set_option("ringc_smax", 0)
    outs, ran, redone = _ab(flt, plan, f, smax=smax)
    want = model(wet, S)
    assert f"k_ringcz<double, {S}, " in ran[0][0] and "units" not in ran[0][1] and "xoff" not in ran[0][1], ran
    assert f"k_ringcz<double, {S}, " in ran[1][0], ran
    g = ran[1][1]
    assert _tight(g) == want[:4], (ran, want)
    assert g["nstrips"] % 2 == 0 and g["grid"] == f"{(want[0] + 1) // 2}x1", ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    if how != "mixed":      # (mixed puts NaN into wet cells)
        assert redone == [0, 0], redone
    if oracle:
        ref = _oracle((mask_name, shape, n_steps, how), flt, f, gv)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(outs[1]), np.isnan(ref))
        if ok.any():
            assert np.abs(outs[1][ok] - ref[ok]).max() <= 1e-12 * np.abs(ref[ok]).max()
    return plan, f, ran, want


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
@pytest.mark.parametrize("shape,n_steps,smax", [(BIG, 18, 0), (SMALL, 18, 0), (BIG, 23, 8)])
def test_fixture_mask(shape, n_steps, smax, how):
    """testing.land_mask: the quadrant's edge at column nx / 2 falls inside a window of the grid pinned at column 0; at 97 x 236 with nine
    levels and at 192 x 432 with eight the planner shifts the grid (unowned columns next to wet ones), at 192 x 432 with nine it does not."""
    _, _, _, want = _check("fixture", shape, n_steps, how, smax=smax, oracle=(how == "nan" and smax == 0))
    if (shape, smax) in ((SMALL, 0), (BIG, 8)):
        assert want[3] != 0, want


@pytest.mark.parametrize("how", ["nan", "garbage", "zero"])
@pytest.mark.parametrize("name,shape", [("fixture", SMALL), ("lakes", BIG), ("band", BIG)])
def test_values_on_land_never_reach_a_wet_cell(name, shape, how):
    """NaN, finite garbage of any size and zeros on land: f is masked by the land bits as it is loaded -- ghost rows and ghost columns
    included, in the first launch too -- so no strip meets a non-finite value (ring_fallbacks() == 0, asserted in _check) and the
    wet cells get the bits of the even cut whatever lies on the unowned cells next to them."""
    _check(name, shape, 18, how, oracle=(how == "zero"))


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
@pytest.mark.parametrize("shape,n_steps,smax", [(BIG, 18, 0), (SMALL, 18, 0), (SMALL, 23, 8)])
@pytest.mark.parametrize("name", ["lakes", "all_land", "on_the_cuts", "one_land_cell", "speckle"])
def test_coastlines(name, shape, n_steps, smax, how):
    """`lakes`: runs of one to three rows padded to four, land one row away, a lake across the x seam and one across the y seam (runs are
    not joined there); `all_land`: no pair at all, the whole result is k_land_fix's; `one_land_cell` and `speckle` leave no row out, and the
    policy of option 3 keeps the even cut there."""
    # (all_land with NaN on all land has no finite cell: the oracle is held on finite values there)
    plan, f, ran, want = _check(name, shape, n_steps, how, smax=smax, oracle=(smax == 0 and how == ("finite" if name == "all_land" else "nan")))
    if name == "all_land":
        assert ran[1][1]["units"] == 0 and ran[1][1]["xoff"] == 0, ran
    if name == "lakes":
        assert want[1] == 2, want       # (every run is one pair of two strips of two rows)
    if name in ("one_land_cell", "speckle") and smax == 0:
        flt = _case(name, shape, n_steps)[0]
        outs, ran3, _ = _ab(flt, plan, f, options=(3,))
        assert "k_ringcz<double, 9, " in ran3[0][0] and "units" not in ran3[0][1], ran3


@pytest.mark.parametrize("how", T.LAND_TREATMENTS)
def test_land_band_with_a_lake(how):
    """The lake's one needed row is a run of four rows in one window (round 7: 2 S + 3 = 21 rows), between the two runs every window has,
    which end AT the band's edges."""
    flt, plan, f0, wet, gv = _case("band", BIG, 18)
    dry = wet.copy()
    dry[BIG[0] // 2, 150:152] = 0
    assert model(wet, 9)[0] == model(dry, 9)[0] + 1
    _check("band", BIG, 18, how, oracle=(how == "nan"))


def test_redo_pass_in_the_last_row_of_a_run():
    """A NaN and an inf in wet cells of the last rows before the band -- the last row of one run and the first row of another, unowned rows
    right behind them: the workgroups that meet them redo their march with nan_to_num, from the table, with the bits of the even cut."""
    flt, plan, f0, wet, gv = _case("band", BIG, 18)
    f = T.treat_land(f0, wet, "nan")
    ny = BIG[0]
    f[ny // 2 - 37, 150] = np.nan
    f[ny // 2 + 36, 160] = np.inf
    assert wet[ny // 2 - 37, 150] == 1 and wet[ny // 2 + 36, 160] == 1 and wet[ny // 2 - 36, 150] == 0 and wet[ny // 2 + 35, 160] == 0
    outs, ran, redone = _ab(flt, plan, f)
    assert "units" not in ran[0][1] and _tight(ran[1][1]) == model(wet, 9)[:4], ran
    assert redone[0] > 0 and redone[1] > 0, redone
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    assert np.isnan(outs[1][ny // 2 - 37, 150]) and not np.isnan(outs[1][wet == 1]).all()


def test_work_planes_are_made_finite_after_another_schedule():
    """gcmf_plan::pool_clean under the tight cut, where an unowned cell is the direct neighbour of a wet one: a NaN left there reaches the
    wet cell in the first level.  As tests/test_gpu_wet_rows.py does: the one-launch-per-step schedule (multi_s 1: k_scalar_step) leaves NaN
    on land in all four planes of the pool; the next table launch has to fill the planes first -- the result must equal a plan's that
    never ran anything else AND no strip may have been redone."""
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
        plan2.set_option("wet_rows", DEFAULT)
    units = model(wet, 9)[0]
    try:
        plan.set_option("wet_rows", 4)
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
        plan.set_option("wet_rows", DEFAULT)


def test_the_table_cache_is_keyed_by_the_cut():
    """Options 1 and 2 on a plan on which option 4 has run give the table of round 7 (its model, tests/test_gpu_wet_rows.py), and option 4
    after them the tight one again; all with the values of the even cut."""
    for name, shape in (("fixture", SMALL), ("band", BIG)):
        flt, plan, f0, wet, gv = _case(name, shape, 18)
        f = T.treat_land(f0, wet, "mixed", seed=3)
        outs, ran, _ = _ab(flt, plan, f, options=(0, 4, 2, 1, 4, 2))
        old, new = model_r07(wet, 9), model(wet, 9)[:4]
        assert old != new[:3]
        assert _tight(ran[1][1]) == new and _tight(ran[4][1]) == new, ran
        assert _tight(ran[2][1]) == old + (None,) and _tight(ran[5][1]) == old + (None,), (ran, old)
        g1 = ran[3][1]      # (option 1: the table of round 7 or, where its policy refuses it, the even cut)
        assert "xoff" not in g1 and ("units" not in g1 or _tight(g1)[:3] == old), ran
        for o in outs[1:]:
            assert np.array_equal(outs[0], o, equal_nan=True), ran


def test_batches_keep_the_even_cut():
    """Batches are not taken: the fields of a batch keep today's launches, whatever the option says."""
    flt, plan, f0, wet, gv = _case("fixture", BIG, 18)
    f = T.treat_land(np.stack([f0 + 0.1 * i for i in range(3)]), wet, "mixed", seed=5)
    outs, ran, _ = _ab(flt, plan, f)
    assert "units" not in ran[0][1] and "units" not in ran[1][1], ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True)


def test_default_policy_takes_the_tight_table_at_baseline_size():
    """The default (option 3) on the fixture mask at 2400 x 3600: 510 pairs, the tallest strip 60 rows marching 72 (round 7: 67 marching
    80; the even cut: 80 marching 92), the window grid shifted by 36 columns."""
    shape = (2400, 3600)
    flt, plan, f0, wet, gv = _case("fixture", shape, 18)
    want = model(wet, 9)
    assert want == (510, 60, 40, 36, 72)
    f = T.treat_land(f0, wet, "nan")
    # (two applications only: a plan that has seen more single-field host calls of this size hands them to the row-block pipeline)
    plan.last_kernel()
    plan.ring_fallbacks()
    with np.errstate(all="ignore"):
        got = flt.apply(f)            # no option set: the plan's default, option 3
    kernel, g = plan.last_kernel(), plan.last_kernel_geometry()
    assert plan.ring_fallbacks() == 0
    assert "k_ringcz<double, 9, " in kernel and _tight(g) == want[:4], (kernel, g)
    assert g["H"] <= 62 and -(-(g["H"] + 10) // 4) * 4 <= 72, g      # (the rows a nine-level table launch marches: H + S + 1, up to its next exit)
    outs, ran, redone = _ab(flt, plan, f, options=(0,))
    assert "k_ringcz<double, 9, " in ran[0][0] and (ran[0][1]["H"], ran[0][1]["nstrips"]) == (80, 30) and "units" not in ran[0][1], ran
    assert redone == [0], redone
    assert np.array_equal(outs[0], got, equal_nan=True)
