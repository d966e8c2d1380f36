"""The table march of k_ringcz keeps its rows as running 32-bit byte offsets (round 9, ringc_march<XO> in csrc/gcmf_ringc_impl.hpp): the
cursor's row offset moves by one row per phase and wraps by compare-and-select, a lane's address is a uniform plane base plus one 32-bit
offset per row, the store rows trail the cursor as one more running offset.  The arithmetic is untouched, so -- the method of
tests/test_gpu_wet_tight.py -- every case runs option "wet_rows" 4 (the tight table whenever eligible) against option 0 (the even cut, whose
kernels are the instruction stream they were) on ONE plan and compares with ``==`` and identical NaN patterns; ``units=`` / ``xoff=`` in
``last_kernel_geometry()`` show that the table ran; one case per mask is also held to the oracle at 1e-12.

Where the new addressing can go wrong, and the smallest shapes that get there (97 x 236 and 192 x 432):

  * launches of every depth 5 .. 9, each cut with a first, a later and a last launch: 27 steps as 9 + 9 + 9, and under option "ringc_smax"
    8, 7 and 6: 23 as 8 + 8 + 7, 20 as 7 + 7 + 6, 17 as 6 + 6 + 5 (asserted through ``clenshaw_cut``; on grids this small the default
    policy prices a launch by the rows it marches and cuts 63, 24, 14 and 20 steps into eights, eights, 7 + 7 and 7 + 7 + 6 -- those
    polynomials run as well, with whatever cut the plan gives them);
  * wet runs that touch row 0 and row ny - 1 of the y-periodic grid (`ends`, `open_south`): ghost rows and the cursor wrap inside a ring
    period, in the strip that marches up the grid and in the one that marches down;
  * a window across the x seam under a shifted window grid, xoff != 0 (`seam`, and the fixture mask at 97 x 236);
  * runs of exactly four rows (`lakes`): strips of two rows, a march of twelve -- it leaves inside the peeled period, whole-period form;
  * strips of three rows at nine levels: a march of 13 rows, one more than a ring period -- the early-exit form by default, the
    whole-period form under option "ringc_zip" 3 (one trip through the main loop after the peeled period);
  * a NaN and an inf in wet cells: the workgroup's redo march (nan_to_num) through the same addressing, counted by ``ring_fallbacks()``;
  * NaN on all land and no strip redone (``gcmf_plan::pool_clean`` holds: cells no pair owns are read as ghost cells).

Closed ends: no plan takes a table on a grid that does not wrap in y -- gcmf_apply offers the table to whole grids without a tripole fold
only (``wet_now``, csrc/gcmf_api.hip), which wrap, MOM5U / MOM5T included; row slabs and tripolar plans keep the even cut.  The march
therefore has no closed-end form, the launcher's predicate (``table_rows_ok``, tests/test_table_rows_predicate.py) refuses such a grid,
and there is no such case here.  Long marches (60-row strips, six ring periods) are tests/test_gpu_wet_tight.py's full-size case."""
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O
from tests.wet_tight_model import model

pytestmark = pytest.mark.gpu

GRID = "IRREGULAR_WITH_LAND"
BIG, SMALL = (192, 432), (97, 236)
DEFAULT = 3
STEPS = (63, 24, 14, 20)                              # the default policy's cuts
FORCED = ((27, 0, [9, 9, 9]), (23, 8, [8, 8, 7]), (20, 7, [7, 7, 6]), (17, 6, [6, 6, 5]))     # (n_steps, "ringc_smax", the cut)


def ends_mask(shape):
    """All land but a band that touches row 0, one that touches row ny - 1 (runs are not joined across the y wrap) and a block of five rows."""
    ny, nx = shape
    m = np.zeros(shape)
    m[0:7, 20:200] = 1
    m[ny - 6 : ny, 40:220] = 1
    m[ny // 2 : ny // 2 + 5, 60:90] = 1
    return m


def seam_mask(shape):
    """An ocean across the x seam (the last 25 and the first 31 columns) and a block of five rows: the planner shifts the window grid."""
    ny, nx = shape
    m = np.zeros(shape)
    m[10 : ny - 10, nx - 25 :] = 1
    m[10 : ny - 10, :31] = 1
    m[30:35, 100:140] = 1
    return m


def _mask(name, shape):
    if name == "fixture":
        return T.land_mask(shape)
    if name == "ends":
        return ends_mask(shape)
    if name == "seam":
        return seam_mask(shape)
    return T.coastline(name, shape, seed=7)


_CASES, _WANT = {}, {}


def _case(name, shape, n_steps):
    key = (name, shape, n_steps)
    if key not in _CASES:
        f, gv = T.scalar_case(GRID, shape)
        wet = _mask(name, shape)
        gv = dict(gv, wet_mask=wet)
        dx = T.grid_dx_min(GRID, gv) if O.DIMENSIONAL[GRID] else 1.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=n_steps, filter_shape=FilterShape.TAPER, grid_type=GridType[GRID], grid_vars=gv)
        plan = ALL_KERNELS[GridType[GRID]](**gv)._plan(_lib.F64, shape)
        _CASES[key] = (flt, plan, f, wet, gv)
    return _CASES[key]


def _oracle(key, flt, f, gv):
    if key not in _WANT:
        fs = flt.filter_spec
        with np.errstate(all="ignore"):
            _WANT[key] = O.filter_func(O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq), GRID, f, gv)
    return _WANT[key]


def _ab(flt, plan, f, zip_opt=None, smax=0):
    """The filter under "wet_rows" 0 and 4: results, (kernel, geometry) of the deepest launch, strips redone."""
    outs, ran, redone = [], [], []
    try:
        plan.set_option("ringc_smax", smax)
        if zip_opt is not None:
            plan.set_option("ringc_zip", zip_opt)
        for opt in (0, 4):
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
        if zip_opt is not None:
            plan.set_option("ringc_zip", 1)
    return outs, ran, redone


def _cut(plan, n_steps, smax=0):
    try:
        plan.set_option("ringc_smax", smax)
        return list(plan.clenshaw_cut(n_steps))
    finally:
        plan.set_option("ringc_smax", 0)


def _check(name, shape, n_steps, how="nan", oracle=False, zip_opt=None, xe=None, smax=0):
    flt, plan, f0, wet, gv = _case(name, shape, n_steps)
    f = T.treat_land(f0, wet, how, seed=3)
    cut = _cut(plan, n_steps, smax)
    assert cut and sum(cut) == n_steps and all(5 <= d <= 9 for d in cut), cut
    S = max(cut)
    outs, ran, redone = _ab(flt, plan, f, zip_opt, smax)
    want = model(wet, S)
    assert f"k_ringcz<double, {S}, " in ran[0][0] and "units" not in ran[0][1] and "xoff" not in ran[0][1], ran
    assert f"k_ringcz<double, {S}, " in ran[1][0] and ran[1][0].endswith(", true>"), ran
    g = ran[1][1]
    assert (g.get("units"), g["H"], g["nstrips"], g.get("xoff")) == want[:4], (ran, want)
    if xe is not None:      # (k_ringcz<double, S, FIRST, XE, true>)
        assert ran[1][0].endswith(f", {'true' if xe else 'false'}, true>"), ran
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    if how != "mixed":      # (mixed puts NaN into wet cells)
        assert redone == [0, 0], redone
    if oracle:
        ref = _oracle((name, shape, n_steps, how), flt, f, gv)
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(outs[1]), np.isnan(ref))
        assert ok.any() and np.abs(outs[1][ok] - ref[ok]).max() <= 1e-12 * np.abs(ref[ok]).max()
    return cut, want, ran


@pytest.mark.parametrize("n_steps,smax,cut", FORCED)
@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_fixture_mask_at_every_depth(shape, n_steps, smax, cut):
    """testing.land_mask under cuts that hold launches of nine, eight, seven, six and five levels, each with a first, a later and a last
    launch; at 97 x 236 with nine levels and at 192 x 432 with eight the planner shifts the window grid."""
    assert {d for _, _, c in FORCED for d in c} == {5, 6, 7, 8, 9} and all(len(c) == 3 for _, _, c in FORCED)
    got, want, _ = _check("fixture", shape, n_steps, oracle=(n_steps == 20), smax=smax)
    assert got == cut, (got, cut)
    if (shape, max(cut)) in ((SMALL, 9), (BIG, 8)):
        assert want[3] != 0, want


@pytest.mark.parametrize("n_steps", STEPS)
def test_fixture_mask_under_the_default_cuts(n_steps):
    """63, 24, 14 and 20 steps with the cut the plan's own policy gives them at 97 x 236."""
    cut, _, _ = _check("fixture", SMALL, n_steps)
    assert len(cut) >= 2, cut


@pytest.mark.parametrize("n_steps", [18, 20])
@pytest.mark.parametrize("name,shape", [("ends", SMALL), ("ends", BIG), ("open_south", SMALL)])
def test_runs_that_touch_the_y_seam(name, shape, n_steps):
    """The strips next to row 0 march up the grid through rows ny - 1, ny - 2, .. as ghost rows, those next to row ny - 1 down through rows
    0, 1, ..: the running row offset wraps inside a ring period, in both directions."""
    wet = _mask(name, shape)
    need = (wet == 1).any(axis=1)
    assert need[0] and need[-1]
    _check(name, shape, n_steps, oracle=(n_steps == 18 and shape == SMALL))


@pytest.mark.parametrize("how", ["nan", "finite"])
@pytest.mark.parametrize("shape", [SMALL, BIG])
def test_a_window_across_the_x_seam_of_a_shifted_grid(shape, how):
    cut, want, _ = _check("seam", shape, 18, how=how, oracle=(how == "nan" and shape == SMALL))
    assert want[3] != 0 and want[1] == 3, want


def test_runs_of_four_rows_leave_inside_the_peeled_period():
    """`lakes`: every run is one pair of two strips of two rows -- a march of twelve rows, the whole-period form."""
    cut, want, _ = _check("lakes", BIG, 18, oracle=True, xe=False)
    assert want[1] == 2 and want[4] == 12, want


@pytest.mark.parametrize("zip_opt,xe", [(None, True), (3, False)])
def test_a_march_one_row_longer_than_a_period(zip_opt, xe):
    """Strips of three rows at nine levels march 3 + 9 + 1 = 13 rows: the early-exit form leaves after row 16, the whole-period form (option
    "ringc_zip" 3: never exits) after one trip through the main loop."""
    cut, want, _ = _check("seam", BIG, 18, zip_opt=zip_opt, xe=xe)
    assert cut == [9, 9] and want[1] == 3, (cut, want)


@pytest.mark.parametrize("name,shape", [("ends", SMALL), ("fixture", SMALL)])
def test_redo_march_through_the_new_addressing(name, shape):
    """A NaN and an inf in wet cells (at the y seam for `ends`): the workgroups that meet them redo their strips with nan_to_num -- the SAME
    march, from the table -- and give the bits of the even cut; NaN on all land alone sends no strip there (asserted in _check)."""
    flt, plan, f0, wet, gv = _case(name, shape, 18)
    _check(name, shape, 18, how="nan")
    f = T.treat_land(f0, wet, "nan")
    jj, ii = np.nonzero(wet)
    first, last = (jj[0], ii[0]), (jj[-1], ii[-1])
    f[first] = np.nan
    f[last] = np.inf
    outs, ran, redone = _ab(flt, plan, f)
    assert "units" not in ran[0][1] and "units" in ran[1][1], ran
    assert redone[0] > 0 and redone[1] > 0, redone
    assert np.array_equal(outs[0], outs[1], equal_nan=True), ran
    assert np.isnan(outs[1][first]) and not np.isnan(outs[1][wet == 1]).all()
