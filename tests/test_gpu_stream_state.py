"""Nine-level table launches of k_ringcz may stream their state planes (round 10, ringc_march<NT> in csrc/gcmf_ringc_impl.hpp): the loads
of b_{k+1} / b_{k+2} and the stores of the two new states carry the non-temporal policy, so that on a grid whose launch moves more than the
memory-side cache holds the constant planes stay cached from launch to launch.  Which launches do is the host's decision (option
"stream_state": 0 never, 1 by ``stream_state_ok`` of csrc/gcmf_wet_cut.hpp -- tests/test_stream_predicate.py --, 2 whenever a nine-level
table launch runs); the arithmetic is untouched.  So every case runs option 2 against option 0 on ONE plan (option "wet_rows" 4: the tight
table whenever eligible) and compares with ``==`` and identical NaN patterns; `` nt=1`` behind ``xoff=`` in ``last_kernel_geometry()`` shows
which form ran.

  * 97 x 236 at nine levels, 18 steps (a first and a last launch) and 27 (a later one between them): a first launch streams its stores only,
    a last one writes the result through the same stores;
  * the fixture mask (a shifted window grid, a window across the x seam) and `lakes` (runs of four rows: the march leaves inside the peeled
    period);
  * NaN on land and finite garbage on land, no strip redone;
  * a NaN in a wet cell, and one in the last row of a run: the workgroup's redo march keeps the default policy and gives the same bits;
  * the default (option 1) keeps the default policy on this small grid and streams at 2400 x 3600;
  * the streamed result against the oracle at 1e-12, once."""
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O

pytestmark = pytest.mark.gpu

GRID = "IRREGULAR_WITH_LAND"
SMALL = (97, 236)

_CASES = {}


def _mask(name, shape):
    return T.land_mask(shape) if name == "fixture" else T.coastline(name, shape, seed=7)


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


def _run(flt, plan, f, options, wet_rows=4):
    """The filter under each value of "stream_state": results, (kernel, geometry) of the deepest launch, strips redone."""
    outs, ran, redone = [], [], []
    try:
        plan.set_option("wet_rows", wet_rows)
        for opt in options:
            plan.set_option("stream_state", opt)
            plan.last_kernel()
            plan.ring_fallbacks()
            with np.errstate(all="ignore"):
                outs.append(flt.apply(f))
            ran.append((plan.last_kernel(), plan.last_kernel_geometry()))
            redone.append(plan.ring_fallbacks())
    finally:
        plan.set_option("wet_rows", 3)
        plan.set_option("stream_state", 1)
    return outs, ran, redone


def _table_ran(ran):
    for kernel, g in ran:
        assert "k_ringcz<double, 9, " in kernel and kernel.endswith(", true>") and "units" in g and "xoff" in g, ran


def _same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and bool((a[~np.isnan(a)] == b[~np.isnan(b)]).all())


@pytest.mark.parametrize("how", ["nan", "finite"])
@pytest.mark.parametrize("name", ["fixture", "lakes"])
@pytest.mark.parametrize("n_steps", [18, 27])
def test_streamed_state_gives_the_same_bits(n_steps, name, how):
    flt, plan, f0, wet, gv = _case(name, SMALL, n_steps)
    cut = list(plan.clenshaw_cut(n_steps))
    assert cut == [9] * (n_steps // 9), cut
    f = T.treat_land(f0, wet, how, seed=3)
    outs, ran, redone = _run(flt, plan, f, (0, 2, 1))
    _table_ran(ran)
    assert "nt" not in ran[0][1] and ran[1][1].get("nt") == 1, ran
    assert "nt" not in ran[2][1], ran        # (the default: this grid's launches move far less than the cache holds)
    assert list(ran[1][1])[-2:] == ["xoff", "nt"], ran
    assert {k: v for k, v in ran[1][1].items() if k != "nt"} == ran[0][1] and ran[1][0] == ran[0][0], ran
    assert redone == [0, 0, 0], redone
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), ran
    assert (~np.isnan(outs[1])).any()


@pytest.mark.parametrize("where", ["first", "last_row"])
def test_the_redo_march_keeps_the_default_policy_and_the_bits(where):
    """One NaN in a wet cell -- the first wet cell, or one in the last wet row of the grid, where a run ends: the workgroup that meets it
    marches again through nan_to_num, with default-policy accesses in both forms of the kernel."""
    flt, plan, f0, wet, gv = _case("fixture", SMALL, 27)
    f = T.treat_land(f0, wet, "nan")
    jj, ii = np.nonzero(wet)
    cell = (jj[0], ii[0]) if where == "first" else (jj[-1], ii[-1])
    assert where == "first" or not wet[cell[0] + 1 :].any()
    f[cell] = np.nan
    outs, ran, redone = _run(flt, plan, f, (0, 2))
    _table_ran(ran)
    assert "nt" not in ran[0][1] and ran[1][1].get("nt") == 1, ran
    assert redone[0] > 0 and redone[1] == redone[0], redone
    assert _same(outs[0], outs[1]), ran
    assert np.isnan(outs[1][cell]) and not np.isnan(outs[1][wet == 1]).all()


def test_streamed_result_against_the_oracle():
    flt, plan, f0, wet, gv = _case("fixture", SMALL, 27)
    f = T.treat_land(f0, wet, "nan")
    (got,), ran, redone = _run(flt, plan, f, (2,))
    _table_ran(ran)
    assert ran[0][1].get("nt") == 1 and redone == [0], (ran, redone)
    fs = flt.filter_spec
    with np.errstate(all="ignore"):
        ref = O.filter_func(O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq), GRID, f, gv)
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert ok.any() and np.abs(got[ok] - ref[ok]).max() <= 1e-12 * np.abs(ref[ok]).max()


def test_the_default_streams_at_baseline_size():
    """2400 x 3600 with the fixture mask: 6.5 M owned cells x 65 bytes = 421 MB per launch, more than the cache holds -- the plan's defaults
    (options "wet_rows" 3, "stream_state" 1) take the streaming form; option 0 gives the same bits.  One application each."""
    flt, plan, f0, wet, gv = _case("fixture", (2400, 3600), 18)
    f = T.treat_land(f0, wet, "nan")
    outs, ran, redone = _run(flt, plan, f, (1, 0), wet_rows=3)
    _table_ran(ran)
    assert ran[0][1].get("nt") == 1 and "nt" not in ran[1][1], ran
    assert (ran[0][1]["units"], ran[0][1]["H"], ran[0][1]["xoff"]) == (510, 60, 36), ran
    assert redone == [0, 0], redone
    assert _same(outs[0], outs[1])
