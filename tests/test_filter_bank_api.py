"""``FilterBank`` without a device: the one polynomial degree of a sweep, its per-scale ``FilterSpec`` objects against the oracle's
Galerkin fit, and construction-time validation (``Filter``'s own messages, raised once, plus the bank's own for its scales).  Nothing here
builds a Laplacian or a plan: construction is host work, as ``Filter``'s is."""
import warnings

import numpy as np
import pytest

import gcm_filters_amd
from gcm_filters_amd import Filter, FilterBank, FilterShape, GridType, _lib
from gcm_filters_amd import filter as F
from oracle import gcmf_oracle as O

SCALES = [2.0, 3.0, 4.5, 8.0, 12.5]
BELOW = "You have set n_steps below the default. Results might not be accurate."


def default_of(shape, scale, dx_min=1.0, width=np.pi, ndim=2):
    return int(O.n_steps_default(ndim, shape.name, scale, dx_min, width))


def test_exported():
    assert gcm_filters_amd.FilterBank is F.FilterBank and "FilterBank" in gcm_filters_amd.__all__
    assert set(_lib.EXPORTS_BANK) == {"gcmf_apply_bank", "gcmf_bank_cut"}


@pytest.mark.parametrize("shape", [FilterShape.GAUSSIAN, FilterShape.TAPER])
@pytest.mark.parametrize("ndim", [1, 2])
def test_n_steps_is_the_largest_default(shape, ndim):
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # (the bank's own degree warns about nothing)
        bank = FilterBank(filter_scales=SCALES, dx_min=1.0, filter_shape=shape, ndim=ndim)
    per_scale = [default_of(shape, s, ndim=ndim) for s in SCALES]
    assert bank.n_steps == max(per_scale) and len(set(per_scale)) > 1
    assert [f.n_steps for f in bank.filters] == [bank.n_steps] * len(SCALES)
    assert [f.filter_scale for f in bank.filters] == SCALES == bank.filter_scales
    # ... which is Filter's default for the largest scale
    assert bank.n_steps == Filter(filter_scale=max(SCALES), dx_min=1.0, filter_shape=shape, ndim=ndim).n_steps
    assert bank.last_route is None


def test_callers_n_steps_is_honoured_and_warns_once_below_the_default():
    top = max(default_of(FilterShape.TAPER, s) for s in SCALES)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        bank = FilterBank(filter_scales=SCALES, dx_min=1.0, filter_shape=FilterShape.TAPER, n_steps=top - 5)
    assert bank.n_steps == top - 5 and [f.n_steps for f in bank.filters] == [top - 5] * len(SCALES)
    assert [str(x.message) for x in w] == [BELOW]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert FilterBank(filter_scales=SCALES, dx_min=1.0, filter_shape=FilterShape.TAPER, n_steps=top + 7).n_steps == top + 7
        assert FilterBank(filter_scales=SCALES, dx_min=1.0, filter_shape=FilterShape.TAPER, n_steps=top).n_steps == top
        assert FilterBank(filter_scales=SCALES, dx_min=1.0, filter_shape=FilterShape.TAPER, n_steps=2).n_steps == top   # (< 3: the default)


@pytest.mark.parametrize("shape", [FilterShape.GAUSSIAN, FilterShape.TAPER])
@pytest.mark.parametrize("dx_min, width, n_steps", [(1.0, np.pi, 0), (0.37, 2.0, 0), (1.0, np.pi, 40)])
def test_filter_specs_are_the_oracles(shape, dx_min, width, n_steps):
    scales = [s * dx_min for s in SCALES]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bank = FilterBank(filter_scales=scales, dx_min=dx_min, filter_shape=shape, transition_width=width, n_steps=n_steps)
    assert len(bank.filter_specs) == len(scales)
    for s, spec in zip(scales, bank.filter_specs):
        want = O.filter_spec(s, dx_min, shape.name, width, 2, bank.n_steps)
        assert spec.n_steps == want.n_steps == bank.n_steps
        assert spec.s_max == want.s_max and spec.dx_min_sq == want.dx_min_sq
        p, q = np.asarray(spec.p), np.asarray(want.p)
        assert p.shape == q.shape == (bank.n_steps + 1,)
        assert np.max(np.abs(p - q)) <= 1e-13 * np.max(np.abs(q)), (s, np.max(np.abs(p - q)))
    assert len({spec.s_max for spec in bank.filter_specs}) == 1          # one operator for every scale
    assert len({tuple(np.asarray(spec.p)) for spec in bank.filter_specs}) == len(scales)   # ... and a polynomial each
    assert [f.filter_spec for f in bank.filters] == bank.filter_specs


@pytest.mark.parametrize("scales", [[], (), [1.0, 0.0], [2.0, -3.0], [np.nan], [np.inf, 2.0]])
def test_bad_scales(scales):
    with pytest.raises(ValueError, match="filter_scales"):
        FilterBank(filter_scales=scales, dx_min=1.0)


def test_filters_own_validation_raised_as_filter_raises_it():
    def both(match, exc=ValueError, **kw):
        one = {k: v for k, v in kw.items()}
        with pytest.raises(exc) as e1:
            Filter(filter_scale=4.0, **one)
        with pytest.raises(exc) as e2:
            FilterBank(filter_scales=[4.0, 8.0], **one)
        assert str(e1.value) == str(e2.value) and match in str(e2.value)

    area = np.ones((8, 16))
    both("dx_min must be set to 1", dx_min=2.0, grid_type=GridType.REGULAR_AREA_WEIGHTED, grid_vars={"area": area})
    both("Transition width must be > 1", dx_min=1.0, transition_width=1.0)
    both("Transition width must be > 1", dx_min=1.0, transition_width=0.5, filter_shape=FilterShape.TAPER)
    both("do not match expected", dx_min=1.0, grid_type=GridType.REGULAR_WITH_LAND, grid_vars={"area": area})
    both("do not match expected", dx_min=1.0, grid_type=GridType.REGULAR, grid_vars={"wet_mask": area})
    both("When ndim > 2, you must set n_steps manually", dx_min=1.0, ndim=3)
    both("evaluation must be one of", dx_min=1.0, evaluation="forward")
    both("plan_cache must be one of", dx_min=1.0, plan_cache="sometimes")


def test_apply_and_apply_to_vector_refuse_the_other_kind_as_filter_does():
    """The kind of Laplacian is tested before anything touches a device."""
    from gcm_filters_amd import testing as T
    f = np.zeros((16, 32))
    gv = T.vector_grid_vars("VECTOR_C_GRID", (16, 32))
    vec = FilterBank(filter_scales=[2.0, 4.0], dx_min=1.0, n_steps=8, grid_type=GridType.VECTOR_C_GRID, grid_vars=gv)
    one = vec.filters[0]
    with pytest.raises(ValueError) as e1:
        one.apply(f)
    with pytest.raises(ValueError) as e2:
        vec.apply(f)
    assert str(e1.value) == str(e2.value) and "is a vector Laplacian" in str(e2.value)
    sca = FilterBank(filter_scales=[2.0, 4.0], dx_min=1.0)
    with pytest.raises(ValueError) as e1:
        sca.filters[0].apply_to_vector(f, f)
    with pytest.raises(ValueError) as e2:
        sca.apply_to_vector(f, f)
    assert str(e1.value) == str(e2.value) and "is a scalar Laplacian" in str(e2.value)
    assert vec.last_route is None and sca.last_route is None
