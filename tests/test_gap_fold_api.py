"""`Filter(nan_mask="auto")` / `GCMF_FACES_FROM_NAN`: the host-side surface of the per-entry face coefficients of the flux-form grid
types (no GPU needed).  What the flag computes is checked on the GPU in tests/test_gpu_gap_fold.py, the fold rule itself in
tests/test_gap_fold_rule.py."""
import inspect
import os
import re

import numpy as np
import pytest

from gcm_filters_amd import Filter, GridType, _lib
from gcm_filters_amd.kernels import ALL_KERNELS, GAP_FOLD_GRID_TYPES, NAN_MASK_GRID_TYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAND_MASK_KINDS = ("REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED")
FLUX_KINDS = ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T")
SIX = LAND_MASK_KINDS + FLUX_KINDS


def _grid_vars(grid):
    """Placeholders with the right names: a Filter's construction only looks at the names (the plans are made at the first call)."""
    return {k: np.ones((8, 8)) for k in ALL_KERNELS[GridType[grid]].required_grid_args()}


def _filter(grid, **kw):
    return Filter(filter_scale=4.0, dx_min=1.0, grid_type=GridType[grid], grid_vars=_grid_vars(grid), **kw)


@pytest.mark.parametrize("grid", SIX)
def test_auto_is_accepted_on_the_six_kinds(grid):
    assert _filter(grid, nan_mask="auto").nan_mask == "auto"
    assert tuple(g.name for g in NAN_MASK_GRID_TYPES) == LAND_MASK_KINDS and tuple(g.name for g in GAP_FOLD_GRID_TYPES) == FLUX_KINDS


@pytest.mark.parametrize("grid", [g.name for g in GridType if g.name not in SIX])
def test_auto_is_a_value_error_on_the_other_five(grid):
    assert len([g for g in GridType if g.name not in SIX]) == 5
    with pytest.raises(ValueError) as e:
        _filter(grid, nan_mask="auto")
    for kind in SIX:
        assert kind in str(e.value)
    assert grid in str(e.value)
    _filter(grid)      # unflagged: as before


@pytest.mark.parametrize("grid", ["IRREGULAR_WITH_LAND", "REGULAR_WITH_LAND", "REGULAR"])
def test_any_other_string_is_a_value_error(grid):
    with pytest.raises(ValueError, match="yes"):
        _filter(grid, nan_mask="yes")


@pytest.mark.parametrize("grid", FLUX_KINDS)
def test_true_keeps_its_error_on_the_flux_kinds(grid):
    with pytest.raises(ValueError, match="nan_mask=True needs one of the grid types"):
        _filter(grid, nan_mask=True)


def test_repr_unchanged():
    a, b = _filter("IRREGULAR_WITH_LAND"), _filter("IRREGULAR_WITH_LAND", nan_mask="auto")
    assert repr(a) == repr(b) and "nan_mask" not in repr(b)
    assert '"auto"' in Filter.__doc__ and "GCMF_FACES_FROM_NAN" in Filter.__doc__


def test_header_carries_the_flag_with_a_bit_of_its_own():
    with open(os.path.join(REPO, "include", "gcmf.h")) as f:
        src = f.read()
    head = src[src.index("/* gcmf_apply / gcmf_laplacian flags */"):src.index("/* Chebyshev step modes")]
    flags = {name: int(val, 16) for name, val in re.findall(r"#define (GCMF_[A-Z0-9_]+) (0x[0-9a-fA-F]+)u", head)}
    assert flags["GCMF_FACES_FROM_NAN"] == 0x40 == _lib.FACES_FROM_NAN
    assert len(set(flags.values())) == len(flags) >= 7, flags
    for v in flags.values():
        assert v & (v - 1) == 0, flags      # single bits: any two may be combined
    for kind in FLUX_KINDS:
        assert kind in head[head.index("GCMF_FACES_FROM_NAN"):]
    assert '"gap_scratch_mb"' in src


def test_binding_and_drivers_take_the_keyword():
    assert inspect.signature(_lib.Plan.apply).parameters["faces_from_nan"].default is False
    for cls in ALL_KERNELS.values():
        assert inspect.signature(cls._run).parameters["faces_from_nan"].default is False
    assert "gcmf_apply" in _lib.EXPORTS and len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 55     # no new exported symbol


def test_run_refuses_the_keyword_elsewhere():
    lap = object.__new__(ALL_KERNELS[GridType.REGULAR])
    with pytest.raises(ValueError, match="IRREGULAR_WITH_LAND, MOM5U, MOM5T"):
        lap._run([np.zeros((8, 8))], spec=object(), faces_from_nan=True)
