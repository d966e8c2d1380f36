"""``FilterBank(nan_mask=...)`` and ``gcmf_apply_bank_gaps``: what can be checked without a device -- the argument, its validation (Filter's
own messages), the binding and the header."""
import inspect
import os
import re

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterBank, GridType, _lib, testing as T

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcmf.h")
SHAPE = (16, 32)


def bank_of(kind, nan_mask, **kw):
    gv = T.scalar_grid_vars(kind, SHAPE)
    dx = T.grid_dx_min(kind, gv)
    return FilterBank(filter_scales=[2.0 * dx, 3.0 * dx, 4.0 * dx], dx_min=dx, n_steps=12, grid_type=GridType[kind], grid_vars=gv,
                      nan_mask=nan_mask, **kw)


@pytest.mark.parametrize("kind, nan_mask", [("REGULAR_WITH_LAND", True), ("REGULAR_WITH_LAND", "auto"), ("REGULAR_WITH_LAND", False),
                                            ("REGULAR_WITH_LAND_AREA_WEIGHTED", True), ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "auto"),
                                            ("IRREGULAR_WITH_LAND", "auto"), ("MOM5U", "auto"), ("MOM5T", "auto"), ("MOM5T", False)])
def test_nan_mask_reaches_every_filter(kind, nan_mask):
    bank = bank_of(kind, nan_mask)
    assert bank.nan_mask == nan_mask
    assert [f.nan_mask for f in bank.filters] == [nan_mask] * 3
    assert bank.last_route is None


def test_nan_mask_is_keyword_only_and_off_by_default():
    par = inspect.signature(FilterBank.__init__).parameters["nan_mask"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    bank = FilterBank(filter_scales=[2.0, 4.0], dx_min=1.0)
    assert bank.nan_mask is False and [f.nan_mask for f in bank.filters] == [False, False]


def test_bad_values_and_grid_types_raise_what_filter_raises():
    def both(match, exc=ValueError, **kw):
        with pytest.raises(exc) as e1:
            Filter(filter_scale=4.0, **kw)
        with pytest.raises(exc) as e2:
            FilterBank(filter_scales=[4.0, 8.0], **kw)
        assert str(e1.value) == str(e2.value) and match in str(e2.value)

    both('nan_mask must be False, True or "auto"', dx_min=1.0, nan_mask="yes")
    both('nan_mask must be False, True or "auto"', dx_min=1.0, nan_mask="AUTO", grid_type=GridType.MOM5U,
         grid_vars=T.scalar_grid_vars("MOM5U", SHAPE))
    both('nan_mask="auto" needs one of the grid types', dx_min=1.0, nan_mask="auto")                       # REGULAR
    both("nan_mask=True needs one of the grid types", dx_min=1.0, nan_mask=True)
    for kind in ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T"):       # True is the land-mask kinds' alone
        gv = T.scalar_grid_vars(kind, SHAPE)
        both("nan_mask=True needs one of the grid types", dx_min=T.grid_dx_min(kind, gv), nan_mask=True, grid_type=GridType[kind], grid_vars=gv)
    gv = T.scalar_grid_vars("TRIPOLAR_POP_WITH_LAND", SHAPE)     # outside the six
    for value, match in ((True, "nan_mask=True needs"), ("auto", 'nan_mask="auto" needs')):
        both(match, dx_min=T.grid_dx_min("TRIPOLAR_POP_WITH_LAND", gv), nan_mask=value, grid_type=GridType.TRIPOLAR_POP_WITH_LAND, grid_vars=gv)
    gvec = T.vector_grid_vars("VECTOR_C_GRID", SHAPE)
    both('nan_mask="auto" needs', dx_min=1.0, nan_mask="auto", grid_type=GridType.VECTOR_C_GRID, grid_vars=gvec)
    # the order of Filter's checks: evaluation and plan_cache come before nan_mask, the other arguments after it
    both("evaluation must be one of", dx_min=1.0, evaluation="forward", nan_mask="yes")
    both("plan_cache must be one of", dx_min=1.0, plan_cache="sometimes", nan_mask="yes")
    both("nan_mask must be", dx_min=1.0, transition_width=1.0, nan_mask="yes")


def test_the_symbol_has_a_list_of_its_own():
    assert _lib.EXPORTS_BANK_GAPS == ["gcmf_apply_bank_gaps"]
    assert _lib.EXPORTS_BANK == ["gcmf_apply_bank", "gcmf_bank_cut"]
    assert len(_lib.EXPORTS) == 55 and "gcmf_apply_bank_gaps" not in _lib.EXPORTS


def test_the_header_declares_it_with_extern():
    with open(HEADER) as f:
        src = f.read()
    decl = re.findall(r"^(extern\s+)?int\s+gcmf_apply_bank_gaps\s*\(([^;]*)\);", src, flags=re.M)
    assert len(decl) == 1 and decl[0][0].startswith("extern"), decl
    args = " ".join(decl[0][1].split())
    assert args == ("gcmf_plan *plan, const double *p, int nbank, int n_steps, double c, const void *in, void *out, int64_t nfield, "
                    "uint32_t flags, void *stream")
    same = re.findall(r"^extern\s+int\s+gcmf_apply_bank\s*\(([^;]*)\);", src, flags=re.M)
    assert len(same) == 1 and " ".join(same[0].split()) == args      # gcmf_apply_bank's own argument list
    assert "gap_scratch_mb" in src and "levels=<" in src


def test_plan_apply_bank_takes_faces_from_nan():
    par = inspect.signature(_lib.Plan.apply_bank).parameters["faces_from_nan"]
    assert par.default is False
    from gcm_filters_amd.kernels import BaseScalarLaplacian
    assert inspect.signature(BaseScalarLaplacian._run_bank).parameters["faces_from_nan"].default is False


def test_the_library_exports_it():
    """The built library has the symbol and load() binds it with gcmf_apply_bank's argument types."""
    lib = _lib.load()
    assert lib.gcmf_apply_bank_gaps.argtypes == lib.gcmf_apply_bank.argtypes
    assert lib.gcmf_apply_bank_gaps.restype is lib.gcmf_apply_bank.restype
