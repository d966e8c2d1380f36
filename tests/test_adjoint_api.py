"""`Filter.adjoint` / `adjoint_to_vector`, `Plan.apply_adjoint`, `gcmf_apply_adjoint`: the host-side surface (no GPU needed).  What the
call computes is checked on the GPU in tests/test_gpu_adjoint.py, the scaling rule itself in tests/test_adjoint_rule.py."""
import glob
import inspect
import os
import re

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterBank, GridType, _lib
from gcm_filters_amd.kernels import ALL_KERNELS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")


def _grid_vars(grid):
    """Placeholders with the right names: a Filter's construction only looks at the names (the plans are made at the first call)."""
    return {k: np.ones((8, 8)) for k in ALL_KERNELS[GridType[grid]].required_grid_args()}


def _filter(grid, **kw):
    return Filter(filter_scale=4.0, dx_min=1.0, grid_type=GridType[grid], grid_vars=_grid_vars(grid), **kw)


@pytest.mark.parametrize("grid,nan_mask", [("REGULAR_WITH_LAND", True), ("REGULAR_WITH_LAND_AREA_WEIGHTED", "auto"),
                                           ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", True), ("IRREGULAR_WITH_LAND", "auto"),
                                           ("MOM5U", "auto"), ("MOM5T", "auto")])
def test_nan_mask_requires_like(grid, nan_mask):
    with pytest.raises(ValueError, match="needs `like`"):
        _filter(grid, nan_mask=nan_mask).adjoint(np.zeros((8, 8)))


def test_the_laplacian_drivers_require_like_too():
    lap = object.__new__(ALL_KERNELS[GridType.REGULAR_WITH_LAND])
    with pytest.raises(ValueError, match="needs `like`"):
        lap._run([np.zeros((8, 8))], spec=object(), mask_from_nan=True, adjoint=True)
    with pytest.raises(ValueError, match="filter application"):
        lap._run([np.zeros((8, 8))], spec=None, adjoint=True)


def test_the_b_grid_raises_and_names_the_missing_symmetrizer():
    flt = _filter("VECTOR_B_GRID")
    with pytest.raises(NotImplementedError, match="symmetrizer"):
        flt.adjoint_to_vector(np.zeros((8, 8)), np.zeros((8, 8)))
    lap = object.__new__(ALL_KERNELS[GridType.VECTOR_B_GRID])
    with pytest.raises(NotImplementedError, match="symmetrizer"):
        lap._run([np.zeros((8, 8))] * 2, spec=object(), adjoint=True)


def test_the_b_grid_does_not_detach_a_tensor_that_requires_grad():
    torch = pytest.importorskip("torch")
    flt = _filter("VECTOR_B_GRID")
    u = torch.zeros(8, 8, dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        flt.apply_to_vector(u, torch.zeros(8, 8, dtype=torch.float64))


def test_scalar_and_vector_methods_refuse_each_other():
    with pytest.raises(ValueError, match="only suitable for scalar Laplacians"):
        _filter("VECTOR_C_GRID").adjoint(np.zeros((8, 8)))
    with pytest.raises(ValueError, match="only suitable for vector Laplacians"):
        _filter("REGULAR").adjoint_to_vector(np.zeros((8, 8)), np.zeros((8, 8)))


def test_binding_and_drivers_take_the_keywords():
    sig = inspect.signature(_lib.Plan.apply_adjoint).parameters
    assert sig["likes"].default is None and sig["mask_from_nan"].default is False and sig["faces_from_nan"].default is False
    for cls in ALL_KERNELS.values():
        p = inspect.signature(cls._run).parameters
        assert p["adjoint"].default is False and p["like"].default is None
    assert _lib.EXPORTS_ADJOINT == ["gcmf_apply_adjoint"] and "gcmf_apply_adjoint" not in _lib.EXPORTS
    assert list(inspect.signature(Filter.adjoint).parameters) == ["self", "field", "dims", "like"]
    assert list(inspect.signature(Filter.adjoint_to_vector).parameters) == ["self", "ufield", "vfield", "dims"]
    assert not hasattr(FilterBank, "adjoint")      # (a batched adjoint bank is out of scope: FilterBank.apply is differentiable the plain way)


def test_header_declares_the_call_and_its_contract():
    with open(os.path.join(REPO, "include", "gcmf.h")) as f:
        src = f.read()
    decl = re.search(r"int gcmf_apply_adjoint\(([^;]*)\);", src)
    assert decl, "gcmf_apply_adjoint is not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in, const void *const *like, "
                    "void *const *out, int64_t nbatch, uint32_t flags, void *stream")
    doc = src[src.index("THE ADJOINT"):decl.start()]
    for word in ("F^T = D F D^-1", "area^2", "(area_u, area_v)", "VECTOR_B_GRID", "two planes more", "`like`", "GCMF_MASK_FROM_NAN",
                 "GCMF_FACES_FROM_NAN", "b % nlev", '"adjoint_scratch_mb"', "row slabs", "GCMF_PLAN_SELF_RING", "k_prepare"):
        assert word in doc, word
    assert src.count('"adjoint_scratch_mb"') >= 2      # the contract and gcmf_set_option's list


def test_the_two_passes_are_forms_of_k_prepare():
    """No kernel of a new name: tests/test_kernel_inventory.py would fail on one; this says where the passes live instead."""
    with open(os.path.join(CSRC, "gcmf_scalar.hip")) as f:
        src = f.read()
    forms = re.findall(r"template <([^>]*)>\s*__global__[^\n]*\bvoid\s+k_prepare\s*\(", src)
    assert len(forms) == 2, forms
    assert any("DIV" in f and "VEC" in f for f in forms), forms
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(path) as f:
            names.update(re.findall(r"__global__[^\n]*?\bvoid\s+(k_[a-z_0-9]+)\s*\(", f.read()))
    assert not [n for n in names if "adj" in n or "scale" in n], names


def test_option_and_docs():
    with open(os.path.join(CSRC, "gcmf_api_options.hip")) as f:
        assert '"adjoint_scratch_mb"' in f.read()
    assert "adjoint_scratch_mb" in _lib.Plan.set_option.__doc__
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        with open(os.path.join(REPO, name)) as f:
            assert "gcmf_apply_adjoint" in f.read(), name
