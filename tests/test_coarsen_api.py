"""`Filter.apply_coarsened`, `Plan.set_coarsen_weights` / `Plan.apply_coarsen`, `gcmf_coarsen_weights` / `gcmf_apply_coarsen`: the
host-side surface (no GPU needed: every refusal here comes before a plan is made).  What the call computes is checked on the GPU in
tests/test_gpu_coarsen.py, the rule itself in tests/test_coarsen_rule.py."""
import glob
import inspect
import os
import re

import numpy as np
import pytest

import fake_xarray
from gcm_filters_amd import Filter, GridType, _build, _lib, coarsen
from gcm_filters_amd.kernels import ALL_KERNELS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gcm_filters_amd", "csrc")


def _grid_vars(grid, shape=(8, 12)):
    """Placeholders with the right names: a Filter's construction only looks at the names (the plans are made at the first call)."""
    return {k: np.ones(shape) for k in ALL_KERNELS[GridType[grid]].required_grid_args()}


def _filter(grid, shape=(8, 12), **kw):
    return Filter(filter_scale=4.0, dx_min=1.0, grid_type=GridType[grid], grid_vars=_grid_vars(grid, shape), **kw)


def test_header_declares_both_calls_and_their_contract():
    with open(os.path.join(REPO, "include", "gcmf.h")) as f:
        src = f.read()
    w = re.search(r"int gcmf_coarsen_weights\(([^;]*)\);", src)
    a = re.search(r"int gcmf_apply_coarsen\(([^;]*)\);", src)
    assert w and a, "gcmf_coarsen_weights / gcmf_apply_coarsen are not declared"
    assert " ".join(w.group(1).split()) == "gcmf_plan *plan, const void *w, int64_t nlev, uint32_t flags"
    assert " ".join(a.group(1).split()) == ("gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in, void *const *out, "
                                            "void *const *wsum, int64_t nbatch, int fy, int fx, uint32_t flags, void *stream")
    doc = src[src.index("FILTER, THEN COARSE-GRAIN"):a.start()]
    for word in ("GCMF_OUT_F32", "row slabs", "b % nlev", '"coarsen_scratch_mb"', "k_prepare", "GCMF_PLAN_SELF_RING", "ncomp == 2", "wsum = 0",
                 "never multiplied", "GCMF_MASK_FROM_NAN", "GCMF_FACES_FROM_NAN", "w == NULL"):
        assert word in doc, word
    assert src.count('"coarsen_scratch_mb"') >= 2      # the contract and gcmf_set_option's list


def test_option_is_known_to_the_library_and_the_binding():
    with open(os.path.join(CSRC, "gcmf_api_options.hip")) as f:
        assert '"coarsen_scratch_mb"' in f.read()
    assert "coarsen_scratch_mb" in _lib.Plan.set_option.__doc__


def test_exports_and_binding():
    assert _lib.EXPORTS_COARSEN == ["gcmf_coarsen_weights", "gcmf_apply_coarsen"]
    assert not set(_lib.EXPORTS_COARSEN) & set(_lib.EXPORTS)
    src = inspect.getsource(_lib.load)
    for name in _lib.EXPORTS_COARSEN:
        assert f"lib.{name}.argtypes" in src and f"lib.{name}.restype" in src, name
    sig = inspect.signature(_lib.Plan.apply_coarsen).parameters
    assert list(sig)[:8] == ["self", "p", "c", "ins", "outs", "nbatch", "fy", "fx"]
    assert sig["wsums"].default is None and sig["mask_from_nan"].default is False and sig["faces_from_nan"].default is False
    assert "out_f32" not in sig      # the coarse planes are always float64
    assert list(inspect.signature(_lib.Plan.set_coarsen_weights).parameters) == ["self", "weights", "nlev", "device_ptrs"]


def test_filter_method_and_nothing_else_changed_on_the_class():
    assert list(inspect.signature(Filter.apply_coarsened).parameters) == ["self", "field", "factor", "dims", "weights", "return_weights"]
    p = inspect.signature(Filter.apply_coarsened).parameters
    assert p["dims"].default is None and p["weights"].default is None and p["return_weights"].default is False
    assert list(inspect.signature(Filter.apply).parameters) == ["self", "ds", "dims"]
    assert "coarsen" not in repr(_filter("REGULAR"))


def test_the_pass_is_a_form_of_k_prepare_in_its_own_unit():
    """No kernel of a new name (tests/test_kernel_inventory.py would fail on one) and none added to gcmf_scalar.hip, whose two forms
    tests/test_adjoint_api.py counts: the pass lives in gcmf_coarsen.hip, which the library is built from, and shares the rule header
    with the plain C++ restatement."""
    with open(os.path.join(CSRC, "gcmf_coarsen.hip")) as f:
        src = f.read()
    forms = re.findall(r"template <([^>]*)>\s*__global__[^\n]*\bvoid\s+(k_[a-z_0-9]+)\s*\(const (\w+) P\)", src)
    assert forms == [("int VEC", "k_prepare", "CoarsenP")], forms
    assert "gcmf_coarsen.hip" in _build.SOURCES
    assert '#include "gcmf_coarsen.hpp"' in src and "coarsen_term(" in src and "coarsen_mean(" in src
    assert "atomic" not in src.replace("No atomics", "")
    with open(os.path.join(CSRC, "gcmf_coarsen.hpp")) as f:
        rule = f.read()
    for word in ("coarsen_counts", "coarsen_term", "coarsen_mean", "coarsen_plane", "hip_runtime"):
        assert (word in rule) == (word != "hip_runtime"), word
    words = set()
    for path in glob.glob(os.path.join(CSRC, "gcmf_coarsen.hip")) + glob.glob(os.path.join(CSRC, "gcmf_coarsen.hpp")):
        with open(path) as f:
            words.update(re.findall(r"\bk_[a-z_0-9]+", f.read()))
    assert words <= {"k_prepare", "k_land_fix", "k_resident"}, words


# ---- refusals, all before any plan exists ---------------------------------------------------------------------------------------------
def test_a_factor_that_does_not_divide_names_both_lengths():
    flt = _filter("REGULAR_WITH_LAND")
    with pytest.raises(ValueError, match=r"ny = 8 over fy = 3 .* nx = 12 over fx = 4"):
        flt.apply_coarsened(np.zeros((8, 12)), (3, 4))
    with pytest.raises(ValueError, match=r"ny = 8 over fy = 5 .* nx = 12 over fx = 5"):
        flt.apply_coarsened(np.zeros((2, 8, 12)), 5)
    assert coarsen.check_factor(4, 8, 12) == (4, 4) and coarsen.check_factor((2, 3), 8, 12) == (2, 3)


@pytest.mark.parametrize("factor", [0, (0, 2), (2, -1), 1.5, "x", (1, 2, 3)])
def test_a_factor_that_is_no_positive_int_raises(factor):
    with pytest.raises(ValueError, match="factor must be"):
        _filter("REGULAR").apply_coarsened(np.zeros((8, 12)), factor)


def test_xarray_objects_are_refused_with_what_to_do_instead():
    da = fake_xarray.DataArray(np.zeros((8, 12)), dims=("y", "x"))
    with pytest.raises(NotImplementedError, match=r"\.data"):
        _filter("REGULAR").apply_coarsened(da, 2, dims=["y", "x"])


def test_vector_grid_types_are_refused():
    with pytest.raises(NotImplementedError, match="vector grid type"):
        _filter("VECTOR_C_GRID").apply_coarsened(np.zeros((8, 12)), 2)
    with pytest.raises(NotImplementedError, match="vector grid type"):
        coarsen.default_weights(GridType.VECTOR_B_GRID, {})


def test_a_tensor_that_requires_grad_is_never_detached_silently():
    torch = pytest.importorskip("torch")
    x = torch.zeros(8, 12, dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="detach"):
        _filter("REGULAR").apply_coarsened(x, 2)


@pytest.mark.parametrize("bad,match", [(np.ones((8, 6)), "weights have shape"), (np.ones((3, 8, 12)), "weights have shape"),
                                       (-np.ones((8, 12)), "negative or NaN"), (np.full((8, 12), np.nan), "negative or NaN")])
def test_bad_weights_raise(bad, match):
    with pytest.raises(ValueError, match=match):
        _filter("REGULAR_WITH_LAND").apply_coarsened(np.zeros((8, 12)), 2, weights=bad)


def test_weights_with_the_grid_variables_leading_dims_are_a_shape_that_fits():
    flt = _filter("REGULAR_WITH_LAND", shape=(3, 8, 12))
    with pytest.raises(ValueError, match=r"\(3, 8, 12\)"):
        flt.apply_coarsened(np.zeros((3, 8, 12)), 2, weights=np.ones((2, 8, 12)))


def test_default_weights_table():
    rng = np.random.default_rng(3)
    for grid, names in (("REGULAR", ()), ("REGULAR_WITH_LAND", ("wet_mask",)), ("REGULAR_AREA_WEIGHTED", ("area",)),
                        ("REGULAR_WITH_LAND_AREA_WEIGHTED", ("area", "wet_mask")),
                        ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", ("area", "wet_mask")), ("IRREGULAR_WITH_LAND", ("area", "wet_mask")),
                        ("MOM5U", ("area_u", "wet_mask")), ("MOM5T", ("area_t", "wet_mask")), ("TRIPOLAR_POP_WITH_LAND", ("tarea", "wet_mask"))):
        gv = {k: rng.random((8, 12)) for k in ALL_KERNELS[GridType[grid]].required_grid_args()}
        if "wet_mask" in gv:
            gv["wet_mask"] = (gv["wet_mask"] < 0.7).astype(np.float64)
        w = coarsen.default_weights(GridType[grid], gv)
        if not names:
            assert w is None
            continue
        want = gv[names[0]] if len(names) == 1 else gv[names[0]] * gv[names[1]]
        assert np.array_equal(w, want), grid
    # a level axis on one variable is the weights' level axis
    gv = {k: rng.random((8, 12)) for k in ALL_KERNELS[GridType.IRREGULAR_WITH_LAND].required_grid_args()}
    gv["wet_mask"] = (rng.random((3, 8, 12)) < 0.7).astype(np.float64)
    assert coarsen.default_weights(GridType.IRREGULAR_WITH_LAND, gv).shape == (3, 8, 12)


def test_the_numpy_restatement_follows_the_rule():
    f = np.array([[1.0, np.nan, 3.0, np.inf], [5.0, 6.0, -np.inf, 8.0]])
    w = np.array([[1.0, 1.0, 0.0, 0.0], [3.0, -1.0, np.nan, -0.0]])
    coarse, wsum = coarsen.block_means(f, w, (2, 2))
    assert np.array_equal(wsum, [[4.0, 0.0]]) and coarse[0, 0] == (1.0 + 15.0) / 4.0 and np.isnan(coarse[0, 1])
    coarse, wsum = coarsen.block_means(f, None, (2, 4))
    assert wsum[0, 0] == 7.0 and np.isnan(coarse[0, 0])      # +inf and -inf both count: their sum is NaN, as the rule has it


def test_docs_mention_the_call():
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        with open(os.path.join(REPO, name)) as f:
            assert "gcmf_apply_coarsen" in f.read(), name
