"""Stacked plans (``gcmf_plan_create_levels``): what can be checked without a GPU -- the header declares the entry points, the ctypes
binding exports them, and the built library holds the ten instantiations of k_ringc that add a level offset to their coefficient rows,
each inside the budget of the marching kernels (no scratch, at most 512 registers).  tests/test_gpu_level_stack.py runs them."""
import os
import re
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import check_isa  # noqa: E402

needs_llvm = pytest.mark.skipif(not os.path.exists(os.path.join(check_isa.LLVM, "llvm-readelf")), reason="no ROCm llvm tools")


def test_the_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "gcmf.h")).read())
    assert ("int gcmf_plan_create_levels(const gcmf_plan_desc *desc, const void *const *planes, const int64_t *plane_levels, int nplanes, "
            "int64_t nlev, gcmf_plan **out);") in text
    assert "int64_t gcmf_plan_levels(const gcmf_plan *plan);" in text
    # gcmf_plan_desc keeps its layout: the new entry point takes the level counts beside it
    desc = text[text.index("typedef struct gcmf_plan_desc {"): text.index("} gcmf_plan_desc;")]
    assert re.findall(r"int(?:32|64)_t ([a-z_, ]+);", desc) == ["grid_type", "dtype", "ny, nx", "row_begin", "row_end", "halo", "device",
                                                              "planes_on_device", "flags"]


def test_the_binding_exports_them():
    from gcm_filters_amd import _lib
    assert {"gcmf_plan_create_levels", "gcmf_plan_levels"} <= set(_lib.EXPORTS_LEVELS)
    assert callable(_lib.Plan.create_levels) and isinstance(_lib.Plan.levels, property)
    from gcm_filters_amd import _build
    assert {"gcmf_ringc_levels.hip", "gcmf_ringc_levels_b.hip"} <= set(_build.SOURCES)
    if os.path.exists(_lib.LIB_PATH):           # the built library: the symbols are there and typed
        lib = _lib.load()
        assert lib.gcmf_plan_levels.restype is not None and lib.gcmf_plan_levels(None) == 0
        assert len(lib.gcmf_plan_create_levels.argtypes) == 6


@needs_llvm
def test_the_library_holds_the_ten_instantiations_within_budget():
    want = {f"gcmf::k_ringc<double, 2, {S}, {first}, false, true>" for S in range(5, 10) for first in ("true", "false")}
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        kernels = []
        for i, co in enumerate(check_isa.code_objects(check_isa.LIB)):
            kernels += check_isa.kernel_metadata(co, tmp, i)
        for k, d in zip(kernels, check_isa.demangle([k["name"] for k in kernels])):
            name = d.replace("void ", "").split("(")[0]
            if name in want:
                found[name] = k
    assert set(found) == want, sorted(want - set(found))
    for name, k in sorted(found.items()):
        alloc = (k["vgpr"] + 7) // 8 * 8
        print(f"{name}: registers {k['vgpr']} (allocated {alloc}), scratch {k['scratch']}")
        assert k["scratch"] == 0, (name, k["scratch"])
        assert alloc <= 512, (name, alloc)
    # ... and the ordinary instantiations are still there beside them (a stacked launch must not replace them)
    assert len(want) == 10
