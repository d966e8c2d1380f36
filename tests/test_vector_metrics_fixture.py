"""``testing.vector_grid_vars_irregular`` must be able to see the faults that ``testing.vector_grid_vars`` cannot (CPU, the oracle only).

On the spherical fixture no metric plane varies along x, so a vector kernel that reads a coefficient one column off, or takes dxT for dxCu,
gives the same answer as a correct one.  For the irregular fixture this module asserts, with the oracle's Laplacian of the seeded fields
(42, 43) at (24, 32) and (40, 64):

* every ordered pair of distinct spacing / area planes differs somewhere, and no plane is constant along x or along y;
* rolling any one spacing, area or kappa plane by one column changes L by at least 1e-3 of max|L|; so does rolling it by one row;
* so does each swap of two planes a kernel could mistake for one another (SWAPS);
* on ``vector_grid_vars`` the same column rolls change L by exactly 0 -- which is why the new fixture exists;
* all ten B-grid stencil weights reach 1e-3 of max|cc|;
* the oracle's filter stays bounded (max|out| <= 2 max|in|) for every (shape, n_steps, scale) the GPU cases on this fixture use.

1e-3 is a condition on the inputs, not a tolerance: a plane that falls short calls for a stronger fixture, not a lower threshold.
The module also checks that the irregular GPU cases name every vector kernel family the dispatch-edge table names.
"""
import functools

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from oracle import gcmf_oracle as O

SHAPES = [(24, 32), (40, 64)]
SEE = 1e-3
SWAPS = {
    "VECTOR_C_GRID": [("dxT", "dxCu"), ("dxBu", "dxCv"), ("dxCu", "dxCv"), ("dyT", "dyCu"), ("dyCu", "dyCv"), ("dyBu", "dyT"),
                      ("area_u", "area_v")],
    "VECTOR_B_GRID": [("HUS", "HTE"), ("HUW", "HTN"), ("HUS", "HUW"), ("HTE", "HTN"), ("DXU", "DYU"), ("UAREA", "TAREA")],
}


def metric_names(grid):
    """The spacing and area planes of a vector kind."""
    return [n for n in T.FIXTURE_ARG_ORDER[grid] if n not in T.VECTOR_MASKS + T.VECTOR_KAPPAS]


def rolled_names(grid):
    """Spacing, area and kappa planes."""
    return [n for n in T.FIXTURE_ARG_ORDER[grid] if n not in T.VECTOR_MASKS]


def laplacian(grid, gv, shape):
    with np.errstate(all="ignore"):
        return np.stack(O.make_laplacian(grid, gv)(T.random_field(shape, 42), T.random_field(shape, 43)))


@functools.lru_cache(maxsize=None)
def base(grid, shape, irregular=True):
    gv = T.vector_grid_vars_irregular(grid, shape) if irregular else T.vector_grid_vars(grid, shape)
    L = laplacian(grid, gv, shape)
    for a in list(gv.values()) + [L]:
        a.setflags(write=False)
    return gv, L


def change(grid, shape, mutated, irregular=True):
    """max|L(mutated planes) - L| / max|L|."""
    gv, L = base(grid, shape, irregular)
    return float(np.abs(laplacian(grid, {**gv, **mutated}, shape) - L).max() / np.abs(L).max())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("grid", T.VECTOR_GRIDS)
def test_the_fixture_is_plain_float64_in_fixture_order(grid, shape):
    gv, L = base(grid, shape)
    assert list(gv) == T.FIXTURE_ARG_ORDER[grid]
    assert all(type(v) is np.ndarray and v.dtype == np.float64 and v.shape == shape for v in gv.values())
    assert np.isfinite(L).all() and np.abs(L).max() > 0
    old = T.vector_grid_vars(grid, shape)
    for n in T.VECTOR_MASKS:
        if n in gv:
            assert np.array_equal(gv[n], old[n])
    if grid == "VECTOR_C_GRID":
        assert gv["kappa_iso"].max() == 1.0 and gv["kappa_iso"].min() > 0 and 0 < gv["kappa_aniso"].min() and gv["kappa_aniso"].max() < 1
        t = T.coastline("speckle", shape, 7)
        for indq in (False, True):
            cv = T.vector_grid_vars_irregular(grid, shape, coast="speckle", independent_q=indq, coast_seed=7)
            want = T.cgrid_coast_vars("speckle", shape, 7, independent_q=indq)
            assert np.array_equal(cv["wet_mask_t"], t) and np.array_equal(cv["wet_mask_q"], want["wet_mask_q"])
            assert all(np.array_equal(cv[n], gv[n]) for n in rolled_names(grid))
    # seed0 moves every metric plane
    other = T.vector_grid_vars_irregular(grid, shape, seed0=90)
    assert all(not np.array_equal(other[n], gv[n]) for n in rolled_names(grid))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("grid", T.VECTOR_GRIDS)
def test_planes_are_distinct_and_vary_along_both_axes(grid, shape):
    gv, _ = base(grid, shape)
    names = metric_names(grid)
    for a in names:
        for b in names:
            if a != b:
                assert (gv[a] != gv[b]).any(), (a, b)
    for n in rolled_names(grid):
        assert (np.ptp(gv[n], axis=1) > 0).all(), (n, "a row is constant along x")
        assert (np.ptp(gv[n], axis=0) > 0).all(), (n, "a column is constant along y")


@pytest.mark.parametrize("axis", [1, 0], ids=["column", "row"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("grid", T.VECTOR_GRIDS)
def test_a_plane_rolled_by_one_shows(grid, shape, axis):
    gv, _ = base(grid, shape)
    for n in rolled_names(grid):
        d = change(grid, shape, {n: np.roll(gv[n], 1, axis=axis)})
        print(f"{grid} {shape} {n} rolled along axis {axis}: {d:.3e} of max|L|")
        assert d >= SEE, (grid, shape, n, axis, d)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("grid", T.VECTOR_GRIDS)
def test_two_planes_swapped_show(grid, shape):
    gv, _ = base(grid, shape)
    for a, b in SWAPS[grid]:
        d = change(grid, shape, {a: gv[b], b: gv[a]})
        print(f"{grid} {shape} {a} <-> {b}: {d:.3e} of max|L|")
        assert d >= SEE, (grid, shape, a, b, d)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("grid", T.VECTOR_GRIDS)
def test_the_spherical_fixture_sees_no_column_roll(grid, shape):
    """Why the irregular fixture exists: on vector_grid_vars a coefficient read one column off is the same number."""
    gv, _ = base(grid, shape, irregular=False)
    for n in rolled_names(grid):
        assert change(grid, shape, {n: np.roll(gv[n], 1, axis=1)}, irregular=False) == 0.0, n
    if grid == "VECTOR_B_GRID":
        c = O.bgrid_coefficients(**gv)
        assert all(np.all(c[k] == 0.0) for k in ("dmc", "dme", "dmw"))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_b_grid_weight_is_live(shape):
    gv, _ = base("VECTOR_B_GRID", shape)
    c = O.bgrid_coefficients(**gv)
    assert len(c) == 10
    cc = np.abs(c["cc"]).max()
    for k, w in c.items():
        print(f"B-grid {shape} max|{k}| = {np.abs(w).max() / cc:.3e} max|cc|")
        assert np.abs(w).max() > SEE * cc, (k, float(np.abs(w).max() / cc))


# ------------------------------------------------------------------------------------------------------------------------------
# the filters the GPU cases run on this fixture stay bounded
# ------------------------------------------------------------------------------------------------------------------------------
def gpu_filters():
    """Every distinct (grid, shape, coastline, filter shape, scale in dx_min, n_steps (0 = the default)) of the GPU cases on the irregular
    fixture: tests/test_gpu_vector_metrics.py (both tables), the ':irr' rows of tests/test_gpu_slab_seams.py, the C-grid cases of
    tests/test_gpu_adjoint.py."""
    import make_golden as MG
    import test_gpu_slab_seams as SS
    import test_gpu_vector_metrics as VM

    out = {(c.grid, c.shape, c.coast, "GAUSSIAN", 4.0, c.n_steps) for c in VM.CASES}
    for name in MG.vector_metrics_case_names():
        grid, _, _, fk = MG.build_vector_metrics_case(name)
        if fk is not None:
            scale = {"GAUSSIAN": 8.0, "TAPER": 4.0}[fk["filter_shape"]]
            out.add((grid, MG.SMALL, "speckle:indq" if name.endswith("speckle_indq") else "", fk["filter_shape"], scale, 0))
    out |= {(c.grid, c.shape, c.coast.replace(":irr", ""), "GAUSSIAN", 4.0, c.n_steps) for c in SS.CASES if c.coast.endswith(":irr")}
    out.add(("VECTOR_C_GRID", (96, 160), "", "GAUSSIAN", 6.0, 12))
    return sorted(out)


@pytest.mark.parametrize("grid,shape,coast,fshape,scale,n_steps", gpu_filters(),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_filter_stays_bounded(grid, shape, coast, fshape, scale, n_steps):
    name, _, variant = coast.partition(":")
    gv = T.vector_grid_vars_irregular(grid, shape, coast=name, independent_q=variant == "indq", coast_seed=55)
    dx = T.grid_dx_min(grid, gv)
    spec = O.make_spec(scale * dx, dx, fshape, n_steps=n_steps)
    u, v = T.random_field(shape, 42), T.random_field(shape, 43)
    with np.errstate(all="ignore"):
        out = O.filter_func_vec(spec, grid, u, v, gv)
    worst, largest_in = max(float(np.abs(o).max()) for o in out), max(float(u.max()), float(v.max()))
    print(f"{grid} {shape} {coast} {fshape} {scale} dx n_steps {spec.n_steps}: max|out| = {worst:.3f}, max|in| = {largest_in:.3f}")
    assert np.isfinite(worst) and worst <= 2.0 * largest_in, (grid, shape, coast, spec.n_steps, worst)


def test_the_irregular_cases_name_every_vector_kernel_family():
    import test_gpu_dispatch_edges as DE
    import test_gpu_vector_metrics as VM

    want = VM.families(DE.CASES)
    assert len(want) >= 9, want
    assert VM.families(VM.CASES) == want, (sorted(VM.families(VM.CASES) ^ want))
