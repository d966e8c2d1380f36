"""The adjoint by diagonal similarity, checked on the CPU against dense matrices of the pinned oracle (oracle/gcmf_oracle.py).

For every grid type but VECTOR_B_GRID ``gcm_filters_amd.adjoint.adjoint_scaling`` returns planes with F^T = post F pre, F being the
matrix of the WHOLE ``filter_func`` / ``filter_func_vec`` (prepare, polynomial, finalize).  The matrices are built column by column on
the 16 x 24 fixture grids of ``gcm_filters_amd.testing``; the scalar kinds run a Taper of 12 steps, the vector kinds a Gaussian of 8.
Gate: max|F^T - post F pre| <= 1e-13 max|F| (measured 4.3e-16 at worst; the wrong power of the area misses by more than 3e-2)."""
import numpy as np
import pytest

from gcm_filters_amd import GridType, testing as T
from gcm_filters_amd.adjoint import adjoint_scaling, exchanging_cells
from oracle import gcmf_oracle as O

SHAPE = (16, 24)
GATE = 1e-13
_DENSE = {}


def spec_for(kind, gv):
    dx = T.grid_dx_min(kind, gv)
    if kind in T.VECTOR_GRIDS:
        return O.make_spec(4 * dx, dx, "GAUSSIAN", n_steps=8)
    return O.make_spec(4 * dx, dx, "TAPER", n_steps=12)


def dense_filter(kind):
    """(F, grid_vars): F[:, q] = the filter of the q-th unit field (vector kinds: u cells first, then v), computed once per kind."""
    if kind not in _DENSE:
        n = SHAPE[0] * SHAPE[1]
        if kind in T.VECTOR_GRIDS:
            _, gv = T.vector_case(kind, SHAPE)
            spec = spec_for(kind, gv)
            F = np.empty((2 * n, 2 * n))
            for q in range(2 * n):
                e = np.zeros(2 * n)
                e[q] = 1.0
                u, v = O.filter_func_vec(spec, kind, e[:n].reshape(SHAPE), e[n:].reshape(SHAPE), gv)
                F[:, q] = np.concatenate([u.ravel(), v.ravel()])
        else:
            _, gv = T.scalar_case(kind, SHAPE)
            spec = spec_for(kind, gv)
            F = np.empty((n, n))
            for q in range(n):
                e = np.zeros(n)
                e[q] = 1.0
                F[:, q] = O.filter_func(spec, kind, e.reshape(SHAPE), gv).ravel()
        assert np.isfinite(F).all(), kind
        _DENSE[kind] = (F, gv)
    return _DENSE[kind]


def miss(F, pre, post):
    """max|F^T - post F pre| / max|F| for diagonal scalings given as flat vectors."""
    return np.abs(F.T - post[:, None] * F * pre[None, :]).max() / np.abs(F).max()


def flat(x, n):
    if isinstance(x, tuple):
        return np.concatenate([np.broadcast_to(a, SHAPE).ravel() for a in x])
    return np.broadcast_to(x, SHAPE).ravel().astype(float)


@pytest.mark.parametrize("kind", [k for k in T.ALL_GRIDS if k != "VECTOR_B_GRID"])
def test_the_transpose_is_the_filter_between_two_scalings(kind):
    F, gv = dense_filter(kind)
    pre, post = adjoint_scaling(GridType[kind], gv)
    n = F.shape[0]
    err = miss(F, flat(pre, n), flat(post, n))
    print(f"{kind}: max|F^T - post F pre| / max|F| = {err:.2e}")
    assert err <= GATE, (kind, err)
    if kind in ("REGULAR", "REGULAR_WITH_LAND"):
        assert np.all(flat(pre, n) == 1) and np.all(flat(post, n) == 1)


def test_the_c_grid_rule_holds_with_areas_of_their_own():
    """On testing.vector_grid_vars_irregular area_u and area_v are independent planes, not dxCu * dyCu and dxCv * dyCv, and every metric
    varies along x: D = (area_u, area_v) still symmetrizes the filter, and taking one area for the other does not."""
    kind = "VECTOR_C_GRID"
    n = SHAPE[0] * SHAPE[1]
    gv = T.vector_grid_vars_irregular(kind, SHAPE)
    spec = spec_for(kind, gv)
    F = np.empty((2 * n, 2 * n))
    for q in range(2 * n):
        e = np.zeros(2 * n)
        e[q] = 1.0
        u, v = O.filter_func_vec(spec, kind, e[:n].reshape(SHAPE), e[n:].reshape(SHAPE), gv)
        F[:, q] = np.concatenate([u.ravel(), v.ravel()])
    assert np.isfinite(F).all()
    pre, post = adjoint_scaling(GridType[kind], gv)
    err = miss(F, flat(pre, 2 * n), flat(post, 2 * n))
    print(f"{kind} on irregular metrics: max|F^T - post F pre| / max|F| = {err:.2e}")
    assert err <= GATE, err
    swapped = miss(F, flat(pre[::-1], 2 * n), flat(post[::-1], 2 * n))
    print(f"{kind} on irregular metrics: area_u and area_v swapped miss by {swapped:.2e}")
    assert swapped > 1e-3, swapped


@pytest.mark.parametrize("kind,area", [("REGULAR_AREA_WEIGHTED", "area"), ("IRREGULAR_WITH_LAND", "area"), ("MOM5U", "area_u"),
                                       ("TRIPOLAR_POP_WITH_LAND", "tarea")])
def test_the_wrong_power_of_the_area_misses(kind, area):
    """area^1 where area^2 belongs (and the other way round) is off by percents: the gate above can tell the two apart."""
    F, gv = dense_filter(kind)
    a = gv[area].ravel().astype(float)
    d = a if kind == "REGULAR_AREA_WEIGHTED" else a ** 2
    err = miss(F, 1 / d, d)
    print(f"{kind}: the wrong power misses by {err:.2e}")
    assert err > 3e-2, (kind, err)


@pytest.mark.parametrize("kind", ["REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "TRIPOLAR_POP_WITH_LAND"])
def test_land_cells_keep_the_factor_one(kind):
    """Land evolves on its own (F is diagonal there): the scalings are 1 on it, whatever the metrics hold there -- also junk."""
    F, gv = dense_filter(kind)
    land = gv["wet_mask"] == 0
    assert land.sum() >= 50, land.sum()
    live = exchanging_cells(GridType[kind], gv)
    assert not live[land].any()
    area = {"REGULAR_WITH_LAND_AREA_WEIGHTED": "area", "IRREGULAR_WITH_LAND": "area", "TRIPOLAR_POP_WITH_LAND": "tarea"}[kind]
    junk = {**gv, area: np.where(land, np.nan, gv[area])}
    pre, post = adjoint_scaling(GridType[kind], junk)
    assert np.all(pre[land] == 1) and np.all(post[land] == 1)
    assert np.isfinite(pre).all() and np.isfinite(post).all()
    n = F.shape[0]
    assert miss(F, flat(pre, n), flat(post, n)) <= GATE
    # off the diagonal F is zero in the rows and columns of land
    Fl = F[land.ravel()]
    assert np.count_nonzero(Fl) == np.count_nonzero(np.diag(F)[land.ravel()])


def test_the_b_grid_has_no_diagonal_symmetrizer():
    F, gv = dense_filter("VECTOR_B_GRID")
    with pytest.raises(NotImplementedError, match="symmetrizer"):
        adjoint_scaling(GridType.VECTOR_B_GRID, gv)
    ua = gv["UAREA"].ravel().astype(float)
    d = np.concatenate([ua, ua])
    err = miss(F, 1 / d, d)
    print(f"VECTOR_B_GRID: UAREA as the scaling misses by {err:.2e}")
    assert err > 1e-3, err     # (measured 5.6e-2: nobody "enables" the B-grid with a diagonal)


def test_a_c_grid_with_a_zero_area_is_refused():
    _, gv = T.vector_case("VECTOR_C_GRID", SHAPE)
    for name in ("area_u", "area_v"):
        bad = {**gv, name: gv[name].copy()}
        bad[name][3, 5] = 0.0
        with pytest.raises(ValueError, match=name):
            adjoint_scaling(GridType.VECTOR_C_GRID, bad)


def test_grid_vars_must_match_the_grid_type():
    with pytest.raises(ValueError, match="do not match"):
        adjoint_scaling(GridType.REGULAR_WITH_LAND, {})
    pre, post = adjoint_scaling("REGULAR", {})
    assert pre == 1.0 and post == 1.0
