"""The adjoint of the filter by diagonal similarity -- the rule, in one place, on the host.

``F`` is the linear map ``Filter.apply`` (the reference's ``filter_func`` / ``filter_func_vec``) applies to finite fields.  For every
grid type but ``VECTOR_B_GRID`` its transpose is the filter itself between two diagonal scalings::

    F^T = D F D^-1          i.e.          F^T g = post * F(pre * g),   post = D,  pre = 1 / D

  * the flux-form kinds (``IRREGULAR_WITH_LAND``, ``MOM5U``, ``MOM5T``, ``TRIPOLAR_POP_WITH_LAND``): ``L = diag(1 / area) M`` with ``M``
    symmetric -- every face couples its two cells with one coefficient, and the tripole fold ``i <-> nx-1-i`` is symmetric as well -- so
    ``L^T = D L D^-1`` with ``D = area``, and the same holds for any polynomial in ``L``;
  * the area-weighted kinds run a symmetric stencil between ``prepare`` (``* area``) and ``finalize`` (``/ area``): ``D = area^2``;
  * ``REGULAR`` and ``REGULAR_WITH_LAND`` are symmetric as they are: ``D = 1``;
  * ``VECTOR_C_GRID`` is symmetric under ``diag(area_u, area_v)``;
  * the B-grid Laplacian has no diagonal symmetrizer at all (its matrix has a symmetric pattern, but ``sign(L_ij) != sign(L_ji)`` on part
    of its couplings): it needs a transposed stencil and raises here.

Land cells and cells cut off from the sea evolve on their own: ``F`` is diagonal there and the identity holds for any finite, non-zero
``D``.  The scalings are 1 on those cells, so that junk metrics on land (POP's ``tarea``) never reach a result.

This module is the specification (tests/test_adjoint_rule.py checks it against dense matrices of the pinned oracle).  The device code
(``gcmf_apply_adjoint``, include/gcmf.h) restates it with the planes the plan really holds -- ``ra = 1 / area`` on the flux kinds, hence
``* ra`` on the way in and ``/ ra`` on the way out: the exact symmetrizer of the operator the kernels apply.
"""
from __future__ import annotations

import numpy as np

from .kernels import ALL_KERNELS, GridType

__all__ = ["adjoint_scaling", "exchanging_cells"]

_AREA_OF_FLUX_KIND = {
    GridType.IRREGULAR_WITH_LAND: "area",
    GridType.MOM5U: "area_u",
    GridType.MOM5T: "area_t",
    GridType.TRIPOLAR_POP_WITH_LAND: "tarea",
}
_AREA_SQUARED = (GridType.REGULAR_AREA_WEIGHTED, GridType.REGULAR_WITH_LAND_AREA_WEIGHTED,
                 GridType.TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED)


def _E(a):
    return np.roll(a, -1, axis=-1)


def _W(a):
    return np.roll(a, 1, axis=-1)


def _N(a):
    return np.roll(a, -1, axis=-2)


def _S(a):
    return np.roll(a, 1, axis=-2)


def _host(a):
    if hasattr(a, "dims") and hasattr(a, "data"):     # an xarray.DataArray: its payload
        a = a.data
    if type(a).__module__.split(".")[0] == "torch":
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def exchanging_cells(grid_type, grid_vars):
    """Boolean plane(s): the cells that exchange with at least one neighbour -- where the scalings apply.  The others are land under a
    wet mask, or cells of a flux-form grid whose four faces are closed (an enclosed lake of one cell, zeros in kappa)."""
    grid_type = GridType[grid_type] if isinstance(grid_type, str) else GridType(grid_type)
    gv = {k: _host(v) for k, v in grid_vars.items()}
    if grid_type in (GridType.REGULAR_WITH_LAND, GridType.REGULAR_WITH_LAND_AREA_WEIGHTED,
                     GridType.TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED):
        return gv["wet_mask"] != 0
    if grid_type is GridType.IRREGULAR_WITH_LAND:
        m = gv["wet_mask"]
        cw = gv["dyw"] / gv["dxw"] * (m * _W(m) * gv["kappa_w"])      # the west face; the east face is the eastern neighbour's west face
        cs = gv["dxs"] / gv["dys"] * (m * _S(m) * gv["kappa_s"])
        return (cw != 0) | (_E(cw) != 0) | (cs != 0) | (_N(cs) != 0)
    if grid_type in (GridType.MOM5U, GridType.MOM5T):
        m = gv["wet_mask"]
        fa, fb = m * _E(m), m * _N(m)     # (the reference masks the north face with m * E(m) and the east face with m * N(m))
        return (fa != 0) | (_S(fa) != 0) | (fb != 0) | (_W(fb) != 0)
    if grid_type is GridType.TRIPOLAR_POP_WITH_LAND:
        m = gv["wet_mask"]
        mx = np.concatenate((m, m[..., -1:, ::-1]), axis=-2)        # the tripole ghost row: the top row mirrored
        fe, fn = mx * _E(mx), mx * _N(mx)
        return ((fe != 0) | (_W(fe) != 0) | (fn != 0) | (_S(fn) != 0))[..., :-1, :]
    shape = np.broadcast_shapes(*[v.shape for v in gv.values()]) if gv else ()
    return np.ones(shape, dtype=bool)


def adjoint_scaling(grid_type, grid_vars):
    """``(pre, post)`` with ``F^T g = post * F(pre * g)`` for the filter ``F`` of ``grid_type`` on ``grid_vars``: float64 numpy planes
    of the grid's shape (scalars 1.0 where the grid type has no grid variables), pairs ``((pre_u, pre_v), (post_u, post_v))`` for
    ``VECTOR_C_GRID``.  1 on land cells and on cells that exchange with no neighbour.

    ``NotImplementedError`` for ``VECTOR_B_GRID``; ``ValueError`` for a C-grid whose ``area_u`` or ``area_v`` has a value ``<= 0`` --
    there the reference zeroes a row of ``L`` but not its column, so the identity fails."""
    grid_type = GridType[grid_type] if isinstance(grid_type, str) else GridType(grid_type)
    if grid_type is GridType.VECTOR_B_GRID:
        raise NotImplementedError("VECTOR_B_GRID has no adjoint by diagonal similarity: its Laplacian has no diagonal symmetrizer D with "
                                  "L^T = D L D^-1 (sign(L_ij) != sign(L_ji) on part of its couplings; UAREA misses by 5.6e-2). It needs a "
                                  "transposed stencil kernel.")
    wanted = ALL_KERNELS[grid_type].required_grid_args()
    if set(wanted) != set(grid_vars):
        raise ValueError(f"Provided `grid_vars` {list(grid_vars)} do not match expected {wanted}")
    if grid_type is GridType.VECTOR_C_GRID:
        au, av = _host(grid_vars["area_u"]), _host(grid_vars["area_v"])
        for name, a in (("area_u", au), ("area_v", av)):
            if not np.all(a > 0):
                raise ValueError(f"VECTOR_C_GRID: {name} has values <= 0; the filter zeroes the row of the Laplacian there but not its "
                                 f"column, so F^T = D F D^-1 does not hold: no adjoint by diagonal similarity")
        return (1.0 / au, 1.0 / av), (au, av)
    if grid_type in _AREA_OF_FLUX_KIND:
        d = _host(grid_vars[_AREA_OF_FLUX_KIND[grid_type]])
    elif grid_type in _AREA_SQUARED:
        d = _host(grid_vars["area"]) ** 2
    else:
        one = np.ones(_host(grid_vars["wet_mask"]).shape) if "wet_mask" in grid_vars else np.float64(1.0)
        return one, one
    live = exchanging_cells(grid_type, grid_vars)
    d = np.broadcast_to(d, np.broadcast_shapes(d.shape, live.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        pre = np.where(live, 1.0 / d, 1.0)
    post = np.where(live, d, 1.0)
    return pre, post
