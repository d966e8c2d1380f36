"""Filter, then coarse-grain: the host side of ``Filter.apply_coarsened`` (the device side is ``gcmf_apply_coarsen``, include/gcmf.h).

The rule, for factors ``(fy, fx)`` that divide ``(ny, nx)``, the fine result ``F`` of one 2-D slice and its weight plane ``w``::

    count(j,i)  = w(j,i) > 0  and  F(j,i) == F(j,i)        (+-inf is data; NaN, w <= 0 and NaN weights are skipped, never multiplied)
    wsum(J,I)   = sum of w over the counted cells of block (J, I)
    coarse(J,I) = sum of w * F over the counted cells / wsum(J,I);   NaN (and wsum = 0) when no cell counts

``block_means`` restates it in numpy (the specification the tests compare the device against); ``default_weights`` is the table of the
grid types' own weights.  Everything else here stages arrays and picks the plan, as ``kernels._DeviceLaplacian._run_with`` does for
``apply``: 2-D grid variables run one library call; grid variables with leading dims run the stacked plan's one call where ``apply``
would, and a plan and a call per level otherwise -- each level with its own weight plane either way.
"""
from __future__ import annotations

import threading

import numpy as np

from . import _lib
from .adjoint import _AREA_OF_FLUX_KIND
from .kernels import (CallOptions, GridType, _DEVICE_PTR, _HOST_PTR, _fingerprint, _is_torch, _no_backward_cut, _note_path, _on_gpu,
                      _same_kind, _stage, _translate, _unwrap, compute_dtype, plan_cache_mode)

__all__ = ["block_means", "default_weights", "check_factor"]

_AREA_AND_MASK = (GridType.REGULAR_WITH_LAND_AREA_WEIGHTED, GridType.TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED)
_PLAN_LOCKS_GUARD = threading.Lock()


def _host(a):
    a = _unwrap(a)
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def weight_names(grid_type):
    """The grid variables whose product is the grid type's own weight (() for REGULAR: every cell has weight 1)."""
    grid_type = GridType[grid_type] if isinstance(grid_type, str) else GridType(grid_type)
    if grid_type is GridType.REGULAR:
        return ()
    if grid_type is GridType.REGULAR_WITH_LAND:
        return ("wet_mask",)
    if grid_type is GridType.REGULAR_AREA_WEIGHTED:
        return ("area",)
    if grid_type in _AREA_AND_MASK:
        return ("area", "wet_mask")
    if grid_type in _AREA_OF_FLUX_KIND:
        return (_AREA_OF_FLUX_KIND[grid_type], "wet_mask")
    raise NotImplementedError(f"{grid_type.name} is a vector grid type: fields on it are not coarsened; coarsen each component on the "
                              f"scalar grid type of its points")


def default_weights(grid_type, grid_vars):
    """The weight planes ``Filter.apply_coarsened`` uses without ``weights=``: 1 on REGULAR (None is returned), ``wet_mask``, ``area`` or
    the cell area times ``wet_mask`` (``area``, ``area_u``, ``area_t``, ``tarea``: adjoint.py has the names) -- float64 numpy, with the
    grid variables' broadcast leading dims."""
    names = weight_names(grid_type)
    if not names:
        return None
    w = _host(grid_vars[names[0]])
    for n in names[1:]:
        w = w * _host(grid_vars[n])
    return np.ascontiguousarray(w)


def check_factor(factor, ny, nx):
    """(fy, fx) of ``factor`` -- an int or a pair -- for a grid of (ny, nx); ValueError for a non-positive or non-dividing factor."""
    try:
        fy, fx = (factor, factor) if np.ndim(factor) == 0 else tuple(factor)
        ok = float(fy) == int(fy) and float(fx) == int(fx)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"factor must be a positive int or a pair (fy, fx) of them, not {factor!r}")
    fy, fx = int(fy), int(fx)
    if fy < 1 or fx < 1:
        raise ValueError(f"factor must be positive, not {(fy, fx)}")
    if ny % fy or nx % fx:
        raise ValueError(f"factor {(fy, fx)} does not divide the grid: ny = {ny} over fy = {fy} leaves {ny % fy}, nx = {nx} over fx = {fx} "
                         f"leaves {nx % fx}")
    return fy, fx


def block_means(fine, weights, factor):
    """The rule in numpy: ``(coarse, wsum)`` of ``fine`` (..., ny, nx) with ``weights`` (broadcast against it; None: 1).  The order of
    the sums is numpy's, not the device's: equal to rounding, not bit for bit."""
    F = np.asarray(fine, dtype=np.float64)
    ny, nx = F.shape[-2:]
    fy, fx = check_factor(factor, ny, nx)
    w = np.ones(F.shape) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), F.shape)
    with np.errstate(invalid="ignore"):
        counts = (w > 0) & ~np.isnan(F)
    lead = F.shape[:-2]
    blocks = lambda a: a.reshape(lead + (ny // fy, fy, nx // fx, fx))
    with np.errstate(all="ignore"):
        wc = np.where(counts, w, 0.0)
        prod = np.where(counts, w * np.where(counts, F, 0.0), 0.0)
        wsum = blocks(wc).sum(axis=(-3, -1))
        coarse = np.where(wsum > 0, blocks(prod).sum(axis=(-3, -1)) / np.where(wsum > 0, wsum, 1.0), np.nan)
    return coarse, wsum


# ------------------------------------------------------------------------------------------------
# the call
# ------------------------------------------------------------------------------------------------
def _plan_lock(plan):
    with _PLAN_LOCKS_GUARD:
        return plan.__dict__.setdefault("_coarsen_lock", threading.Lock())


def _call(plan, lap, opts, token, W, nlev, f_staged, out_lead, fy, fx, device, want_wsum):
    """One library call on `plan`: the weights are set when the plan's last ones were another array's (token), then the call runs --
    both under the plan's lock here, so that another Filter's weights never slip in between."""
    ny, nx = plan.ny, plan.nx
    nbatch = int(np.prod(out_lead, dtype=np.int64))
    cshape = tuple(out_lead) + (ny // fy, nx // fx)
    if device is None:
        ptr, cur = _HOST_PTR, None
        outs = [np.empty(cshape, dtype=np.float64) for _ in range(2 if want_wsum else 1)]
    else:
        import torch
        ptr, cur = _DEVICE_PTR, torch.cuda.current_stream(device.index)
        outs = [torch.empty(cshape, dtype=torch.float64, device=device) for _ in range(2 if want_wsum else 1)]
    if nbatch:
        with _plan_lock(plan):
            if plan.__dict__.get("_coarsen_token", ("unset",)) != token:
                plan.__dict__["_coarsen_token"] = ("unset",)
                plan.set_coarsen_weights(W, nlev)
                plan.__dict__["_coarsen_token"] = token
            plan.apply_coarsen(opts.p, opts.shift(lap.is_dimensional), [ptr(f_staged)], [ptr(outs[0])], nbatch, fy, fx,
                               wsums=[ptr(outs[1])] if want_wsum else None, device_ptrs=device is not None,
                               stream=0 if cur is None else cur.cuda_stream, forward=opts.forward, backward_f32=opts.backward_f32,
                               mask_from_nan=opts.mask_from_nan, faces_from_nan=opts.faces_from_nan)
        _note_path(plan.last_path(), plan.device)
    elif want_wsum and device is None:
        outs[1][...] = 0.0
    return outs


def _run_plain(lap, f, opts, fy, fx, W, token, want_wsum):
    """2-D grid variables: one plan, one call (the flux kinds' flagged call where it is on offer, explicit masks per slice where not)."""
    shape = tuple(f.shape)
    ny, nx = shape[-2:]
    lead = shape[:-2]
    nbatch = int(np.prod(lead, dtype=np.int64))
    dtype = compute_dtype([f] + list(lap._planes))
    device = f.device if _on_gpu(f) else None
    gaps = opts.faces_from_nan and nbatch
    plan = None
    if not (gaps and (opts.forward or dtype != _lib.F64 or nx % 4)):
        plan = lap._plan(dtype, (ny, nx), None if device is None else device.index)
    if gaps and (plan is None or not plan.clenshaw_cut(int(opts.spec.n_steps), nbatch)):
        return _run_gap_fallback(lap, f, opts, fy, fx, W, token, want_wsum)
    staged, temporary = _stage(f, dtype, device)
    try:
        outs = _call(plan, lap, opts, token, W, 1, staged, lead, fy, fx, device, want_wsum)
    except _lib.GcmfError as e:
        if opts.faces_from_nan and _no_backward_cut(e):
            return _run_gap_fallback(lap, f, opts, fy, fx, W, token, want_wsum)
        raise _translate(e) from None
    if device is not None and temporary and nbatch:
        import torch
        staged.record_stream(torch.cuda.current_stream(device.index))
    return outs


def _run_gap_fallback(lap, f, opts, fy, fx, W, token, want_wsum):
    """faces_from_nan where the flagged call is not on offer: wet_mask * notnull(field) as a grid variable with the field's leading dims
    (kernels._gap_fallback), every slice coarsened with the one weight plane; the fine result is NaN in the gaps either way."""
    wm = lap._planes[0]
    if _is_torch(f):
        import torch
        w = wm if _is_torch(wm) else torch.as_tensor(np.asarray(wm))
        m = (~torch.isnan(f)).to(w.dtype) * w.to(f.device)
    else:
        w = wm.detach().cpu().numpy() if _is_torch(wm) else np.asarray(wm)
        m = (~np.isnan(np.asarray(f))).astype(w.dtype) * w
    with plan_cache_mode("off"):
        lap2 = type(lap)(m, *lap._planes[1:], _skip_kappa_one=True, _stack_levels=lap._stack_levels)
        return _run_levels(lap2, f, opts.without_faces(), fy, fx, W, token, want_wsum)


def _run_levels(lap, f, opts, fy, fx, W, token, want_wsum):
    """Grid variables with leading dims: the slice of index g of their broadcast leading shape is filtered with the grid of g and
    coarsened with the weight plane of g."""
    shape = tuple(f.shape)
    core = shape[-2:]
    glead = tuple(lap._glead)
    out_lead = tuple(np.broadcast_shapes(shape[:-2], glead))
    pad = len(out_lead) - len(glead)
    nbatch = int(np.prod(out_lead, dtype=np.int64))
    device = f.device if _on_gpu(f) else None
    per_level = W is not None and W.ndim > 2
    if lap._stacked and not (opts.forward or opts.mask_from_nan or opts.faces_from_nan) and out_lead[pad:] == glead:
        plan = lap._stacked_plan(None if device is None else device.index)
        if (plan.ny, plan.nx) != tuple(core):
            raise ValueError(f"field has spatial shape {tuple(core)} but the grid variables have shape {(plan.ny, plan.nx)}")
        if nbatch and plan.clenshaw_cut(int(opts.spec.n_steps), nbatch):
            staged, temporary = _stage(f, _lib.F64, device, out_lead + core)
            nlev = int(np.prod(glead, dtype=np.int64)) if per_level else 1
            Wl = np.ascontiguousarray(np.broadcast_to(W, glead + core)) if per_level else W
            try:
                outs = _call(plan, lap, CallOptions(spec=opts.spec), token, Wl, nlev, staged, out_lead, fy, fx, device, want_wsum)
            except _lib.GcmfError as e:
                raise _translate(e) from None
            if device is not None and temporary:
                import torch
                staged.record_stream(torch.cuda.current_stream(device.index))
            return outs
    full = (f.expand(*out_lead, *core) if _is_torch(f) else np.broadcast_to(f, out_lead + core))
    Wfull = np.broadcast_to(W, glead + core) if per_level else None
    outs = None
    for g, sub in lap._level_laps().items():
        idx = tuple([slice(None)] * pad + [slice(None) if n == 1 else i for i, n in zip(g, glead)])
        res = _run_plain(sub, full[idx], opts, fy, fx, np.ascontiguousarray(Wfull[g]) if per_level else W, token + (g,), want_wsum)
        if outs is None:
            cshape = out_lead + (core[0] // fy, core[1] // fx)
            if _is_torch(res[0]):
                import torch
                outs = [torch.empty(cshape, dtype=torch.float64, device=res[0].device) for _ in res]
            else:
                outs = [np.empty(cshape, dtype=np.float64) for _ in res]
        for o, r in zip(outs, res):
            o[idx] = r
    return outs


def _lead_of_grid(grid_vars):
    leads = [tuple(getattr(_unwrap(v), "shape", ()))[:-2] for v in grid_vars.values()]
    return tuple(np.broadcast_shapes(*leads)) if leads else ()


def _checked_weights(flt, weights, core):
    """`weights=` as float64 numpy of shape core or glead + core, and its token; validated once per array (the Filter remembers it)."""
    a = _unwrap(weights)
    fp = _fingerprint(a)
    hit = flt.__dict__.get("_coarsen_weights")
    if hit is not None and hit[0] == fp and hit[1] is weights:
        return hit[2], ("given", fp)
    W = np.ascontiguousarray(_host(a))
    glead = _lead_of_grid(flt.grid_vars)
    if tuple(W.shape) not in {tuple(core), glead + tuple(core)}:
        want = f"{tuple(core)}" + (f" or {glead + tuple(core)}" if glead else "")
        raise ValueError(f"weights have shape {tuple(W.shape)}, expected one plane {want}: the field's (y, x) shape"
                         + (", or planes with the grid variables' leading dims" if glead else ""))
    if np.isnan(W).any() or (W < 0).any():
        raise ValueError("weights must not be negative or NaN (0 keeps a cell out of the means)")
    flt.__dict__["_coarsen_weights"] = (fp, weights, W)
    return W, ("given", fp)


def _default_weights_of(flt):
    names = weight_names(flt.grid_type)
    key = tuple(_fingerprint(_unwrap(flt.grid_vars[n])) for n in names)
    hit = flt.__dict__.get("_coarsen_default")
    if hit is None or hit[0] != key:
        hit = (key, default_weights(flt.grid_type, flt.grid_vars))
        flt.__dict__["_coarsen_default"] = hit
    return hit[1], ("default",)


def apply_coarsened(flt, memo, opts, field, factor, weights, return_weights):
    """Filter.apply_coarsened behind its refusals of kinds of input: `memo` hands out the Laplacian of the Filter's grid variables."""
    given = field
    f = _unwrap(field)
    shape = tuple(f.shape)
    if len(shape) < 2:
        raise ValueError("fields need at least two (y, x) dimensions")
    ny, nx = shape[-2:]
    fy, fx = check_factor(factor, ny, nx)
    W, token = _default_weights_of(flt) if weights is None else _checked_weights(flt, weights, (ny, nx))
    if W is not None and tuple(W.shape[-2:]) != (ny, nx):
        raise ValueError(f"field has spatial shape {(ny, nx)} but the weights have shape {tuple(W.shape[-2:])}")
    with plan_cache_mode(flt.plan_cache):
        lap = memo.get([flt.grid_vars[n] for n in flt.Laplacian.required_grid_args()])
        opts.check(lap.GRID_TYPE, False)
        run = _run_plain if lap._glead is None else _run_levels
        outs = run(lap, f, opts, fy, fx, W, token, bool(return_weights))
    if _is_torch(f) and not _on_gpu(f):   # a host tensor in, host tensors out
        import torch
        outs = [torch.from_numpy(o) for o in outs]
    outs = [_same_kind(o, given) for o in outs]
    return (outs[0], outs[1]) if return_weights else outs[0]
