"""Subfilter covariances: the host side of ``Filter.apply_covariance`` (the device side is ``gcmf_apply_cov``, include/gcmf.h).

For a pair of fields and the filter ``F``::

    tau(f, g) = F(f g) - F(f) F(g)             (g = f: the subfilter variance)

The three applications of every pair run as ONE batch between two streaming passes on the device.  With ``nan_mask`` all three entries
share the gaps ``isnan(f) | isnan(g)`` -- three masks derived from three different sets of NaNs would not give a covariance.  The result
equals, bit for bit, the composition in float64 (``composition`` restates it with ``Filter.apply``): an entry has the same bits alone
and inside a batch, the product is rounded once, and the combine is a product and a difference, never a fused multiply-add.

Everything here stages arrays and picks the plan, as ``coarsen.py`` does for ``apply_coarsened``: 2-D grid variables run one library
call; grid variables with leading dims run the stacked plan's one call where ``apply`` would, and a plan and a call per level
otherwise.  Where ``GCMF_FACES_FROM_NAN`` is not on offer the explicit masks of the common gaps run as grid variables.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .kernels import (CallOptions, _DEVICE_PTR, _HOST_PTR, _is_torch, _no_backward_cut, _note_path, _on_gpu, _same_kind, _stage,
                      _translate, _unwrap, compute_dtype, plan_cache_mode)

__all__ = ["common_gaps", "composition"]


def common_gaps(f, g):
    """``(f', g')``: both fields with NaN wherever either is NaN (numpy or torch, the kind that came in)."""
    if _is_torch(f):
        import torch
        n = ~(torch.isnan(f) | torch.isnan(g))
        nan = torch.full((), float("nan"), dtype=f.dtype, device=f.device)
        return torch.where(n, f, nan), torch.where(n, g, nan.to(g.dtype))
    n = ~(np.isnan(f) | np.isnan(g))
    return np.where(n, f, np.nan), np.where(n, g, np.nan)


def composition(flt, f, g=None):
    """The specification of ``flt.apply_covariance(f, g)`` in numpy float64, from three ``flt.apply`` calls."""
    f = np.asarray(f, dtype=np.float64)
    g = f if g is None else np.asarray(g, dtype=np.float64)
    if flt.nan_mask:
        f, g = common_gaps(f, g)
    return flt.apply(f * g) - flt.apply(f) * flt.apply(g)


# ------------------------------------------------------------------------------------------------
# the call
# ------------------------------------------------------------------------------------------------
def _call(plan, lap, opts, f_staged, g_staged, out_lead, device):
    """One library call on `plan`: `npair` pairs of staged float64 planes (g_staged None: the variance)."""
    npair = int(np.prod(out_lead, dtype=np.int64))
    shape = tuple(out_lead) + (plan.ny, plan.nx)
    if device is None:
        ptr, cur, out = _HOST_PTR, None, np.empty(shape, dtype=np.float64)
    else:
        import torch
        ptr, cur, out = _DEVICE_PTR, torch.cuda.current_stream(device.index), torch.empty(shape, dtype=torch.float64, device=device)
    if npair:
        plan.apply_cov(opts.p, opts.shift(lap.is_dimensional), ptr(f_staged), None if g_staged is None else ptr(g_staged), ptr(out), npair,
                       device_ptrs=device is not None, stream=0 if cur is None else cur.cuda_stream, forward=opts.forward,
                       mask_from_nan=opts.mask_from_nan, faces_from_nan=opts.faces_from_nan)
        _note_path(plan.last_path(), plan.device)
    return out


def _keep_alive(device, staged):
    """The temporaries of a device call must outlive it on the caller's stream."""
    if device is not None:
        import torch
        cur = torch.cuda.current_stream(device.index)
        for t, temporary in staged:
            if temporary:
                t.record_stream(cur)


def _run_plain(lap, f, g, opts):
    """2-D grid variables: one plan, one call (the flux kinds' flagged call where it is on offer, explicit masks per slice where not)."""
    shape = tuple(f.shape)
    ny, nx = shape[-2:]
    lead = shape[:-2]
    npair = int(np.prod(lead, dtype=np.int64))
    entries = npair * (2 if g is None else 3)
    device = f.device if _on_gpu(f) else None
    gaps = opts.faces_from_nan and npair
    plan = None
    if not (gaps and (opts.forward or nx % 4)):
        plan = lap._plan(_lib.F64, (ny, nx), None if device is None else device.index)
    if gaps and (plan is None or not plan.clenshaw_cut(int(opts.spec.n_steps), entries)):
        return _run_gap_fallback(lap, f, g, opts)
    staged = [_stage(a, _lib.F64, device) for a in ((f,) if g is None else (f, g))]
    try:
        out = _call(plan, lap, opts, staged[0][0], None if g is None else staged[1][0], lead, device)
    except _lib.GcmfError as e:
        if opts.faces_from_nan and _no_backward_cut(e):
            return _run_gap_fallback(lap, f, g, opts)
        raise _translate(e) from None
    if npair:
        _keep_alive(device, staged)
    return out


def _run_gap_fallback(lap, f, g, opts):
    """faces_from_nan where the flagged call is not on offer: wet_mask * [neither field is NaN] as a grid variable with the fields'
    leading dims (kernels._gap_fallback, on the COMMON gaps), and the fields with those gaps put in; no flag is left on the call."""
    wm = lap._planes[0]
    if g is not None:
        f, g = common_gaps(f, g)
    if _is_torch(f):
        import torch
        w = wm if _is_torch(wm) else torch.as_tensor(np.asarray(wm))
        m = (~torch.isnan(f)).to(w.dtype) * w.to(f.device)
    else:
        w = wm.detach().cpu().numpy() if _is_torch(wm) else np.asarray(wm)
        m = (~np.isnan(np.asarray(f))).astype(w.dtype) * w
    with plan_cache_mode("off"):
        lap2 = type(lap)(m, *lap._planes[1:], _skip_kappa_one=True, _stack_levels=lap._stack_levels)
        return _run_levels(lap2, f, g, opts.without_faces())


def _run_levels(lap, f, g, opts):
    """Grid variables with leading dims: the pair of index i of their broadcast leading shape is filtered with the grid of i."""
    shape = tuple(f.shape)
    core = shape[-2:]
    glead = tuple(lap._glead)
    out_lead = tuple(np.broadcast_shapes(shape[:-2], glead))
    pad = len(out_lead) - len(glead)
    npair = int(np.prod(out_lead, dtype=np.int64))
    device = f.device if _on_gpu(f) else None
    if lap._stacked and not (opts.forward or opts.mask_from_nan or opts.faces_from_nan) and out_lead[pad:] == glead:
        plan = lap._stacked_plan(None if device is None else device.index)
        if (plan.ny, plan.nx) != tuple(core):
            raise ValueError(f"field has spatial shape {tuple(core)} but the grid variables have shape {(plan.ny, plan.nx)}")
        if npair and plan.clenshaw_cut(int(opts.spec.n_steps), npair * (2 if g is None else 3)):
            staged = [_stage(a, _lib.F64, device, out_lead + core) for a in ((f,) if g is None else (f, g))]
            try:
                out = _call(plan, lap, CallOptions(spec=opts.spec), staged[0][0], None if g is None else staged[1][0], out_lead, device)
            except _lib.GcmfError as e:
                raise _translate(e) from None
            _keep_alive(device, staged)
            return out
    full = lambda a: a.expand(*out_lead, *core) if _is_torch(a) else np.broadcast_to(a, out_lead + core)
    ff, gg = full(f), None if g is None else full(g)
    out = None
    for lev, sub in lap._level_laps().items():
        idx = tuple([slice(None)] * pad + [slice(None) if n == 1 else i for i, n in zip(lev, glead)])
        res = _run_plain(sub, ff[idx], None if gg is None else gg[idx], opts)
        if out is None:
            if _is_torch(res):
                import torch
                out = torch.empty(out_lead + core, dtype=torch.float64, device=res.device)
            else:
                out = np.empty(out_lead + core, dtype=np.float64)
        out[idx] = res
    return out


def check_pair(flt, field, other):
    """The refusals that need the arrays, all before any plan is made: (f, g) unwrapped, g None for the variance."""
    f = _unwrap(field)
    g = None if (other is None or other is field) else _unwrap(other)
    if g is not None and tuple(g.shape) != tuple(f.shape):
        raise ValueError(f"field and other must have the same shape, not {tuple(f.shape)} and {tuple(g.shape)}")
    if len(tuple(f.shape)) < 2:
        raise ValueError("fields need at least two (y, x) dimensions")
    planes = [_unwrap(flt.grid_vars[n]) for n in flt.Laplacian.required_grid_args()]
    if compute_dtype([f] + ([] if g is None else [g]) + planes) != _lib.F64:
        raise NotImplementedError("apply_covariance computes in float64 only: tau = F(fg) - F(f) F(g) is a small difference of large numbers, "
                                  "and float32 intermediates would leave little of it -- cast the fields (or the grid variables) to float64")
    return f, g


def apply_covariance(flt, memo, opts, field, f, g):
    """Filter.apply_covariance behind its refusals: `memo` hands out the Laplacian of the Filter's grid variables."""
    if g is not None and _on_gpu(f) != _on_gpu(g):     # one kind of memory for the call: the field's
        g = _stage(g, _lib.F64, f.device if _on_gpu(f) else None)[0]
    with plan_cache_mode(flt.plan_cache):
        lap = memo.get([flt.grid_vars[n] for n in flt.Laplacian.required_grid_args()])
        opts.check(lap.GRID_TYPE, False)
        out = (_run_plain if lap._glead is None else _run_levels)(lap, f, g, opts)
    if _is_torch(f) and not _on_gpu(f):   # a host tensor in, a host tensor out
        import torch
        out = torch.from_numpy(out)
    return _same_kind(out, field)
