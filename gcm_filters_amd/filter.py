"""``Filter`` -- drop-in for ``gcm_filters.Filter`` (reference gcm_filters/filter.py) on MI355X.

Host side (this file): the filter-polynomial fit (n_steps, s_max, Chebyshev coefficients p) and the
xarray / array front door.  Device side (libgcmf): the whole n_steps recurrence and the Laplacian stencils.
Names, signatures, defaults, exceptions and warnings follow the reference so that existing user code and
the reference's own tests read the same.
"""
from __future__ import annotations

import enum
import warnings
from dataclasses import dataclass, field
import os
import types
from typing import Any, Iterable, NamedTuple, Optional

import numpy as np

from .kernels import GAP_FOLD_GRID_TYPES, NAN_MASK_GRID_TYPES, PLAN_CACHE_MODES, plan_cache_mode, kernels_cache_enabled
from .kernels import last_path as kernels_last_path
from .kernels import (
    ALL_KERNELS,
    AreaWeightedMixin,
    BaseScalarLaplacian,
    BaseVectorLaplacian,
    CallOptions,
    GridType,
    _is_torch,
)

FilterShape = enum.Enum("FilterShape", ["GAUSSIAN", "TAPER"])

# coefficients of the default-n_steps rule, keyed [shape][ndim] (reference filter.py:28-37)
filter_params = {
    FilterShape.GAUSSIAN: {
        1: {"offset": 0.8, "factor": 0.0, "exponent": 1},
        2: {"offset": 1.1, "factor": 0.0, "exponent": 1},
    },
    FilterShape.TAPER: {
        1: {"offset": 2.2, "factor": 0.6, "exponent": 2.5},
        2: {"offset": 3.2, "factor": 0.7, "exponent": 2.7},
    },
}


class TargetSpec(NamedTuple):
    s_max: float
    filter_scale: float
    transition_width: float


class FilterSpec(NamedTuple):
    n_steps: int
    s_max: float
    p: Iterable[float]
    dx_min_sq: float


# ------------------------------------------------------------------------------------------------
# target transfer functions F(t), t in [-1, 1]  <->  s = k^2 = s_max (t + 1) / 2
# ------------------------------------------------------------------------------------------------
def _gaussian_target(target_spec: TargetSpec):
    """exp(-k^2 L^2 / 24) (reference filter.py:47-50)."""
    s_max, scale = target_spec.s_max, target_spec.filter_scale
    return lambda t: np.exp(-(s_max * (t + 1) / 2) * scale ** 2 / 24)


def _pchip_slopes(x, y):
    """Fritsch-Carlson monotone slopes with the three-point end formula SciPy's PchipInterpolator uses."""
    h = np.diff(x)
    m = np.diff(y) / h
    n = len(x)
    d = np.zeros(n)
    for k in range(1, n - 1):
        if m[k - 1] * m[k] > 0:
            w1, w2 = 2 * h[k] + h[k - 1], h[k] + 2 * h[k - 1]
            d[k] = (w1 + w2) / (w1 / m[k - 1] + w2 / m[k])

    def end(h0, h1, m0, m1):
        s = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
        if np.sign(s) != np.sign(m0):
            return 0.0
        if np.sign(m0) != np.sign(m1) and abs(s) > 3 * abs(m0):
            return 3 * m0
        return s

    d[0] = end(h[0], h[1], m[0], m[1])
    d[-1] = end(h[-1], h[-2], m[-1], m[-2])
    return d


def _pchip(x, y):
    """Piecewise-cubic Hermite interpolant through (x, y) with PCHIP slopes; returns a vectorised callable."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    d = _pchip_slopes(x, y)
    h = np.diff(x)
    m = np.diff(y) / h
    # local cubic  y_k + d_k s + c2 s^2 + c3 s^3,  s = q - x_k
    c2 = (3 * m - 2 * d[:-1] - d[1:]) / h
    c3 = (d[:-1] + d[1:] - 2 * m) / h ** 2

    def ev(q):
        q = np.asarray(q, dtype=float)
        k = np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)
        s = q - x[k]
        return y[k] + s * (d[k] + s * (c2[k] + s * c3[k]))

    return ev


def _taper_target(target_spec: TargetSpec):
    """1 for k <= 2 pi/(X L), 0 for k >= 2 pi/L, PCHIP in between (reference filter.py:53-65)."""
    s_max, scale, width = target_spec
    knots = [0, 2 * np.pi / (width * scale), 2 * np.pi / scale, 8 * np.sqrt(s_max)]
    fk = _pchip(knots, [1, 1, 0, 0])
    return lambda t: fk(np.sqrt((t + 1) * (s_max / 2)))


_target_function = {FilterShape.GAUSSIAN: _gaussian_target, FilterShape.TAPER: _taper_target}


def _compute_n_steps_default(ndim, filter_shape, filter_scale, dx_min, transition_width):
    """Default polynomial degree for 1-D / 2-D filters (reference filter.py:74-89)."""
    prm = filter_params[filter_shape][ndim]
    per_unit = prm["offset"] + prm["factor"] * ((np.pi / transition_width) ** prm["exponent"])
    return max(np.ceil(per_unit * (filter_scale / dx_min)).astype(int), 3)


def _cheb_T(x, n):
    """Rows T_0(x) .. T_n(x) by the three-term recurrence."""
    T = np.empty((n + 1, len(x)))
    T[0] = 1.0
    if n >= 1:
        T[1] = x
    for k in range(2, n + 1):
        T[k] = 2 * x * T[k - 1] - T[k - 2]
    return T


def _compute_filter_spec(filter_scale, dx_min, filter_shape, transition_width=np.pi, ndim=2, n_steps=0):
    """Chebyshev coefficients of the degree-n_steps polynomial that best fits the target on [-1, 1]
    subject to p(-1) = 1 (mean conservation) and p(1) = F(1)  (reference filter.py:99-151).

    Galerkin projection onto phi_i = T_i - T_{i+2} (Shen 1995) with Chebyshev-Gauss quadrature on
    n_steps + 1 nodes; the boundary values are carried by a linear lifting."""
    n = int(n_steps)
    s_max = ndim * (2 / dx_min) ** 2
    F = _target_function[filter_shape](TargetSpec(s_max, filter_scale, transition_width))
    # quadrature: x_q = cos(pi (2q - 1) / (2 (n + 1))), q = 1..n+1, equal weights pi / (n + 1)
    nq = n + 1
    xq = np.cos(np.pi * np.arange(1, 2 * nq, 2) / (2.0 * nq))
    wq = np.full(nq, np.pi / nq)
    T = _cheb_T(xq, n)
    F1 = F(np.asarray(1.0))
    resid = F(xq) - ((1 - xq) / 2 + F1 * (xq + 1) / 2)
    phi = T[: n - 1] - T[2: n + 1]
    b = (phi * (wq * resid)).sum(axis=1)
    # <phi_i, phi_j>_w : pi/2 (2 delta_ij - delta_{i,j+-2}), with the T_0 term doubling the (0,0) entry
    M = (np.pi / 2) * (2 * np.eye(n - 1) - np.diag(np.ones(n - 3), 2) - np.diag(np.ones(n - 3), -2))
    M[0, 0] = 3 * np.pi / 2
    c_hat = np.linalg.solve(M, b)
    p = np.zeros(n + 1)
    p[: n - 1] += c_hat          # + c_i T_i
    p[2:] -= c_hat               # - c_i T_{i+2}
    p[0] += (1 + F1) / 2         # lifting (1 - x)/2 + F(1)(1 + x)/2 in the Chebyshev basis
    p[1] -= (1 - F1) / 2
    return FilterSpec(n, s_max, p, dx_min ** 2)


# ------------------------------------------------------------------------------------------------
# the operator interface xarray.apply_ufunc calls (reference filter.py:154-291)
# ------------------------------------------------------------------------------------------------
def _make_run(filter_spec: FilterSpec, Laplacian, evaluation, plan_cache, **nan_flags):
    """The `run(fields, args, adjoint=False, like=None)` closure of the two factories below; the call's options are built HERE, once
    per factory -- a call constructs none.  The factory sets `run.func`, the function whose `last_path` a call updates."""
    forward = CallOptions(spec=filter_spec, forward=_forward_only(evaluation), backward_f32=evaluation == "backward", **nan_flags)
    adjoint_of = forward._replace(adjoint=True)
    memo = _LaplacianMemo(Laplacian)

    def run(fields, args, adjoint=False, like=None):
        with plan_cache_mode(plan_cache):
            out = memo.get(args)._run_with(fields, adjoint_of if adjoint else forward, like)   # (plan cached while the grid is unchanged)
        run.func.last_path = kernels_last_path()
        return out

    return run


def _create_filter_func(filter_spec: FilterSpec, Laplacian, evaluation: str = "auto", plan_cache=None, nan_mask=False):
    """Returns ``filter_func(field, *grid_args)``: first argument the field (last two axes = y, x; leading
    axes are independent batches), then the grid variables in ``Laplacian.required_grid_args()`` order.
    ``evaluation``, ``plan_cache``, ``nan_mask``: see ``Filter``."""
    # nan_mask="auto": per-slice masks by whichever route the library has for the kind -- mask bytes (the land-mask kinds) or face
    # coefficients (the flux-form kinds)
    faces = nan_mask == "auto" and Laplacian.GRID_TYPE in GAP_FOLD_GRID_TYPES
    run = _make_run(filter_spec, Laplacian, evaluation, plan_cache, mask_from_nan=bool(nan_mask) and not faces, faces_from_nan=faces)

    def filter_func(field, *args):
        assert len(args) == len(Laplacian.required_grid_args())
        if _wants_grad(field):   # a torch tensor that requires grad: the same call, with a grad_fn (the adjoint runs in backward)
            return _differentiable(_Operator(run, args), [field])[0]
        return run([field], args)[0]

    def adjoint_func(field, *args):
        """The transpose of filter_func applied to `field`."""
        assert len(args) == len(Laplacian.required_grid_args())
        return run([field], args, adjoint=True)[0]

    def adjoint_like_func(field, like, *args):
        """... with the forward input `like`: 0 where it is NaN, and its NaNs are the gaps of a nan_mask filter."""
        assert len(args) == len(Laplacian.required_grid_args())
        return run([field], args, adjoint=True, like=[like])[0]

    run.func = filter_func
    filter_func.last_path = None
    filter_func.adjoint, filter_func.adjoint_like = adjoint_func, adjoint_like_func
    filter_func.operator = lambda args: _Operator(run, args)
    return filter_func


# ------------------------------------------------------------------------------------------------
# torch autograd through the operator: F in forward, F^T (adjoint.py, gcmf_apply_adjoint) in backward
# ------------------------------------------------------------------------------------------------
def _wants_grad(*xs) -> bool:
    """A torch tensor that requires grad while autograd records: everything else -- numpy, xarray payloads, tensors that do not require
    grad, anything under torch.no_grad() -- takes exactly the path it took before there was a backward."""
    if not any(_is_torch(x) and x.requires_grad for x in xs):
        return False
    import torch
    return torch.is_grad_enabled()


class _Operator:
    """One filter (a factory's `run` closure and the grid arguments of a call) as the pair of linear maps autograd needs."""

    def __init__(self, run, args):
        self.run, self.args = run, args

    def forward(self, xs):
        return self.run(list(xs), self.args)

    def adjoint(self, gs, likes):
        return self.run(list(gs), self.args, adjoint=True, like=list(likes))


_AUTOGRAD = None


def _autograd():
    """The two torch.autograd.Functions, made on first use (torch is imported only when a tensor asks for a gradient).

    _Forward: y = F x; backward: x.grad = F^T g with like = x, the saved input itself (no copy).  _Adjoint: that backward as a
    Function of its own, so that it is differentiable in turn: it is linear in g, and its transpose is F again -- on the cells where
    `like` is finite, the only ones it reads or writes (gradgradcheck).  Neither has a derivative with respect to `like`: F is linear
    and its NaN pattern is not a differentiable thing."""
    global _AUTOGRAD
    if _AUTOGRAD is not None:
        return _AUTOGRAD
    import torch

    class _Forward(torch.autograd.Function):
        @staticmethod
        def forward(ctx, op, *xs):
            ctx.op = op
            ctx.save_for_backward(*xs)
            return tuple(op.forward([x.detach() for x in xs]))

        @staticmethod
        def backward(ctx, *gs):
            return (None,) + tuple(_Adjoint.apply(ctx.op, *gs, *ctx.saved_tensors))

    class _Adjoint(torch.autograd.Function):
        @staticmethod
        def forward(ctx, op, *gs_xs):
            n = len(gs_xs) // 2
            gs, xs = gs_xs[:n], gs_xs[n:]
            ctx.op = op
            ctx.save_for_backward(*xs)
            outs = op.adjoint([g.detach() for g in gs], [x.detach() for x in xs])
            # the gradient has the input's dtype and shape
            return tuple(o.to(x.dtype).reshape(x.shape) for o, x in zip(outs, xs))

        @staticmethod
        def backward(ctx, *hs):
            xs = ctx.saved_tensors
            gaps = [torch.isnan(x) for x in xs]
            # (F on h with the gaps of `like` -- a nan_mask filter derives its masks from them, any other reads them as 0 --, 0 on the gaps)
            ins = [torch.where(m, torch.full_like(h, float("nan")), h) for h, m in zip(hs, gaps)]
            outs = _differentiable(ctx.op, ins) if _wants_grad(*hs) else ctx.op.forward(ins)
            outs = [torch.where(m, torch.zeros_like(o), o) for o, m in zip(outs, gaps)]
            return (None,) + tuple(outs) + (None,) * len(xs)

    _AUTOGRAD = (_Forward, _Adjoint)
    return _AUTOGRAD


_BANK_FUNCTION = None


def _bank_function():
    """FilterBank.apply as a torch.autograd.Function: whichever route the forward takes, the backward is the plain sum over the scales
    of each filter's adjoint (no batched adjoint bank), every term differentiable in turn."""
    global _BANK_FUNCTION
    if _BANK_FUNCTION is None:
        import torch

        class _Bank(torch.autograd.Function):
            @staticmethod
            def forward(ctx, bank, args, x):
                ctx.bank, ctx.args = bank, args
                ctx.save_for_backward(x)
                return bank._bank_func(x.detach(), *args)

            @staticmethod
            def backward(ctx, g):
                (x,) = ctx.saved_tensors
                total = None
                for j, flt in enumerate(ctx.bank.filters):
                    op = flt._operator(_create_filter_func).operator(ctx.args)
                    term = _differentiable_adjoint(op, [g[j]], [x])[0]
                    total = term if total is None else total + term
                return None, None, total

        _BANK_FUNCTION = _Bank
    return _BANK_FUNCTION


def _differentiable(op, xs):
    """op.forward(xs) with a grad_fn."""
    return _autograd()[0].apply(op, *xs)


def _differentiable_adjoint(op, gs, likes):
    """op.adjoint(gs, likes) with a grad_fn (the gradient's dtype and shape are those of `likes`)."""
    return _autograd()[1].apply(op, *gs, *likes)


def _check_nan_mask(nan_mask, grid_type):
    """Filter's (and FilterBank's) check of ``nan_mask`` against the grid type."""
    if isinstance(nan_mask, str):
        if nan_mask != "auto":
            raise ValueError(f'nan_mask must be False, True or "auto", not {nan_mask!r}')
        if grid_type not in NAN_MASK_GRID_TYPES + GAP_FOLD_GRID_TYPES:
            raise ValueError(f'nan_mask="auto" needs one of the grid types '
                             f"{', '.join(g.name for g in NAN_MASK_GRID_TYPES + GAP_FOLD_GRID_TYPES)}, "
                             f"not {getattr(grid_type, 'name', grid_type)}")
    elif nan_mask and grid_type not in NAN_MASK_GRID_TYPES:
        raise ValueError(f"nan_mask=True needs one of the grid types {', '.join(g.name for g in NAN_MASK_GRID_TYPES)}, "
                         f"not {getattr(grid_type, 'name', grid_type)}")


def _create_filter_func_vec(filter_spec: FilterSpec, Laplacian, evaluation: str = "auto", plan_cache=None):
    """Returns ``filter_func_vec(u, v, *grid_args) -> (u_filtered, v_filtered)``."""
    run = _make_run(filter_spec, Laplacian, evaluation, plan_cache)

    def filter_func_vec(ufield, vfield, *args):
        assert len(args) == len(Laplacian.required_grid_args())
        if _wants_grad(ufield, vfield):
            if Laplacian.GRID_TYPE is GridType.VECTOR_B_GRID:   # (never a silent detach)
                raise NotImplementedError("VECTOR_B_GRID is not differentiable: its Laplacian has no diagonal symmetrizer, so the adjoint "
                                          "needs a transposed stencil kernel; detach() the fields to filter them without a gradient")
            import torch
            both = [x if _is_torch(x) else torch.as_tensor(np.asarray(x), device=y.device) for x, y in ((ufield, vfield), (vfield, ufield))]
            return tuple(_differentiable(_Operator(run, args), both))
        return tuple(run([ufield, vfield], args))

    def adjoint_func_vec(ufield, vfield, *args):
        """The transpose of filter_func_vec applied to (ufield, vfield)."""
        assert len(args) == len(Laplacian.required_grid_args())
        return tuple(run([ufield, vfield], args, adjoint=True))

    run.func = filter_func_vec
    filter_func_vec.last_path = None
    filter_func_vec.adjoint = adjoint_func_vec
    return filter_func_vec


class _LaplacianMemo:
    """The Laplacian object of the last call, reused while the caller passes the SAME grid arrays, unchanged: numpy planes are
    write-protected while their plan is cached (kernels.py: an edit raises), so "same object and still read-only" means
    unchanged; torch tensors carry a version counter.  Anything else -- other objects, a plane that is writable again (its
    plan left the cache), xarray wrappers -- takes the full path: a fresh Laplacian, fingerprints and validation like the
    reference's per-call construction (gcm_filters/filter.py:183).  Saves ~8 us per grid plane and call: what a small grid
    (BASELINE config 1: two 8-us launches) spends most of its time on."""

    def __init__(self, Laplacian):
        self.Laplacian = Laplacian
        self._entry = (None, None)    # (key, Laplacian object): ONE attribute, so that dask worker threads see a consistent pair

    @staticmethod
    def _token(a):
        if hasattr(a, "dims") and hasattr(a, "data"):    # an xarray.DataArray grid variable: its (numpy / torch) payload
            a = a.data
        if isinstance(a, np.ndarray):
            return None if a.flags.writeable else (id(a), 0)
        if _is_torch(a):
            return (id(a), a._version)
        return None

    def get(self, args):
        key = tuple(self._token(a) for a in args)
        have_key, have = self._entry
        if have is not None and key == have_key and None not in key and kernels_cache_enabled():
            return have
        lap = self.Laplacian(*args)
        key = tuple(self._token(a) for a in args)    # (construction write-protects host planes)
        self._entry = (key, lap) if None not in key else (None, None)
        return lap


EVALUATIONS = ("auto", "reference", "backward")


def _forward_only(evaluation: str) -> bool:
    if evaluation not in EVALUATIONS:
        raise ValueError(f"evaluation must be one of {EVALUATIONS}, not {evaluation!r}")
    return evaluation == "reference"


def _xarray():
    try:
        import xarray as xr
        return xr
    except ImportError:
        return None


def _is_bare_array(x) -> bool:
    return (isinstance(x, np.ndarray) or _is_torch(x) or hasattr(x, "__cuda_array_interface__")
            or (hasattr(x, "__dlpack__") and not hasattr(x, "dims")))


@dataclass
class Filter:
    """A class for applying diffusion-based smoothing filters to gridded data.

    Parameters
    ----------
    filter_scale : float
        The filter scale, which has different meaning depending on filter shape
    dx_min : float
        The smallest grid spacing. Should have same units as ``filter_scale``
    n_steps : int, optional
        Number of total steps in the filter (``0``: chosen automatically)
    filter_shape : FilterShape
        ``GAUSSIAN``: target :math:`e^{-(k L)^2/24}`; ``TAPER``: sharp cut-off at scale L
    transition_width : float, optional
        Width of the transition region of the Taper filter (> 1)
    ndim : int, optional
        Dimension of the grid the Laplacian acts on
    grid_type : GridType
    grid_vars : dict
        Grid variables required by ``grid_type`` (see ``required_grid_vars``); xarray DataArrays, numpy
        arrays or torch tensors (host or MI355X-resident); planes (y, x) or with leading level / time dims
    evaluation : {"auto", "reference", "backward"}, keyword only (not a field of the reference class)
        How the filter polynomial is summed.  ``"reference"``: the reference's forward Chebyshev recurrence with its
        accumulation scheme -- for float32 fields a float32 recurrence and a float64 running sum (NumPy >= 2 promotion,
        gcm_filters/filter.py:192-206); BIT-EXACT with numpy on the REGULAR / land-mask / B-grid types, and the path that
        reproduces the reference's NaN / inf pattern around a non-finite value in a wet cell.
        ``"auto"`` (default): the same polynomial by Clenshaw's backward recurrence (two state planes, fused multiply-adds)
        wherever that is at least as close to float64 arithmetic as the reference's own path for the dtype:
        every float64 field (<= 1e-14 from numpy; flux-form grids <= 3e-15 from the forward result) and float32 VECTOR_C_GRID fields
        (carried in float32 in Reinsch's form of the recurrence: 0.55-0.6 x the error of the reference's float32 path, e.g.
        1.8e-6 instead of 3.2e-6 at n_steps 44).  float32 scalar and VECTOR_B_GRID fields take the forward recurrence (round 5):
        summed backwards in float32 they are 15-45 x (B-grid 2-3 x) further from float64 arithmetic than the reference is.
        ``"backward"``: backward evaluation for those too -- 1.1-1.5 x faster, all float32 (e.g. 9.5e-6 instead of 2.1e-7 on
        IRREGULAR_WITH_LAND at n_steps 98; inside SURVEY 8d's 1e-4 for float32).  The result is float64 in every case.
    plan_cache : {None, "protect", "verify", "off"}, keyword only (not a field of the reference class)
        The reference builds (and validates) a fresh Laplacian on every call (gcm_filters/filter.py:183); here the folded grid lives in
        HBM as a *plan* that is reused while the grid arrays are unchanged.  ``"protect"`` (the default, also ``None`` unless the
        environment says otherwise): the numpy grid arrays are made READ-ONLY while their plan is cached -- an in-place edit such as
        ``wet_mask[10, 10] = 0`` raises ``ValueError: assignment destination is read-only`` instead of silently filtering with stale
        coefficients; call ``gcm_filters_amd.kernels.clear_plan_cache()`` (or drop the Filter and its arrays) to get writability back.
        ``"verify"``: the arrays stay writable and every plane is hashed on every call (~5 ms per 2400 x 3600 plane): edits between
        calls just work, as with the reference.  ``"off"``: a fresh plan per call, exactly the reference's behaviour (~10 ms per
        call at 2400 x 3600).  Process-wide defaults: ``GCMF_PLAN_CACHE=0`` (off), ``GCMF_PLAN_CACHE_VERIFY=full`` (verify).
    nan_mask : bool, keyword only (not a field of the reference class)
        Fields with gaps that differ from one 2-D slice to the next (satellite products, model output with NaN below the sea floor).
        ``False`` (default): the reference's behaviour -- the stencil reads a NaN in a wet cell through ``nan_to_num``, i.e. as the
        VALUE 0, which bleeds into every neighbour within the filter scale; only the gap cell itself comes out NaN.  ``True``: every
        2-D slice ``b`` of the field is filtered with its own wet mask ``m_b = wet_mask * notnull(field_b)``, derived on the device
        inside the batched launches -- the result of the reference's ``filter_func`` with ``wet_mask`` replaced by ``m_b`` (no flux
        across a gap), bit for bit what handing ``wet_mask(n, y, x) = wet_mask * notnull(field)`` in as a grid variable gives, without
        one plan per slice.  The output is NaN exactly where the input is; +-inf is data, not a gap; a slice without NaN gives the bits
        of ``nan_mask=False``.  Only for ``REGULAR_WITH_LAND``, ``REGULAR_WITH_LAND_AREA_WEIGHTED`` and
        ``TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED`` (``ValueError`` otherwise); ``last_path`` is ``"strips"``.
        ``"auto"``: the same contract wherever the library has per-slice masks -- on those three grid types it is ``True``'s route, on
        ``IRREGULAR_WITH_LAND``, ``MOM5U`` and ``MOM5T`` every slice's FACE coefficients are folded on the device from the plan's own
        and the slice's NaNs inside the call (``GCMF_FACES_FROM_NAN``: one streaming pass, 25 bytes of scratch per cell and slice, no
        plan build), bit for bit what the stacked plan of ``wet_mask(n, y, x) = wet_mask * notnull(field)`` gives.  Where that call is
        not on offer -- ``evaluation="reference"``, float32 grids, ``nx % 4 != 0``, polynomials without a backward cut -- the masks are
        built here and run as grid variables with a leading axis: the same contract, slower.  ``ValueError`` on the other five grid
        types, and for any other string.

    Beyond ``apply`` and ``apply_to_vector`` (none of these is in the reference class): ``adjoint``, ``apply_coarsened`` (filter, then
    weighted block means) and ``apply_covariance(field, other=None)`` -- the subfilter covariance ``F(f g) - F(f) F(g)`` of two scalar
    fields (``other=None``: the variance) in one call, float64, bit for bit the composition of three ``apply`` calls, with the gaps of
    a ``nan_mask`` filter taken from both fields together.

    Attributes
    ----------
    filter_spec: FilterSpec
    """

    filter_scale: float
    dx_min: float
    filter_shape: FilterShape = FilterShape.GAUSSIAN
    transition_width: float = np.pi
    ndim: int = 2
    n_steps: int = 0
    grid_type: GridType = GridType.REGULAR
    grid_vars: dict = field(default_factory=dict, repr=False)
    evaluation: str = field(default="auto", kw_only=True, repr=False)   # extension, see the docstring
    plan_cache: Optional[str] = field(default=None, kw_only=True, repr=False)   # extension, see the docstring
    nan_mask: Any = field(default=False, kw_only=True, repr=False)   # False / True / "auto": extension, see the docstring

    # Same fields, defaults, attribute names (Laplacian, filter_spec, n_steps, grid_ds) and exception / warning texts as
    # the reference class (gcm_filters/filter.py:294-393): they are the contract its users and tests rely on.  The
    # bodies below are this package's own.
    def __post_init__(self):
        self.Laplacian = ALL_KERNELS[self.grid_type]
        _forward_only(self.evaluation)   # ValueError for anything else
        if self.plan_cache is not None and self.plan_cache not in PLAN_CACHE_MODES:
            raise ValueError(f"plan_cache must be one of {PLAN_CACHE_MODES} or None, not {self.plan_cache!r}")
        _check_nan_mask(self.nan_mask, self.grid_type)
        self._reject_bad_arguments()
        self.n_steps = self._choose_n_steps()
        self.filter_spec = _compute_filter_spec(self.filter_scale, self.dx_min, self.filter_shape, self.transition_width,
                                                self.ndim, self.n_steps)
        wanted, given = self.Laplacian.required_grid_args(), list(self.grid_vars)
        if set(wanted) != set(given):
            raise ValueError(f"Provided `grid_vars` {given} do not match expected {wanted}")
        self.grid_ds = self._bundle_grid_vars()

    def _reject_bad_arguments(self):
        fixed_factor = issubclass(self.Laplacian, AreaWeightedMixin)
        if fixed_factor and self.dx_min != 1:
            raise ValueError("Provided Laplacian is for simple fixed factor filtering, "
                             "where transformed field is filtered on a regular grid with dx = dy = 1. "
                             "dx_min must be set to 1.")
        if not self.transition_width > 1:
            raise ValueError("Transition width must be > 1.")
        if self.ndim > 2 and self.n_steps < 3:
            raise ValueError("When ndim > 2, you must set n_steps manually")

    def _choose_n_steps(self):
        """The caller's n_steps when it asks for at least 3 steps, else the default rule (1-D / 2-D only)."""
        asked = self.n_steps
        if self.ndim > 2:
            return asked
        default = _compute_n_steps_default(self.ndim, self.filter_shape, self.filter_scale, self.dx_min,
                                           self.transition_width)
        if asked < 3:
            return default
        if asked < default:
            warnings.warn("You have set n_steps below the default. Results might not be accurate.", stacklevel=4)
        return asked

    def _bundle_grid_vars(self):
        """An ``xarray.Dataset`` when every grid variable is an xarray object (what ``apply`` feeds apply_ufunc from),
        a plain dict otherwise (bare numpy / torch arrays)."""
        xr = _xarray()
        if xr is not None and self.grid_vars and all(isinstance(v, (xr.DataArray, xr.Variable)) for v in self.grid_vars.values()):
            return xr.Dataset(dict(self.grid_vars))
        return dict(self.grid_vars)

    # -- the target and its polynomial, for inspection -------------------------------------------
    def plot_shape(self, ax=None):
        """Plot the shape of the target filter and approximation."""
        import matplotlib.pyplot as plt

        spec = self.filter_spec
        target = _target_function[self.filter_shape](TargetSpec(spec.s_max, self.filter_scale, self.transition_width))
        t = np.linspace(-1.0, 1.0, 10001)
        wavenumber = np.sqrt(0.5 * spec.s_max * (t + 1.0))
        fitted = np.asarray(spec.p) @ _cheb_T(t, spec.n_steps)
        cutoff = 2 * np.pi / self.filter_scale
        if ax is None:
            ax = plt.subplots()[1]
        for curve, style, label in ((target(t), "g", "target filter"), (fitted, "m", "approximation")):
            ax.plot(wavenumber, curve, style, label=label, linewidth=4)
        ax.axvline(cutoff, color="k", label="filter cutoff wavenumber", linewidth=2)
        right = 2 * cutoff if self.filter_scale / self.dx_min > 10 else None   # zoom in on strong filters
        ax.set_xlim(left=0, right=right)
        ax.set_ylim(bottom=-0.1, top=1.1)
        ax.set_xlabel("Wavenumber k", fontsize=18)
        ax.grid(True)
        ax.legend()
        return ax

    # -- applying the filter ---------------------------------------------------------------------
    def _grid_args(self, as_xarray: bool):
        names = self.Laplacian.required_grid_args()
        if not as_xarray:
            return [self.grid_vars[n] for n in names]
        if isinstance(self.grid_ds, dict):
            bare = [n for n in names if not hasattr(self.grid_ds[n], "dims")]
            if bare:
                raise TypeError(f"grid_vars {bare} must be xarray DataArrays to filter xarray objects")
        return [self.grid_ds[n] for n in names]

    def _through_apply_ufunc(self, func, fields, dims, extra=()):
        """The one call into ``xarray.apply_ufunc`` (reference filter.py:478-486, 518-527): every field and grid
        variable has ``dims`` as core dims (moved last), one output per field, same keywords as upstream so that lazy
        (dask) inputs keep working: ``dask="parallelized"`` then calls ``func`` from worker threads, block by block.
        extra: operands handed to ``func`` between the fields and the grid variables (the adjoint's ``like``)."""
        xr = _xarray()
        if xr is None:
            raise ImportError("xarray is required to filter xarray objects; pass numpy arrays or torch tensors instead")
        assert len(dims) == 2
        operands = list(fields) + list(extra) + self._grid_args(as_xarray=True)
        return xr.apply_ufunc(
            func,
            *operands,
            input_core_dims=len(operands) * [dims],
            output_core_dims=[dims] if len(fields) == 1 else len(fields) * [dims],
            output_dtypes=[f.dtype for f in fields],
            dask="parallelized",
        )

    def _operator(self, make):
        """``make(filter_spec, Laplacian, evaluation)`` (one of the two factories above), built once per Filter: the closure
        remembers the Laplacian object of its last call (_LaplacianMemo)."""
        key = (make, id(self.filter_spec), self.Laplacian, self.evaluation, self.plan_cache, self.nan_mask if isinstance(self.nan_mask, str) else bool(self.nan_mask))
        hit = self.__dict__.get("_op")
        if hit is None or hit[0] != key:
            extra = {} if self.plan_cache is None else {"plan_cache": self.plan_cache}
            if self.nan_mask:
                extra["nan_mask"] = self.nan_mask if isinstance(self.nan_mask, str) else True
            hit = (key, make(self.filter_spec, self.Laplacian, self.evaluation, **extra))
            self.__dict__["_op"] = hit
        return hit[1]

    @property
    def last_path(self):
        """Which of the library's bit-identical paths this Filter's last application took (not in the reference, which has one numpy
        path): ``"resident"`` -- the whole polynomial in one on-chip launch (small grids); ``"strips"`` -- the strip-marching launches;
        ``"resident-lock-busy"`` -- strips, because another process holds this GPU's on-chip lock (a ``RuntimeWarning`` says so once per
        process); ``"resident-disabled"`` -- strips, because an on-chip launch of this process timed out earlier;
        ``"host-row-blocks"`` -- a large host array streamed through row blocks; ``None`` before the first call."""
        hit = self.__dict__.get("_op")
        return None if hit is None else getattr(hit[1], "last_path", None)

    def apply(self, ds, dims=None):
        """Filter an ``xarray.DataArray`` / ``xarray.Dataset`` with a scalar Laplacian across ``dims``
        (two names, latitude-like dimension first).

        Extension: a bare ``numpy.ndarray`` or ``torch.Tensor`` (``dims`` omitted) is filtered over its
        last two axes (y, x), leading axes being independent batches -- exactly what ``apply_ufunc`` hands
        to ``filter_func``; an MI355X-resident tensor is filtered in HBM and returned as a tensor.
        """
        if issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a vector Laplacian. "
                             f"The ``.apply`` method is only suitable for scalar Laplacians.")
        filter_func = self._operator(_create_filter_func)
        if _is_bare_array(ds):
            return filter_func(ds, *self._grid_args(as_xarray=False))
        xr = _xarray()
        if xr is None or not isinstance(ds, xr.Dataset):
            return self._through_apply_ufunc(filter_func, [ds], dims)
        # a Dataset: every variable that has both dims is filtered, the others are carried along untouched
        result = ds.copy(deep=True)
        hits = [name for name, var in result.variables.items() if set(dims) <= set(var.dims)]
        for name in hits:
            result[name] = self._through_apply_ufunc(filter_func, [result.variables[name]], dims)
        if not hits:
            warnings.warn(f"No variables in the dataset had all of the given dimensions ({dims}), so nothing was filtered.",
                          stacklevel=2)
        return result

    def apply_to_vector(self, ufield, vfield, dims=None):
        """Filter a vector field (u, v) with a vector Laplacian across ``dims``; bare arrays as in ``apply``."""
        if not issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a scalar Laplacian. "
                             f"The ``.apply_to_vector`` method is only suitable for vector Laplacians.")
        filter_func_vec = self._operator(_create_filter_func_vec)
        if _is_bare_array(ufield) and _is_bare_array(vfield):
            return filter_func_vec(ufield, vfield, *self._grid_args(as_xarray=False))
        u_filtered, v_filtered = self._through_apply_ufunc(filter_func_vec, [ufield, vfield], dims)
        return (u_filtered, v_filtered)

    # -- filter, then coarse-grain (not in the reference) --------------------------------------------
    def apply_coarsened(self, field, factor, dims=None, weights=None, return_weights=False):
        """``apply``, then one weighted mean per block of ``factor`` cells -- "smooth the 0.1 degree field to 1 degree, then keep one value
        per 1 degree box" in one call (``gcmf_apply_coarsen``): the fine result never leaves the device, and a numpy caller gets back
        only the coarse planes.

        ``factor``: an int, or ``(fy, fx)``; each must divide its grid length (``ValueError`` gives both lengths).  ``field``: numpy, a
        torch tensor (host or MI355X-resident) or a DLPack / ``__cuda_array_interface__`` array, filtered over its last two axes with
        any leading dims; the same kind comes back, of shape ``lead + (ny / fy, nx / fx)`` and dtype float64.  ``dims`` is accepted for
        symmetry with ``apply`` and not used.

        The rule (``gcm_filters_amd.coarsen``): a cell counts where its weight is > 0 and the filtered value is not NaN (+-inf is data);
        a block's value is the sum of ``weight * value`` over its counted cells over the sum of their weights -- NaN where no cell
        counts.  Cells that do not count are skipped, never multiplied, so neither the finite junk ``apply`` leaves on land nor the gaps
        of a ``nan_mask`` filter reach a mean.  The sums run in float64 in one fixed order: the bits of a block do not depend on the
        batch, on where the arrays lie or on whether they are host or device arrays.

        ``weights``: ``None`` -- the grid's own: 1 (``REGULAR``), ``wet_mask`` (``REGULAR_WITH_LAND``), ``area``
        (``REGULAR_AREA_WEIGHTED``), and the cell area times ``wet_mask`` on the other scalar grid types (``area``, ``area_u``,
        ``area_t``, ``tarea``), with the level axis of grid variables that have leading dims --, or one plane (y, x), or planes with
        the grid variables' leading dims; negative or NaN entries raise ``ValueError``.  The weights go to the device once per
        weights array (and plan), not once per call: to change them pass another array, not the same one edited in place.
        ``return_weights=True`` returns ``(coarse, wsum)``, ``wsum`` being the blocks' sums of counted weights (0 where ``coarse`` is NaN).

        ``evaluation``, ``plan_cache`` and ``nan_mask`` carry over from the Filter.  ``NotImplementedError``: xarray objects (the core
        dims shrink: pass ``.data`` and re-wrap the result), tensors that require grad (``detach()`` them, or coarsen ``apply``'s
        result with torch to keep the gradient), and vector grid types."""
        if issubclass(self.Laplacian, BaseVectorLaplacian):
            raise NotImplementedError(f"{self.grid_type.name} is a vector grid type: apply_coarsened coarsens scalar fields only; filter "
                                      f"with apply_to_vector and coarsen each component on the scalar grid of its points")
        if hasattr(field, "dims") and not _is_torch(field) and not isinstance(field, np.ndarray):
            raise NotImplementedError("apply_coarsened does not take xarray objects (the core dims of the result are shorter than the "
                                      "input's): pass the array itself, `field.data`, with (y, x) as its last two axes, and wrap the result")
        if _wants_grad(field):
            raise NotImplementedError("apply_coarsened has no backward: pass `field.detach()` to coarsen without a gradient, or call "
                                      "apply() -- which is differentiable -- and take the block means with torch")
        from . import coarsen
        if not _is_bare_array(field):
            field = np.asarray(field)
        hit = self.__dict__.get("_coarsen_memo")
        if hit is None:
            hit = self.__dict__["_coarsen_memo"] = _LaplacianMemo(self.Laplacian)
        faces = self.nan_mask == "auto" and self.grid_type in GAP_FOLD_GRID_TYPES
        opts = CallOptions(spec=self.filter_spec, forward=_forward_only(self.evaluation), backward_f32=self.evaluation == "backward",
                           mask_from_nan=bool(self.nan_mask) and not faces, faces_from_nan=faces)
        out = coarsen.apply_coarsened(self, hit, opts, field, factor, weights, return_weights)
        self._operator(_create_filter_func).last_path = kernels_last_path()
        return out

    # -- subfilter covariances (not in the reference) ------------------------------------------------
    def apply_covariance(self, field, other=None, dims=None):
        """The subfilter (eddy) covariance ``tau(f, g) = F(f g) - F(f) F(g)`` of ``field`` and ``other`` in one call
        (``gcmf_apply_cov``); ``other=None`` is the subfilter variance ``F(f f) - F(f) F(f)``.  Eddy kinetic energy is
        ``(tau(u, u) + tau(v, v)) / 2``; eddy fluxes and subgrid forcings are covariances, too.

        ``field``, ``other``: numpy, torch tensors (host or MI355X-resident) or DLPack / ``__cuda_array_interface__`` arrays of one
        shape, filtered over their last two axes with any leading dims; the kind of ``field`` comes back, float64, of the shape
        ``apply`` would return.  ``dims`` is accepted for symmetry with ``apply`` and not used.

        The three applications of every pair run as one batch on the device between two streaming passes, and the result equals, bit
        for bit, ``apply(f * g) - apply(f) * apply(g)`` computed in float64 (``gcm_filters_amd.covariance.composition``).  With
        ``nan_mask`` all three share the gaps ``isnan(field) | isnan(other)``: the result is NaN exactly where either field is, and
        it is the composition on the two fields with those common gaps put in -- three masks from three sets of NaNs would not give a
        covariance.  ``evaluation``, ``plan_cache`` and ``nan_mask`` carry over from the Filter.

        ``ValueError``: the two differ in shape, or have fewer than two dims.  ``NotImplementedError``: xarray objects (pass
        ``.data`` and re-wrap the result), tensors that require grad (``detach()`` them, or compose the covariance from ``apply``,
        which is differentiable), vector grid types (take the covariance of each component on the scalar grid of its points), and a
        float32 compute dtype -- float32 fields with float32 grid variables: cast to float64, tau being a small difference of large
        numbers."""
        if issubclass(self.Laplacian, BaseVectorLaplacian):
            raise NotImplementedError(f"{self.grid_type.name} is a vector grid type: apply_covariance takes scalar fields only; take the "
                                      f"covariance of each component on the scalar grid type of its points")
        for a in (field, other):
            if hasattr(a, "dims") and not _is_torch(a) and not isinstance(a, np.ndarray):
                raise NotImplementedError("apply_covariance does not take xarray objects: pass the arrays themselves, `field.data` and "
                                          "`other.data`, with (y, x) as their last two axes, and wrap the result")
            if _wants_grad(a):
                raise NotImplementedError("apply_covariance has no backward: pass `field.detach()` (and `other.detach()`), or compose "
                                          "apply(f * g) - apply(f) * apply(g) from apply(), which is differentiable")
        from . import covariance
        if not _is_bare_array(field):
            field = np.asarray(field)
        if other is not None and not _is_bare_array(other):
            other = np.asarray(other)
        f, g = covariance.check_pair(self, field, other)
        hit = self.__dict__.get("_coarsen_memo")
        if hit is None:
            hit = self.__dict__["_coarsen_memo"] = _LaplacianMemo(self.Laplacian)
        faces = self.nan_mask == "auto" and self.grid_type in GAP_FOLD_GRID_TYPES
        opts = CallOptions(spec=self.filter_spec, forward=_forward_only(self.evaluation), mask_from_nan=bool(self.nan_mask) and not faces,
                           faces_from_nan=faces)
        out = covariance.apply_covariance(self, hit, opts, field, f, g)
        self._operator(_create_filter_func).last_path = kernels_last_path()
        return out

    # -- the adjoint (not in the reference) --------------------------------------------------------
    def adjoint(self, field, dims=None, like=None):
        """Apply the TRANSPOSE of ``apply`` to ``field`` (a gradient with respect to the filtered field, say): ``F^T field``, where
        ``F`` is the linear map ``apply`` is on finite fields.  No transposed stencil runs: ``F^T = D F D^-1`` with a diagonal ``D``
        made of the grid's cell areas (``gcm_filters_amd.adjoint``), so the cost is one application plus two plane passes.

        Inputs as for ``apply`` -- numpy, torch (host or MI355X-resident), DLPack producers, ``xarray`` objects with ``dims`` -- and the
        same kind comes out; ``evaluation``, ``plan_cache``, ``nan_mask`` and grid variables with leading dims carry over.

        ``like``: the input the forward ``apply`` was given (same kind and shape as ``field``).  Only its NaN pattern is read: where it
        is NaN the result is 0, because a NaN input cell has no derivative.  ``Filter(nan_mask=...)`` requires it (``ValueError``
        without): its NaNs are the gaps the per-slice masks are made of.  The precision is the forward call's: with ``like`` given, the
        data type of ``like`` and the grid variables decides between a float32 and a float64 plan, not that of ``field``.

        ``torch`` tensors that require grad need none of this: ``apply`` returns a tensor with a ``grad_fn`` whose backward is this
        method with ``like`` = the input (and is differentiable in turn)."""
        if issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a vector Laplacian. "
                             f"The ``.adjoint`` method is only suitable for scalar Laplacians.")
        if self.nan_mask and like is None:
            raise ValueError("Filter(nan_mask=...).adjoint needs `like`, the field the forward apply() was given: its NaNs are the gaps "
                             "each slice's wet mask is made of")
        filter_func = self._operator(_create_filter_func)
        if _is_bare_array(field):
            if like is None:
                return filter_func.adjoint(field, *self._grid_args(as_xarray=False))
            return filter_func.adjoint_like(field, like, *self._grid_args(as_xarray=False))
        xr = _xarray()
        if xr is not None and isinstance(field, xr.Dataset):
            raise TypeError("Filter.adjoint takes one DataArray at a time: pass the Dataset's variables one by one")
        if like is None:
            return self._through_apply_ufunc(filter_func.adjoint, [field], dims)
        return self._through_apply_ufunc(filter_func.adjoint_like, [field], dims, extra=[like])

    def adjoint_to_vector(self, ufield, vfield, dims=None):
        """Apply the transpose of ``apply_to_vector`` to the pair (ufield, vfield); inputs and outputs as there.  ``VECTOR_C_GRID``
        only: ``VECTOR_B_GRID`` raises ``NotImplementedError`` (its Laplacian has no diagonal symmetrizer)."""
        if not issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a scalar Laplacian. "
                             f"The ``.adjoint_to_vector`` method is only suitable for vector Laplacians.")
        if self.grid_type is GridType.VECTOR_B_GRID:
            raise NotImplementedError("VECTOR_B_GRID has no adjoint: its Laplacian has no diagonal symmetrizer D with L^T = D L D^-1; "
                                      "it needs a transposed stencil kernel")
        adjoint_vec = self._operator(_create_filter_func_vec).adjoint
        if _is_bare_array(ufield) and _is_bare_array(vfield):
            return adjoint_vec(ufield, vfield, *self._grid_args(as_xarray=False))
        u_adj, v_adj = self._through_apply_ufunc(adjoint_vec, [ufield, vfield], dims)
        return (u_adj, v_adj)


def _bank_by_default(nbank: int, ny: int, nx: int, grid_type=None) -> bool:
    """Whether FilterBank takes the one-batch route where the library offers it and GCMF_FILTER_BANK does not say: wherever
    tools/measure_filter_bank.py measured it at least as fast as the loop over the scales beyond both spreads (README, "Filter banks")."""
    if grid_type == GridType.TRIPOLAR_POP_WITH_LAND:
        # measured (tools/measure_filter_bank.py --pop; README "One field at many scales"): 2 .. 32 scales on 384 x 320, 1080 x 1440 and
        # 2400 x 3600, 56 and 63 steps -- the bank won every row beyond both spreads (20 % .. 92 % less time).  Between those rows the
        # default goes by cells x scales; outside the measured range the loop stays the default (GCMF_FILTER_BANK=1 still asks for the bank)
        return _POP_BANK_RANGE[0] <= int(nbank) * int(ny) * int(nx) <= _POP_BANK_RANGE[1]
    return True


# FilterBank(nan_mask="auto") on the flux-form kinds: whether the one-batch route (gcmf_apply_bank_gaps) is the default, by the rule of
# DESIGN.md 6 -- only where it was measured faster than the loop beyond both spreads (tools/measure_filter_bank.py --gaps)
_GAPS_BANK_BY_DEFAULT = True

_POP_BANK_RANGE = (2 * 384 * 320, 32 * 2400 * 3600)      # cells x scales: the smallest and the largest measured row


class FilterBank:
    """One field filtered at many scales: the ``Filter`` objects of a sweep over ``filter_scales`` sharing everything else -- shape,
    ``dx_min``, grid, and ONE polynomial degree -- applied in one call (not in the reference, whose users loop over ``Filter`` objects).

    ``s_max`` does not depend on the filter scale, so the operator of every scale is the same and only the Chebyshev coefficients
    differ: on float64 ``IRREGULAR_WITH_LAND`` / ``MOM5U`` / ``MOM5T`` / ``TRIPOLAR_POP_WITH_LAND`` grids the scales run as ONE batch of the
    backward evaluation with a polynomial per entry (``gcmf_apply_bank``; on the tripolar grid the plain strips below the seam and
    ``k_fold_band``'s per-entry form on its rows); everything else runs ``filters[j]`` one after the other.  Either way
    ``bank.apply(f)[j]`` is what ``bank.filters[j].apply(f)`` returns.

    Parameters
    ----------
    filter_scales : sequence of float
        The filter scales, positive and finite (``ValueError`` otherwise, and for an empty sequence)
    n_steps : int, optional
        One degree for all scales: the largest of ``Filter``'s default ``n_steps`` over the scales; a caller's ``n_steps >= 3`` is taken
        instead (with ``Filter``'s warning when it is below that largest default)
    dx_min, filter_shape, transition_width, ndim, grid_type, grid_vars, evaluation, plan_cache
        As for ``Filter``, validated as ``Filter`` validates them
    nan_mask : bool or "auto", keyword only
        As for ``Filter`` (same values, same grid types, same messages), handed to every ``filters[j]``: every 2-D slice is filtered with
        ``wet_mask * notnull(slice)`` at every scale.  ``"auto"`` on float64 ``IRREGULAR_WITH_LAND`` / ``MOM5U`` / ``MOM5T`` has a one-batch
        route of its own (``gcmf_apply_bank_gaps``: the slices' face coefficients folded once per slice, not once per scale and slice;
        needs ``nx % 4 == 0``); ``True`` / ``"auto"`` on the three land-mask kinds run the filters one after the other.

    Attributes
    ----------
    n_steps : int
    filters : list of Filter
        ``Filter(filter_scale=s, n_steps=bank.n_steps, <the same other arguments>)`` for every scale
    filter_specs : list of FilterSpec
        Their FilterSpecs: the same ``n_steps``, ``s_max`` and ``dx_min_sq``, different ``p``
    last_route : {"bank", "loop", None}
        Which route the last application took.  ``"bank"``: float64 data on the four grid types above with 2-D grid variables,
        ``evaluation != "reference"``, more than one scale and a backward cut for the polynomial (``Plan.bank_cut``); ``"loop"``:
        everything else -- and ``TRIPOLAR_POP_WITH_LAND`` outside the measured range of cells x scales (2 scales of 384 x 320 up to 32 of
        2400 x 3600, ``_bank_by_default``) and whatever ``nan_mask`` sends there.  ``GCMF_FILTER_BANK=0`` forces the loop, ``=1`` the bank wherever it is on offer.  At most
        ``GCMF_BANK_ENTRIES`` (64) entries -- scales x 2-D slices -- go into one library call, which bounds the device memory of a
        sweep: longer ones are cut over the scales, and over the leading axes of the field where those alone exceed the bound.
    """

    def __init__(self, filter_scales, dx_min, filter_shape=FilterShape.GAUSSIAN, transition_width=np.pi, ndim=2, n_steps=0,
                 grid_type=GridType.REGULAR, grid_vars=None, *, evaluation="auto", plan_cache=None, nan_mask=False):
        self.dx_min, self.filter_shape, self.transition_width, self.ndim = dx_min, filter_shape, transition_width, ndim
        self.grid_type, self.grid_vars = grid_type, dict(grid_vars or {})
        self.evaluation, self.plan_cache, self.nan_mask = evaluation, plan_cache, nan_mask
        self.Laplacian = ALL_KERNELS[grid_type]
        try:
            scales = [float(s) for s in filter_scales]
        except TypeError:
            raise ValueError(f"filter_scales must be a sequence of positive finite numbers, not {filter_scales!r}") from None
        if not scales:
            raise ValueError("filter_scales is empty: a FilterBank needs at least one filter scale")
        for s in scales:
            if not (np.isfinite(s) and s > 0):
                raise ValueError(f"filter_scales must be positive finite numbers, not {s!r}")
        self.filter_scales = scales
        # Filter's own checks, once (the per-scale objects below repeat them silently: they pass)
        _forward_only(evaluation)
        if plan_cache is not None and plan_cache not in PLAN_CACHE_MODES:
            raise ValueError(f"plan_cache must be one of {PLAN_CACHE_MODES} or None, not {plan_cache!r}")
        _check_nan_mask(nan_mask, grid_type)
        Filter._reject_bad_arguments(types.SimpleNamespace(Laplacian=self.Laplacian, dx_min=dx_min, transition_width=transition_width,
                                                           ndim=ndim, n_steps=n_steps))
        asked = int(n_steps)
        if ndim > 2:
            self.n_steps = asked
        else:
            default = max(int(_compute_n_steps_default(ndim, filter_shape, s, dx_min, transition_width)) for s in scales)
            if asked >= 3 and asked < default:
                warnings.warn("You have set n_steps below the default. Results might not be accurate.", stacklevel=2)
            self.n_steps = asked if asked >= 3 else default
        with warnings.catch_warnings():   # (a scale whose own default lies above the bank's degree: said once, above, or meant)
            warnings.filterwarnings("ignore", message="You have set n_steps below the default")
            self.filters = [Filter(filter_scale=s, dx_min=dx_min, filter_shape=filter_shape, transition_width=transition_width, ndim=ndim,
                                   n_steps=self.n_steps, grid_type=grid_type, grid_vars=self.grid_vars, evaluation=evaluation,
                                   plan_cache=plan_cache, nan_mask=nan_mask) for s in scales]
        self.filter_specs = [f.filter_spec for f in self.filters]
        self.last_route = None
        self._memo = _LaplacianMemo(self.Laplacian)

    def __repr__(self):
        return (f"FilterBank(filter_scales={self.filter_scales!r}, dx_min={self.dx_min!r}, filter_shape={self.filter_shape!r}, "
                f"transition_width={self.transition_width!r}, ndim={self.ndim!r}, n_steps={self.n_steps!r}, grid_type={self.grid_type!r})")

    # -- the two routes ----------------------------------------------------------------------------
    def _wants_bank(self):
        """None: the measured default decides; False / True: GCMF_FILTER_BANK=0 / 1."""
        env = os.environ.get("GCMF_FILTER_BANK", "")
        return {"0": False, "1": True}.get(env)

    def _stack(self, parts):
        if _is_torch(parts[0]):
            import torch
            return torch.stack(list(parts))
        return np.stack([np.asarray(x) for x in parts])

    def _bank_func(self, field, *args):
        """(len(filter_scales),) + field.shape: every scale's filter of `field`."""
        if _wants_grad(field):   # the same call with a grad_fn; backward: sum_j filters[j].adjoint(g[j], like=field)
            return _bank_function().apply(self, args, field)
        want = self._wants_bank()
        eligible = (len(self.filters) > 1 and self.evaluation != "reference" and want is not False
                    and not issubclass(self.Laplacian, BaseVectorLaplacian))
        # nan_mask: the batch exists for "auto" on the flux-form kinds (gcmf_apply_bank_gaps: the faces folded once per slice); the
        # land-mask kinds, True or "auto", run the filters -- which carry nan_mask -- one after the other
        faces = self.nan_mask == "auto" and self.grid_type in GAP_FOLD_GRID_TYPES
        if self.nan_mask and not faces:
            eligible = False
        if eligible and faces and want is None:
            eligible = _GAPS_BANK_BY_DEFAULT
        if eligible and want is None:
            shape = tuple(getattr(field, "shape", ()))
            eligible = len(shape) >= 2 and _bank_by_default(len(self.filters), int(shape[-2]), int(shape[-1]), self.grid_type)
        if eligible:
            with plan_cache_mode(self.plan_cache):
                out = self._memo.get(args)._run_bank(field, self.filter_specs, faces_from_nan=faces)
            if out is not None:
                self.last_route = "bank"
                self.last_path = kernels_last_path()
                return out
        outs = [f._operator(_create_filter_func)(field, *args) for f in self.filters]
        self.last_route = "loop"
        self.last_path = self.filters[-1].last_path
        return self._stack(outs)

    last_path = None

    def apply(self, field, dims=None):
        """Every scale's filter of a scalar field: a bare ``numpy.ndarray`` / ``torch.Tensor`` (filtered over its last two axes)
        gives the same kind of array of shape ``(len(filter_scales),) + field.shape``; an ``xarray.DataArray`` gives one with a
        new dimension ``filter_scale`` directly before ``dims`` (and, with real xarray, the scales as its coordinate)."""
        if issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a vector Laplacian. "
                             f"The ``.apply`` method is only suitable for scalar Laplacians.")
        f0 = self.filters[0]
        if _is_bare_array(field):
            return self._bank_func(field, *f0._grid_args(as_xarray=False))
        xr = _xarray()
        if xr is None:
            raise ImportError("xarray is required to filter xarray objects; pass numpy arrays or torch tensors instead")
        if isinstance(field, xr.Dataset):
            raise TypeError("FilterBank.apply filters one DataArray at a time: pass the Dataset's variables one by one")
        assert len(dims) == 2

        def scales_before_core(f, *args):   # apply_ufunc wants the new core dim behind the broadcast dims
            out = self._bank_func(f, *args)
            return out.movedim(0, -3) if _is_torch(out) else np.moveaxis(out, 0, -3)

        operands = [field] + f0._grid_args(as_xarray=True)
        res = xr.apply_ufunc(
            scales_before_core,
            *operands,
            input_core_dims=len(operands) * [list(dims)],
            output_core_dims=[["filter_scale"] + list(dims)],
            output_dtypes=[field.dtype],
            dask="parallelized",
        )
        if hasattr(res, "assign_coords"):
            res = res.assign_coords(filter_scale=list(self.filter_scales))
        return res

    def apply_to_vector(self, ufield, vfield, dims=None):
        """Every scale's filter of a vector field (u, v): two results shaped as ``apply``'s.  Vector Laplacians have no one-batch route:
        the scales run one after the other."""
        if not issubclass(self.Laplacian, BaseVectorLaplacian):
            raise ValueError(f"Provided Laplacian {self.Laplacian} is a scalar Laplacian. "
                             f"The ``.apply_to_vector`` method is only suitable for vector Laplacians.")
        f0 = self.filters[0]

        def both(u, v, *args):
            parts = [f._operator(_create_filter_func_vec)(u, v, *args) for f in self.filters]
            self.last_route = "loop"
            self.last_path = self.filters[-1].last_path
            return self._stack([x[0] for x in parts]), self._stack([x[1] for x in parts])

        if _is_bare_array(ufield) and _is_bare_array(vfield):
            return both(ufield, vfield, *f0._grid_args(as_xarray=False))
        xr = _xarray()
        if xr is None:
            raise ImportError("xarray is required to filter xarray objects; pass numpy arrays or torch tensors instead")
        assert len(dims) == 2

        def scales_before_core(u, v, *args):
            return tuple(x.movedim(0, -3) if _is_torch(x) else np.moveaxis(x, 0, -3) for x in both(u, v, *args))

        operands = [ufield, vfield] + f0._grid_args(as_xarray=True)
        res = xr.apply_ufunc(
            scales_before_core,
            *operands,
            input_core_dims=len(operands) * [list(dims)],
            output_core_dims=2 * [["filter_scale"] + list(dims)],
            output_dtypes=[ufield.dtype, vfield.dtype],
            dask="parallelized",
        )
        return tuple(r.assign_coords(filter_scale=list(self.filter_scales)) if hasattr(r, "assign_coords") else r for r in res)
