"""The bits of the Python call path, route by route: a fixed list of calls through the public API on fixed seeds, one line per case --
the case, `last_path` (FilterBank: `last_route` too) and, per output, its kind, dtype, shape and the sha256 of its bytes.  Two commits
that print the same lines hand the library the same calls: run it on both and `diff` the outputs (profiles/call_options/).
    python tools/call_path_digest.py > digest.txt"""
import hashlib
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gcm_filters_amd import Filter, FilterBank, GridType, testing as T  # noqa: E402
from gcm_filters_amd import kernels as K  # noqa: E402

SHAPE, ODD, BIG, N_STEPS = (40, 64), (40, 62), (2048, 2048), 12     # ODD: nx % 4 != 0, the gap fold's fallback; BIG: the row blocks' size


def report(name, outs, who):
    """`who`: the Filter / FilterBank that made `outs` (its last_path is read after the call), or kernels.last_path itself."""
    path = who() if callable(who) else who.last_path
    if isinstance(who, FilterBank):
        path = f"{who.last_route}/{path}"
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    words = []
    for o in outs:
        a = o.detach().cpu().numpy() if torch.is_tensor(o) else np.asarray(o)
        where = f"torch@{o.device.type}" if torch.is_tensor(o) else type(o).__name__
        words.append(f"{where}:{a.dtype}{list(a.shape)}:{hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}")
    print(f"{name:44s} {str(path):22s} {' '.join(words)}", flush=True)


def make(kind, gv, cls=Filter, **kw):
    dx = T.grid_dx_min(kind, gv)
    scale = {"filter_scales": [3 * dx, 4 * dx, 6 * dx]} if cls is FilterBank else {"filter_scale": 4 * dx}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (n_steps below the default)
        return cls(dx_min=dx, n_steps=N_STEPS, grid_type=GridType[kind], grid_vars=gv, **scale, **kw)


def gappy(shape, seed, slices=None):
    """A random field with 4 % NaNs in every 2-D slice (or in `slices` only)."""
    f = T.random_field(shape, seed)
    holes = T.random_field(shape, seed + 1000) < 0.04
    if slices is not None:
        holes[[i for i in range(shape[0]) if i not in slices]] = False
    f[holes] = np.nan
    return f


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def main():
    irr = T.scalar_grid_vars("IRREGULAR_WITH_LAND", SHAPE)
    flt, f = make("IRREGULAR_WITH_LAND", irr), T.random_field(SHAPE, 100)
    for name, x in (("irregular f64 device", dev(f)), ("irregular f64 host", f), ("irregular f32 device", dev(f.astype(np.float32))),
                    ("irregular f32 host", f.astype(np.float32)), ("irregular view device", dev(T.random_field((40, 128), 101))[:, ::2]),
                    ("irregular view host", T.random_field((40, 128), 101)[:, ::2]), ("irregular batch device", dev(T.random_field((2, 3) + SHAPE, 102))),
                    ("irregular batch host", T.random_field((2, 3) + SHAPE, 102))):
        report(name, flt.apply(x), flt)
    g = T.random_field((3,) + SHAPE, 103)
    like = gappy((3,) + SHAPE, 104)
    for name, out in (("adjoint device", lambda: flt.adjoint(dev(g))), ("adjoint host", lambda: flt.adjoint(g)),
                      ("adjoint like device", lambda: flt.adjoint(dev(g), like=dev(like))), ("adjoint like host", lambda: flt.adjoint(g, like=like)),
                      ("adjoint numpy like, device field", lambda: flt.adjoint(dev(g), like=like))):
        report(name, out(), flt)
    lap = K.ALL_KERNELS[GridType.IRREGULAR_WITH_LAND](**irr)
    report("laplacian __call__ device", lap(dev(f)), K.last_path)
    report("laplacian __call__ host", lap(f), K.last_path)

    land32 = {"wet_mask": T.land_mask(SHAPE).astype(np.float32)}
    for ev in ("reference", "backward"):
        e = make("REGULAR_WITH_LAND", land32, evaluation=ev)
        for name, x in ((f"land f32 {ev} device", dev(f.astype(np.float32))), (f"land f32 {ev} host", f.astype(np.float32))):
            report(name, e.apply(x), e)
    masked = make("REGULAR_WITH_LAND", {"wet_mask": T.land_mask(SHAPE)}, nan_mask=True)
    x = gappy((3,) + SHAPE, 105, slices=(0, 2))
    report("nan_mask=True device", masked.apply(dev(x)), masked)
    report("nan_mask=True host", masked.apply(x), masked)
    report("nan_mask=True adjoint like device", masked.adjoint(dev(g), like=dev(x)), masked)
    for shape in (SHAPE, ODD):
        auto = make("MOM5U", T.scalar_grid_vars("MOM5U", shape), nan_mask="auto")
        x, gg = gappy((3,) + shape, 106), T.random_field((3,) + shape, 107)
        report(f"nan_mask=auto MOM5U {shape[1]} device", auto.apply(dev(x)), auto)
        report(f"nan_mask=auto MOM5U {shape[1]} host", auto.apply(x), auto)
        report(f"nan_mask=auto MOM5U {shape[1]} adjoint device", auto.adjoint(dev(gg), like=dev(x)), auto)

    wet3 = np.stack([T.land_mask(SHAPE) * (T.random_field(SHAPE, 110 + k) > 0.05 * k) for k in range(3)])
    for stack in ("0", "1"):
        os.environ["GCMF_STACK_LEVELS"] = stack     # (read when the Laplacian of the level stack is built: at the first call)
        lev = make("IRREGULAR_WITH_LAND", dict(irr, wet_mask=wet3))
        report(f"levels STACK={stack} device", lev.apply(dev(g)), lev)
        report(f"levels STACK={stack} host", lev.apply(g), lev)
        report(f"levels STACK={stack} batch (2, 3) device", lev.apply(dev(T.random_field((2, 3) + SHAPE, 111))), lev)
        report(f"levels STACK={stack} adjoint like device", lev.adjoint(dev(g), like=dev(like)), lev)
        report(f"levels STACK={stack} adjoint numpy like", lev.adjoint(dev(g), like=like), lev)
    del os.environ["GCMF_STACK_LEVELS"]

    (u, v), cg = T.vector_case("VECTOR_C_GRID", SHAPE)
    vec = make("VECTOR_C_GRID", cg)
    report("C-grid apply_to_vector device", vec.apply_to_vector(dev(u), dev(v)), vec)
    report("C-grid apply_to_vector host", vec.apply_to_vector(u, v), vec)
    report("C-grid adjoint_to_vector device", vec.adjoint_to_vector(dev(u), dev(v)), vec)

    for kw in ({}, {"nan_mask": "auto"}):
        bank = make("IRREGULAR_WITH_LAND", irr, cls=FilterBank, **kw)
        x = gappy((2,) + SHAPE, 120) if kw else T.random_field((2,) + SHAPE, 120)
        for name, xx in (("device", dev(x)), ("host", x)):
            report(f"bank {kw.get('nan_mask', 'plain')} {name}", bank.apply(xx), bank)

    big = make("REGULAR_WITH_LAND", {"wet_mask": T.land_mask(BIG)})
    x = T.random_field(BIG, 130)
    for call in (1, 2, 3):      # the third single host field on a plan takes the row blocks
        report(f"large host field, call {call}", big.apply(x), big)


if __name__ == "__main__":
    main()
