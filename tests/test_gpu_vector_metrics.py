"""Every vector kernel family on metric planes that differ from one another and vary along both axes, against the oracle.

``testing.vector_grid_vars`` -- the metrics of every other vector test -- has no plane that varies along x, constant dy* planes, dxT == dxCu,
dxBu == dxCv, HUS == HTE, HUW == HTN == DXU, areas that are products of the spacings, and B-grid coupling weights dmc, dme, dmw of exactly 0:
a kernel that reads a coefficient one column off, takes one plane for another or has the wrong sign on dme passes on it.  The cases here copy
the selectors (dtype, batch, evaluation, tuning, options, env, kernel regex) of the vector cases of tests/test_gpu_dispatch_edges.py and
tests/test_gpu_coastlines.py, so they reach the same kernels, on ``testing.vector_grid_vars_irregular`` (``Case.metrics = "irregular"``);
tests/test_vector_metrics_fixture.py shows on the CPU that every such fault changes the oracle's answer by more than 1e-3 there.

Assertions are those of ``test_dispatch_edge`` -- NaN pattern, kernel regex, filter and bare Laplacian against the oracle, f64 <= 1e-12 -- plus,
for the B-grid in f64, bit-equality of the bare Laplacian with the oracle (the filter's under ``evaluation="reference"`` is test_dispatch_edge's
own).  f32 gates: each case's own scheme formula of ``errors()``, as the spherical cases of the same selectors have it; no case needed the
looser forward formula (DESIGN.md lists the figures measured on an MI355X).

A second table holds the HIP result to 1e-11 of the imported reference's own output (tests/golden/reference_vector_metrics.npz).

``CASES`` imports without a GPU (tests/test_vector_metrics_fixture.py checks the families it names and the stability of its filters).
"""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import test_gpu_dispatch_edges as DE
from test_gpu_dispatch_edges import BIT_EXACT, Case, _t, errors, run_case

CGRID, BGRID = "VECTOR_C_GRID", "VECTOR_B_GRID"
PRIV = _t(clenshaw=2, multi_s=8)
CASES = []


def add(id, grid, dt, shape, kernel, **kw):
    assert "irr-" + id not in {c.id for c in CASES}, id
    CASES.append(Case("irr-" + id, grid, dt, shape, kernel, metrics="irregular", **kw))


# (tag, grid, dtype, S, selectors) of the rows family of test_gpu_dispatch_edges._rows_family: batched, and single-level (PRIV = true)
ROWS_FORMS = (
    ("stream2", CGRID, "f8", 4, dict(kernel=r"k_cgrid_stream2<double, double, 2, 4, ", nb=3, ev="reference")),
    ("stream2c", CGRID, "f8", 4, dict(kernel=r"k_cgrid_stream2c<double, 2, 4, ", nb=3)),
    ("priv", CGRID, "f8", 4, dict(kernel=r"k_cgrid_stream2c<double, 2, 4, \d, true>", tuning=PRIV)),
    ("priv", CGRID, "f4", 4, dict(kernel=r"k_cgrid_stream2c<float, 2, 4, \d, true>", tuning=PRIV, scheme="cgrid_backward")),
    ("ring", CGRID, "f4", 6, dict(kernel=r"k_cgrid_ring<float, 6, ", nb=4, options=_t(cgrid_ring_smax=6), scheme="cgrid_backward")),
    ("ringf", CGRID, "f4", 5, dict(kernel=r"k_cgrid_ringf<float, 5, ", nb=4, ev="reference")),
    ("stream2", BGRID, "f8", 4, dict(kernel=r"k_bgrid_stream2<double, double, 2, 4, ", nb=3, ev="reference")),
    ("stream2c", BGRID, "f8", 4, dict(kernel=r"k_bgrid_stream2c<double, 2, 4, ", nb=3, tuning=PRIV)),
    ("stream2c", BGRID, "f4", 4, dict(kernel=r"k_bgrid_stream2c<float, 2, 4, ", nb=3, ev="backward", scheme="bgrid_backward")),
    ("priv", BGRID, "f8", 4, dict(kernel=r"k_bgrid_stream2c<double, 2, 4, \d, true>", tuning=PRIV)),
)


def _rows():
    """Rows S + 2 (the ghost rows of the one strip wrap across the periodic y seam) and 2 S + 2, nx = 64."""
    for tag, grid, dt, S, sel in ROWS_FORMS:
        for rows in (S + 2, 2 * S + 2):
            add(f"rows-{tag}-{grid}-{dt}-{rows}", grid, dt, (rows, 64), **sel)


def _other_shapes():
    for dt in ("f8", "f4"):
        ty = "double" if dt == "f8" else "float"
        vec = 2 if dt == "f8" else 4
        # nx odd: the general kernels; nx = 128: the tile and the single-launch selectors
        add(f"odd-cgrid-{dt}", CGRID, dt, (60, 127), rf"k_cgrid_step<{ty}, ")
        add(f"odd-bgrid-{dt}", BGRID, dt, (60, 127), rf"k_bgrid_step<{ty}, ")
        add(f"tile-cgrid-{dt}", CGRID, dt, (60, 128), rf"k_cgrid_step<{ty}, ", nb=2, env=_t(GCMF_CGRID_TILE="1"))
        add(f"tile-bgrid-{dt}", BGRID, dt, (60, 128), rf"k_bgrid_step<{ty}, ", nb=2, tuning=_t(multi_s=1), env=_t(GCMF_CGRID_TILE="1"))
        add(f"single-cgrid-{dt}", CGRID, dt, (60, 128), rf"k_cgrid_stream<{ty}, ", tuning=_t(multi_s=1))
        add(f"single-bgrid-{dt}", BGRID, dt, (60, 128), rf"k_bgrid_stream<{ty}, ", tuning=_t(multi_s=1))
        # tall and narrow: the ghost columns wrap around x more than once
        for nx in (vec, 2 * vec):
            add(f"narrow-cgrid-{dt}-{nx}", CGRID, dt, (120, nx), r"k_cgrid_stream2c<double" if dt == "f8" else r"k_cgrid_ring<float", nb=3,
                scheme="forward" if dt == "f8" else "cgrid_backward")
            add(f"narrow-bgrid-{dt}-{nx}", BGRID, dt, (120, nx), r"k_bgrid_stream2c<double, " if dt == "f8" else r"k_bgrid_stream2<float, ", nb=3)
    # five strips of ten rows, the last of three
    add("strip-cgrid-last3", CGRID, "f8", (43, 128), r"k_cgrid_stream2c<double, 2, 4, ", nb=2, tuning=_t(multi_s=8, strip_rows=10))
    # n_steps = 10 in launches of five levels: the second starts from the first's state planes
    add("ringf-two-launches", CGRID, "f4", (20, 64), r"k_cgrid_ringf<float, 5, ", nb=4, n_steps=10, ev="reference")


def _coastlines():
    """C-grid: land, a wet_mask_q of its own, smooth kappas with noise -- on irregular metrics."""
    for coast in ("speckle:indq", "channels"):
        for shape in ((24, 64), (60, 128)):
            tag = f"{coast.replace(':', '-')}-{shape[0]}x{shape[1]}"
            add(f"coast-stream2c-{tag}", CGRID, "f8", shape, r"k_cgrid_stream2c<double, 2, 4, ", nb=3, coast=coast, land_values="finite")
            add(f"coast-ring-{tag}", CGRID, "f4", shape, r"k_cgrid_ring<float, 6, ", nb=4, options=_t(cgrid_ring_smax=6),
                scheme="cgrid_backward", coast=coast, land_values="finite")


_rows()
_other_shapes()
_coastlines()


def families(cases):
    """The k_cgrid_* / k_bgrid_* kernel families the vector cases of a table name in their regexes."""
    out = set()
    for c in cases:
        if c.grid in (CGRID, BGRID):
            out |= {m for m in re.findall(r"k_[cb]grid_[a-z0-9]+", c.kernel)}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_vector_kernel_on_irregular_metrics(c, monkeypatch):
    r = run_case(c, monkeypatch)
    kernel, geom = r["kernel"], r["geom"]
    for g, w in zip(r["got"], r["truth"]):
        assert g.shape == w.shape
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, kernel, "NaN pattern differs")
    for g, w in zip(r["lap"], r["ltruth"]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, "Laplacian NaN pattern differs")
    e, bound, el, lbound = errors(c, r)
    if c.dt == "f4":
        e_ref = max(DE._rel(g, w) for g, w in zip(r["ref32"], r["truth"]))
        print(f"\n{c.id}: {kernel.split('(')[0]} e {e:.3e} e_ref {e_ref:.3e} bound {bound:.3e} ({c.scheme}); Laplacian {el:.3e} (bound {lbound:.3e})")
    else:
        print(f"\n{c.id}: {kernel.split('(')[0]} e {e:.3e} Laplacian {el:.3e}")
    assert e <= bound, (c.id, kernel, e, bound)
    assert el <= lbound, (c.id, "Laplacian", el, lbound)
    if c.dt == "f8" and c.grid == BGRID:
        assert BGRID in BIT_EXACT
        for g, w in zip(r["lap"], r["ltruth"]):
            assert np.array_equal(g, w, equal_nan=True), (c.id, "Laplacian not bit-equal to the oracle", float(np.abs(g - w).max()))
    if c.dt == "f8" and c.ev == "reference" and c.grid in BIT_EXACT:
        for g, w in zip(r["got"], r["truth"]):
            assert np.array_equal(g, w, equal_nan=True), (c.id, kernel, "not bit-equal to the oracle", float(np.abs(g - w).max()))
    assert re.search(c.kernel, kernel), (c.id, kernel, geom)
    for k, v in c.geom:
        assert geom.get(k) == v, (c.id, kernel, k, geom)


# ------------------------------------------------------------------------------------------------------------------------------
# against the imported reference's own output on the irregular fixture (make_golden.py --vector-metrics)
# ------------------------------------------------------------------------------------------------------------------------------
def _golden_names():
    import make_golden as MG
    return MG.vector_metrics_case_names()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _golden_names())
def test_vs_imported_reference_on_irregular_metrics(name):
    """The HIP result within 1e-11 of what the reference itself computed (the gate of test_gpu_parity.test_vs_imported_reference)."""
    import make_golden as MG
    from test_gpu_parity import gpu_filter, gpu_laplacian, rel_err

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", MG.VECTOR_METRICS_FILE)) as z:
        want = z[name]
    grid, fields, gv, fk = MG.build_vector_metrics_case(name)
    got = gpu_laplacian(grid, fields, gv) if fk is None else gpu_filter(grid, fields, gv, fk)
    assert got.shape == want.shape and got.dtype == want.dtype and np.isfinite(got).all()
    err = rel_err(got, want)
    print(f"\n{name}: rel_err {err:.3e}")
    assert err <= 1e-11, (name, err)
    if grid in BIT_EXACT and fk is None:
        assert np.array_equal(got, want), (name, "the bare Laplacian is not bit-equal to the reference's")
