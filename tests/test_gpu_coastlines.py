"""The land-aware kernels on coastlines the fixture mask never draws, against the oracle (oracle/gcmf_oracle.py).

Every other wet mask in the suite is ``testing.land_mask`` (row 0 and the south-west quadrant are land) or rectangles on top of it: the
periodic y seam is closed, the coast is aligned to 2 and 4 cells in x, no wet cell is cut off from the sea, the tripole seam is open water
and the C-grid's two masks are one array.  This module crosses every way the dispatch-edge table (tests/test_gpu_dispatch_edges.py)
reaches a land-aware kernel with ``testing.COASTLINES``: open southern rows, speckle, a checkerboard, one-cell channels, lakes, one land
cell, all land, coasts exactly on the window and strip cuts, land on the tripole fold; on IRREGULAR_WITH_LAND also with exact zeros in
kappa, on the C-grid with ``wet_mask_q != wet_mask_t`` and a non-zero ``kappa_aniso``.  tests/test_oracle_golden.py pins the oracle to the
imported reference on these very masks (tests/golden/reference_coastlines*.npz).

A case is a ``Case`` of the dispatch-edge module and asserts what ``test_dispatch_edge`` asserts, with its bounds: the kernel reached,
the NaN pattern of filter and Laplacian identical to the oracle's, f64 within 1e-12 of the oracle's largest value, bit-equality for the
BIT_EXACT kinds under ``evaluation="reference"``, f32 by ``errors()``'s policy.  The values on land rotate over NaN everywhere, finite
everywhere, and NaN on half the land plus three NaN in wet cells (``all_land`` with NaN on all land has no finite cell: it takes finite
values instead).

``FAMILIES``, ``CASES`` and ``REFUSED`` import without a GPU: tests/test_coastline_table.py checks that every family is crossed with every
coastline of its grid kinds, that every grid kind meets every coastline in some family, and that `fold` meets both tripolar kinds in both
forms of the seam band.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from test_gpu_dispatch_edges import BIT_EXACT, Case, _inputs, _t, errors, run_case

WIDE, RAGGED = (97, 236), (97, 118)      # nx % 4 == 0 and not (land_ok both ways); two windows of 112 plus a remainder / one plus a remainder
H = 20                                   # strip_rows: five strips on 97 rows
MASK_KINDS = ("REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED")
FLUX_KINDS = ("IRREGULAR_WITH_LAND", "MOM5U", "MOM5T")
TRIPOLAR = ("TRIPOLAR_POP_WITH_LAND", "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED")
CGRID = ("VECTOR_C_GRID",)


@dataclass(frozen=True)
class Family:
    """One way to reach one kernel: the recipe of a dispatch-edge case, on the grid kinds it applies to (they rotate over the coastlines)."""
    id: str
    grids: Tuple[str, ...]
    dt: str
    shape: Tuple[int, int]
    kernel: str                  # regex; "{K}" stands for the KIND template argument, which the grid decides
    kw: Tuple = ()               # the remaining Case fields
    kappa: bool = False          # an IRREGULAR_WITH_LAND family: also with testing.kappa_with_zeros on speckle and one_land_cell
    every_grid: bool = False     # every coastline on EVERY grid kind of the family (the tripole seam's band), not on one of them in turn
    kernel_by_grid: Tuple = ()   # (grid, regex): kinds whose dispatch reaches another kernel of the family by the same recipe
    ragged: Tuple = ()           # coastlines (with variant) this family runs at RAGGED instead of its shape: the pairs REFUSED names

    @property
    def tripolar(self):
        return self.grids[0].startswith("TRIPOLAR")


def _f(id, grids, dt, shape, kernel, kappa=False, every_grid=False, kernel_by_grid=(), ragged=(), **kw):
    return Family(id, tuple(grids), dt, shape, kernel, tuple(sorted(kw.items())), kappa, every_grid, tuple(kernel_by_grid), tuple(ragged))


FWD = dict(ev="reference")
# (not `one_land_cell`: on MOM5U one land t-cell closes no u-cell's four faces, n_land == 0, and such a plan keeps the backward evaluation
# at any nx -- the pair would not be refused)
RAGGED_COASTS = ("speckle", "channels", "lakes", "on_the_cuts", "one_land_cell:kappa")
FAMILIES = [
    # ---- forward ----------------------------------------------------------------------------------------------------------------
    _f("step-f8", FLUX_KINDS[:1] + MASK_KINDS[:1], "f8", RAGGED, r"k_scalar_step<double, double, ", kappa=True, tuning=_t(multi_s=1, clenshaw=0), **FWD),
    _f("step-f4", ("MOM5U", "REGULAR_WITH_LAND_AREA_WEIGHTED"), "f4", RAGGED, r"k_scalar_step<float, ", **FWD),
    _f("multi-mask-f8", MASK_KINDS, "f8", RAGGED, r"k_scalar_multi<double, double, \d, 4, ", tuning=_t(multi_s=4, clenshaw=0, strip_rows=H), **FWD),
    _f("multi-flux-f8", FLUX_KINDS, "f8", RAGGED, r"k_scalar_multi<double, double, {K}, 4, ", kappa=True,
       tuning=_t(multi_s=4, clenshaw=0, strip_rows=H), **FWD),
    _f("multi-mask-f4", MASK_KINDS, "f4", WIDE, r"k_scalar_multi<float, double, \d, 4, ", tuning=_t(multi_s=4, clenshaw=0, strip_rows=H), **FWD),
    _f("multi-flux-f4", FLUX_KINDS, "f4", WIDE, r"k_scalar_multi<float, double, {K}, 4, ", kappa=True,
       tuning=_t(multi_s=4, clenshaw=0, strip_rows=H), **FWD),
    _f("flux-multi2-f8", FLUX_KINDS, "f8", WIDE, r"k_flux_multi2<double, double, 8>", kappa=True, tuning=_t(multi_s=8, clenshaw=0, strip_rows=H),
       env=_t(GCMF_RING="0"), **FWD),
    _f("flux-multi2-f4", FLUX_KINDS, "f4", WIDE, r"k_flux_multi2<float, double, 8>", kappa=True, options=_t(ring_flux_f32=0), **FWD),
    # the static-ring kernel: as a later launch (24 steps: three launches of 8) and as the first one (11 steps: 8 + 3, ring_first)
    _f("ring-maskz-f8", MASK_KINDS, "f8", WIDE, r"k_ring<double, double, {K}, 8, ", tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-flux-f8", FLUX_KINDS, "f8", WIDE, r"k_ring<double, double, {K}, 8, ", kappa=True, tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-first-maskz-f8", MASK_KINDS, "f8", WIDE, r"k_ring<double, double, {K}, 8, ", n_steps=11,
       tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-first-flux-f8", FLUX_KINDS, "f8", WIDE, r"k_ring<double, double, {K}, 8, ", kappa=True, n_steps=11,
       tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-first-maskz-f4", MASK_KINDS, "f4", WIDE, r"k_ring<float, double, {K}, 8, ", n_steps=11,
       tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-first-flux-f4", FLUX_KINDS, "f4", WIDE, r"k_ring<float, double, {K}, 8, ", kappa=True, n_steps=11,
       tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), options=_t(ring_flux_f32=1), **FWD),
    _f("ring-maskz-f4", MASK_KINDS, "f4", WIDE, r"k_ring<float, double, {K}, 8, ", tuning=_t(multi_s=8, clenshaw=0, strip_rows=H), **FWD),
    _f("ring-flux-f4", FLUX_KINDS, "f4", WIDE, r"k_ring<float, double, {K}, 8, ", kappa=True, tuning=_t(multi_s=8, clenshaw=0, strip_rows=H),
       options=_t(ring_flux_f32=1), **FWD),
    # ---- backward ---------------------------------------------------------------------------------------------------------------
    # evaluation="auto" as a user gets it, on every non-tripolar land kind: backward where land can be fixed up (land_ok: nx % 4 == 0), and
    # at RAGGED, where it cannot, the forward kernels -- the pairs in REFUSED, which assert the kernel they do reach
    _f("backward-auto", FLUX_KINDS + MASK_KINDS, "f8", WIDE, r"k_ringc[sz]?<double, (\d, )?8, ", kappa=True, tuning=_t(multi_s=8),
       options=_t(ringc_smax=8), ragged=RAGGED_COASTS),
    _f("ringc-maskz", MASK_KINDS, "f8", WIDE, r"k_ringc<double, {K}, 8, ", every_grid=True, tuning=_t(multi_s=8, strip_rows=H), options=_t(ringc_smax=8)),
    _f("ringc-flux", FLUX_KINDS, "f8", WIDE, r"k_ringc<double, {K}, 8, ", kappa=True, tuning=_t(multi_s=8, strip_rows=H),
       options=_t(ringc_smax=8, ringc_zip=0), env=_t(GCMF_RINGC_XE_ROWS="0")),
    _f("ringc-flux-nozigzag", FLUX_KINDS, "f8", WIDE, r"k_ringc<double, {K}, 8, ", kappa=True, tuning=_t(multi_s=8, strip_rows=H),
       options=_t(ringc_smax=8, ringc_zip=0), env=_t(GCMF_RINGC_XE_ROWS="0", GCMF_ZIGZAG="0")),
    # the early-exit form where it shortens the march (launch_ringc): strips of 22 rows march 40 rows instead of 48
    _f("ringcs", FLUX_KINDS, "f8", WIDE, r"k_ringcs<double, 8, ", kappa=True, tuning=_t(multi_s=8, strip_rows=22), options=_t(ringc_smax=8, ringc_zip=0)),
    # zipped strips choose their own height (ringc_cut offers no zipped strips to a plan with strip_rows set)
    _f("ringcz", FLUX_KINDS, "f8", WIDE, r"k_ringcz<double, 8, ", kappa=True, options=_t(ringc_smax=8, ringc_zip=1)),
    _f("ringc9", FLUX_KINDS, "f8", WIDE, r"k_ringc<double, {K}, 9, ", kappa=True, n_steps=36, tuning=_t(multi_s=8, strip_rows=H), options=_t(ringc_zip=0),
       env=_t(GCMF_RINGC_XE_ROWS="0")),
    # a packed batch whose runs of q = 27 rows cross field boundaries (the geometry of the dispatch-edge case packed-nb7, about the smallest
    # batch the launcher's cost model packs); 16 steps, a first and a later launch of eight levels: the oracle on 3 M cells is this module's cost
    _f("ringcp", MASK_KINDS[:1] + FLUX_KINDS[:1], "f8", (50, 8512), r"k_ringcp<double, {K}, 8, ", kappa=True, nb=7, n_steps=16,
       options=_t(pack_batch=1), geom=_t(H=27)),
    _f("ringc-one", FLUX_KINDS, "f8", (64, 128), r"k_ringc_one<", kappa=True, options=_t(single_launch=1)),
    _f("resident", FLUX_KINDS[:1] + MASK_KINDS[:1], "f8", WIDE, r"k_resident<", kappa=True, env=_t(GCMF_RESIDENT="1")),
    _f("ringc-flux-f4", FLUX_KINDS, "f4", WIDE, r"k_ringcs<float, 7, ", kappa=True, ev="backward", options=_t(ringc_smax=8),
       scheme="scalar_backward"),
    # ---- tripolar: the seam inside the launch (zip_fold, the flux kind only) and in k_fold_band, backward and forward --------------------
    _f("tripolar-zip", TRIPOLAR[:1], "f8", WIDE, r"k_ringcz<double, 8, ", options=_t(ringc_smax=8, zip_fold=1)),
    # (the band families: every coastline on BOTH tripolar kinds -- k_fold_band has a flux form and a mask form)
    _f("tripolar-band-backward", TRIPOLAR, "f8", WIDE, r"k_ringcs<double, 8, ", every_grid=True,
       kernel_by_grid=((TRIPOLAR[1], r"k_ringc<double, 5, 8, "),), tuning=_t(multi_s=8, clenshaw=2),
       options=_t(ringc_smax=8, zip_fold=0, ringc_zip=0)),
    _f("tripolar-band-forward", TRIPOLAR, "f8", WIDE, r"k_ring<double, double, {K}, 8, ", every_grid=True, tuning=_t(multi_s=8, clenshaw=0), **FWD),
    # ---- C-grid: wet_mask_q derived from wet_mask_t, kappa_iso and kappa_aniso smooth and non-zero ---------------------------------
    _f("cgrid-step", CGRID, "f8", WIDE, r"k_cgrid_step<double, ", nb=2, env=_t(GCMF_CGRID_TILE="1")),
    _f("cgrid-stream", CGRID, "f8", WIDE, r"k_cgrid_stream<double, ", tuning=_t(multi_s=1)),
    _f("cgrid-stream2", CGRID, "f8", WIDE, r"k_cgrid_stream2<double, double, 2, 4, ", nb=3, **FWD),
    _f("cgrid-stream2c", CGRID, "f8", WIDE, r"k_cgrid_stream2c<double, 2, 4, ", nb=3),
    _f("cgrid-stream2c-priv", CGRID, "f8", WIDE, r"k_cgrid_stream2c<double, 2, 4, \d, true>", tuning=_t(clenshaw=2, multi_s=8)),
    _f("cgrid-ring", CGRID, "f4", WIDE, r"k_cgrid_ring<float, 6, ", nb=4, options=_t(cgrid_ring_smax=6), scheme="cgrid_backward"),
    _f("cgrid-ringf", CGRID, "f4", WIDE, r"k_cgrid_ringf<float, 5, ", nb=4, **FWD),
]

# (family, coastline) -> the predicate in csrc/ that sends the pair to another kernel, and the kernel it reaches instead (flux-form kinds,
# land-mask kinds).  A refused pair still runs and asserts that kernel.  land_ok (gcmf_api_blocks.hip) is false for a plan with land at
# nx % 4 != 0 (k_land_fix and k_zero_land work on words of four mask bytes), so clenshaw_cut offers no backward evaluation and
# sched_forward_scalar runs without zero_land: the flux kinds take k_ring from the second launch on, the land-mask kinds the general
# k_scalar_multi for every launch (ring_supported wants land_zero there).
REFUSED = {("backward-auto", coast): ("land_ok", (r"k_ring<double, double, 2, 8, ", r"k_scalar_multi<double, double, \d, 8, "))
           for coast in RAGGED_COASTS}


def _coasts(fam: Family, fi: int):
    """(coastline with its variant, the grid it runs on) for every cell of the family's row of the table.  The grid kinds of a family
    take turns over the coastlines, from a start that moves with the family's index: every kind meets every coastline in some family."""
    names = T.coastline_names(fam.tripolar)
    if fam.every_grid:
        out = [(n, g) for n in names for g in fam.grids]
    else:
        out = [(n, fam.grids[(fi + k) % len(fam.grids)]) for k, n in enumerate(names)]
    if fam.grids == CGRID:
        out += [("speckle:indq", "VECTOR_C_GRID"), ("channels:indq", "VECTOR_C_GRID")]
    if fam.kappa:
        out += [("speckle:kappa", "IRREGULAR_WITH_LAND"), ("one_land_cell:kappa", "IRREGULAR_WITH_LAND")]
    return out


def _cases():
    cases, table = [], {}
    for fi, fam in enumerate(FAMILIES):
        for ci, (coast, grid) in enumerate(_coasts(fam, fi)):
            how = T.LAND_TREATMENTS[(fi + ci) % 3]
            if coast.startswith("all_land") and how == "nan":
                how = "finite"           # (no finite cell otherwise: the case would compare NaN patterns alone)
            if fam.grids == CGRID:
                how = "finite"           # (the C-grid stencil does not mask its input: a NaN would spread over the whole result)
            kernel = dict(fam.kernel_by_grid).get(grid, fam.kernel).replace("{K}", r"\d")
            kw = dict(fam.kw)
            refused = REFUSED.get((fam.id, coast))
            if refused:
                kw["not_kernel"], kernel = kernel, refused[1][0 if grid in FLUX_KINDS else 1]
            shape = RAGGED if coast in fam.ragged else fam.shape
            cases.append(Case(f"{fam.id}-{grid}-{coast}", grid, fam.dt, shape, kernel, coast=coast, land_values=how, **kw))
            table.setdefault((fam.id, coast), []).append(cases[-1])
    return cases, table


CASES, TABLE = _cases()          # TABLE: (family id, coastline) -> its cases (one; one per grid kind in an every_grid family)


def _describe_worst(c: Case, r):
    """Grid, coastline, kernel, geometry, and the cell where the filter is furthest from the oracle with its neighbours' mask bytes."""
    _, gv = _inputs(c)
    mk = "wet_mask_t" if c.grid == "VECTOR_C_GRID" else "wet_mask"
    m = np.asarray(gv[mk])
    got, want = np.asarray(r["got"][0], np.float64), np.asarray(r["truth"][0], np.float64)
    d = np.where(np.isnan(got) != np.isnan(want), np.inf, np.nan_to_num(np.abs(got - want)))
    idx = np.unravel_index(np.argmax(d), d.shape)
    j, i = idx[-2:]
    ny, nx = c.shape
    rows = [(j + dj) % ny for dj in (1, 0, -1)]
    cols = [(i + di) % nx for di in (-2, -1, 0, 1, 2)]
    near = "\n".join(f"    row {jj:4d}: " + " ".join(str(int(m[jj, ii])) for ii in cols) for jj in rows)
    return (f"{c.id}: grid {c.grid} coast {c.coast} land values {c.land_values} dtype {c.dt} shape {c.shape}\n  kernel {r['kernel']}\n"
            f"  geometry {r['geom']}\n  worst cell {tuple(int(x) for x in idx)}: got {got[idx]!r} want {want[idx]!r}\n"
            f"  {mk} around it (columns {cols[0]}..{cols[-1]}, north on top):\n{near}")


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_coastline(c, monkeypatch, tmp_path):
    if dict(c.env).get("GCMF_RESIDENT") == "1":
        monkeypatch.setenv("GCMF_RESIDENT_LOCK_DIR", str(tmp_path))
    r = run_case(c, monkeypatch)
    kernel, geom = r["kernel"], r["geom"]
    e, bound, el, lbound = errors(c, r)
    print(f"\n{c.id}: {kernel} {geom} filter {e:.3e} (bound {bound:.3e}) Laplacian {el:.3e} (bound {lbound:.3e})")
    try:
        assert any(np.isfinite(w).any() for w in r["truth"]), (c.id, "the oracle's result has no finite cell")
        for g, w in zip(r["got"], r["truth"]):
            assert g.shape == w.shape
            assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, kernel, "NaN pattern differs")
        for g, w in zip(r["lap"], r["ltruth"]):
            assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, "Laplacian NaN pattern differs")
        assert e <= bound, (c.id, kernel, e, bound)
        assert el <= lbound, (c.id, "Laplacian", el, lbound)
        if c.dt == "f8" and c.ev == "reference" and c.grid in BIT_EXACT:
            for g, w in zip(r["got"], r["truth"]):
                assert np.array_equal(g, w, equal_nan=True), (c.id, kernel, "not bit-equal to the oracle")
    except AssertionError:
        print(_describe_worst(c, r))
        raise
    assert re.search(c.kernel, kernel), (c.id, kernel, geom)
    if c.not_kernel:
        assert not re.search(c.not_kernel, kernel), (c.id, kernel)
    for k, v in c.geom:
        assert geom.get(k) == v, (c.id, kernel, k, geom)


# ------------------------------------------------------------------------------------------------------------------------------
# per-field masks (Filter(nan_mask=True): the PF instantiations) on top of a plan mask that is a coastline
# ------------------------------------------------------------------------------------------------------------------------------
NAN_MASK_CASES = [("REGULAR_WITH_LAND", "speckle"), ("REGULAR_WITH_LAND_AREA_WEIGHTED", "channels"),
                  ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "fold")]


@pytest.mark.gpu
@pytest.mark.parametrize("evaluation", ["auto", "reference"])
@pytest.mark.parametrize("kind,coast", NAN_MASK_CASES)
def test_nan_mask_on_a_coastline(kind, coast, evaluation):
    """Batch entry b is filtered with coastline * [field_b is not NaN]: the oracle per entry with that mask.  This module's bounds: NaN
    exactly where the input has it and where the oracle has it, 1e-12 of the oracle's largest value, bit for bit under
    evaluation="reference"; the per-field instantiation of a blocked kernel ran on the strips (k_ringc / k_ringcs / k_ringcp backward,
    k_ring forward), and the Laplacian of the same plan matches the oracle's on the coastline."""
    from gcm_filters_amd import GridType
    from gcm_filters_amd.kernels import ALL_KERNELS
    from oracle import gcmf_oracle as O
    from test_gpu_dispatch_edges import _rel
    from test_gpu_nan_mask import gappy_stack, make_filter, oracle, plan_of

    shape, nb = WIDE, 3
    gv = {k: v for k, v in T.scalar_grid_vars(kind, shape).items()}
    gv["wet_mask"] = T.coastline(coast, shape, seed=5, tripolar=kind.startswith("TRIPOLAR"))
    stack = gappy_stack(shape, nb, seed=11 + len(coast))
    flt = make_filter(kind, gv, evaluation)
    plan = plan_of(kind, gv, "f8", shape)
    plan.last_kernel()
    got = flt.apply(stack)
    ran = plan.last_kernel()
    assert flt.last_path == "strips"
    blocked = ("k_ringc<", "k_ringcs<", "k_ringcp<") if evaluation == "auto" else ("k_ring<",)
    assert ran.startswith(tuple("gcmf::" + k for k in blocked)), ran
    assert np.array_equal(np.isnan(got), np.isnan(stack))
    want = oracle(flt, kind, stack, gv)
    assert np.isfinite(want).any() and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (kind, coast, evaluation, ran, "NaN pattern differs")
    e = _rel(got, want)
    print(f"\n{kind} {coast} {evaluation}: {ran} filter {e:.3e}")
    assert e <= 1e-12, (kind, coast, evaluation, ran, e)
    if evaluation == "reference":
        assert np.array_equal(got, want, equal_nan=True), (kind, coast, ran, "not bit-equal to the oracle")
    lap_in = T.treat_land(np.stack([T.random_field(shape, 100 + b) for b in range(nb)]), gv["wet_mask"], "nan")
    lap = ALL_KERNELS[GridType[kind]](**gv)(lap_in)
    with np.errstate(all="ignore"):
        ltruth = O.make_laplacian(kind, gv)(lap_in)
    assert np.array_equal(np.isnan(lap), np.isnan(ltruth)), (kind, coast, "Laplacian NaN pattern differs")
    assert _rel(lap, ltruth) <= 1e-12, (kind, coast, "Laplacian", _rel(lap, ltruth))
