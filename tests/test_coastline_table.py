"""The coastline sweep's table (tests/test_gpu_coastlines.py) without a GPU: every kernel family is crossed with every coastline of its
grid kinds, and the generators (gcm_filters_amd.testing.coastline) still draw what the sweep relies on -- so a later edit cannot quietly
turn a coastline back into the fixture mask."""
import glob
import os
import re

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from test_gpu_coastlines import CASES, FAMILIES, REFUSED, TABLE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcm_filters_amd", "csrc")
# the kernels the sweep has to reach, by the family ids that reach them
REQUIRED = {
    "k_scalar_step": ("step-f8", "step-f4"),
    "k_scalar_multi": ("multi-mask-f8", "multi-flux-f8", "multi-mask-f4", "multi-flux-f4"),
    "k_flux_multi2": ("flux-multi2-f8", "flux-multi2-f4"),
    "k_ring": ("ring-maskz-f8", "ring-flux-f8", "ring-first-maskz-f8", "ring-first-flux-f8", "ring-first-maskz-f4", "ring-first-flux-f4",
               "ring-maskz-f4", "ring-flux-f4", "tripolar-band-forward"),
    "k_ringc": ("backward-auto", "ringc-maskz", "ringc-flux", "ringc-flux-nozigzag", "ringc9", "tripolar-band-backward"),
    "k_ringcs": ("backward-auto", "ringcs", "ringc-flux-f4", "tripolar-band-backward"),
    "k_ringcz": ("backward-auto", "ringcz", "tripolar-zip"),
    "k_ringcp": ("ringcp",),
    "k_ringc_one": ("ringc-one",),
    "k_resident": ("resident",),
    "k_cgrid_step": ("cgrid-step",),
    "k_cgrid_stream": ("cgrid-stream",),
    "k_cgrid_stream2": ("cgrid-stream2",),
    "k_cgrid_stream2c": ("cgrid-stream2c", "cgrid-stream2c-priv"),
    "k_cgrid_ring": ("cgrid-ring",),
    "k_cgrid_ringf": ("cgrid-ringf",),
}
LAND_KINDS = ("REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5U", "MOM5T",
              "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "TRIPOLAR_POP_WITH_LAND")


def _kernel_names():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(path) as f:
            names.update(re.findall(r"\b(k_[a-z_0-9]+)\b", f.read()))
    return names


def _names_of(regex, names):
    """The kernels of csrc/ whose name the part of a case's regex before the template arguments accepts."""
    return {n for n in names if re.fullmatch(regex.split("<")[0], n)}


def test_every_family_names_exactly_the_kernels_it_is_listed_for():
    names = _kernel_names()
    assert set(REQUIRED) <= names
    listed = {f.id: {k for k, fams in REQUIRED.items() if f.id in fams} for f in FAMILIES}
    for fam in FAMILIES:
        accepted = set()
        for regex in (fam.kernel,) + tuple(r for _, r in fam.kernel_by_grid):
            accepted |= _names_of(regex, names)
        assert accepted == listed[fam.id] != set(), (fam.id, accepted, listed[fam.id])
    assert {fid for fams in REQUIRED.values() for fid in fams} == {f.id for f in FAMILIES}
    for c in CASES:       # a case names one kernel, but for the family whose dispatch is the library's own choice
        assert len(_names_of(c.kernel, names)) == 1 or c.id.startswith("backward-auto-"), (c.id, c.kernel)


def test_every_family_meets_every_coastline_of_its_kinds():
    for fam in FAMILIES:
        want = list(T.coastline_names(fam.tripolar))
        if fam.grids == ("VECTOR_C_GRID",):
            want += ["speckle:indq", "channels:indq"]
        if "IRREGULAR_WITH_LAND" in fam.grids:
            assert fam.kappa, fam.id
            want += ["speckle:kappa", "one_land_cell:kappa"]
        assert {k[1] for k in TABLE if k[0] == fam.id} == set(want), fam.id
        for coast in want:
            cs = TABLE[(fam.id, coast)]
            grids = [c.grid for c in cs]
            if fam.every_grid:
                assert sorted(grids) == sorted(fam.grids), (fam.id, coast, grids)
            else:
                assert len(cs) == 1 and grids[0] in fam.grids, (fam.id, coast, grids)
            for c in cs:
                assert c.coast == coast and c.shape == ((97, 118) if coast in fam.ragged else fam.shape)
                if (fam.id, coast) not in REFUSED:
                    assert c.kernel == dict(fam.kernel_by_grid).get(c.grid, fam.kernel).replace("{K}", r"\d") and c.not_kernel is None
        treatments = {c.land_values for n in want for c in TABLE[(fam.id, n)]}
        # (the C-grid stencil does not mask its input: its fields stay finite, and the cases say so)
        assert treatments == ({"finite"} if fam.grids == ("VECTOR_C_GRID",) else set(T.LAND_TREATMENTS)), fam.id
    assert len({c.id for c in CASES}) == len(CASES) == sum(len(v) for v in TABLE.values())


def test_every_grid_kind_meets_every_coastline():
    met = {(c.grid, c.coast.partition(":")[0]) for c in CASES if (next(k for k, v in TABLE.items() if c in v)) not in REFUSED}
    for grid in LAND_KINDS + ("VECTOR_C_GRID",):
        for coast in T.coastline_names(grid.startswith("TRIPOLAR")):
            assert (grid, coast) in met, (grid, coast)
    assert {c.grid for c in CASES} == set(LAND_KINDS) | {"VECTOR_C_GRID"}
    # every land kind meets every coastline under the forward AND under the backward evaluation
    for ev_is_fwd in (True, False):
        got = {(c.grid, c.coast.partition(":")[0]) for c in CASES if (c.ev == "reference") == ev_is_fwd and not c.not_kernel}
        for grid in LAND_KINDS:
            for coast in T.coastline_names(grid.startswith("TRIPOLAR")):
                assert (grid, coast) in got, (grid, coast, "forward" if ev_is_fwd else "backward")
    # land on the tripole seam: both tripolar kinds in both forms of the seam band, and the flux kind with the seam inside the launch
    for fid in ("tripolar-band-backward", "tripolar-band-forward"):
        assert sorted(c.grid for c in TABLE[(fid, "fold")]) == ["TRIPOLAR_POP_WITH_LAND", "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED"]
    assert [c.grid for c in TABLE[("tripolar-zip", "fold")]] == ["TRIPOLAR_POP_WITH_LAND"]


def test_refused_pairs_name_a_predicate_and_leave_rows_and_columns():
    srcs = "".join(open(p).read() for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert REFUSED
    for (fid, coast), (predicate, reaches) in REFUSED.items():
        assert (fid, coast) in TABLE, (fid, coast)
        assert re.search(r"\bbool " + re.escape(predicate) + r"\(", srcs), f"{predicate} is not a predicate in csrc/"
        fam = next(f for f in FAMILIES if f.id == fid)
        for c in TABLE[(fid, coast)]:
            assert c.kernel in reaches and c.not_kernel == fam.kernel and c.ev == "auto"
            assert c.shape[1] % 4 != 0                       # land_ok: nx % 4 != 0
    for fam in FAMILIES:
        row = [k for k in TABLE if k[0] == fam.id]
        assert any(k not in REFUSED for k in row), f"REFUSED holds the whole row {fam.id}"
    for coast in {k[1] for k in TABLE}:
        col = [k for k in TABLE if k[1] == coast]
        assert any(k not in REFUSED for k in col), f"REFUSED holds the whole column {coast}"


def test_no_case_is_all_nan():
    for c in CASES:
        assert not (c.coast.startswith("all_land") and c.land_values == "nan"), c.id


SHAPES = [(97, 236), (97, 118), (40, 64), (64, 128), (50, 8512)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_generators_draw_what_the_sweep_relies_on(shape):
    ny, nx = shape
    for seed in (0, 7):
        for tripolar in (False, True):
            for name in T.coastline_names(tripolar):
                m = T.coastline(name, shape, seed, tripolar=tripolar, cuts=(20,))
                assert m.shape == shape and m.dtype == np.float64 and set(np.unique(m)) <= {0.0, 1.0}, name
                assert np.array_equal(m, T.coastline(name, shape, seed, tripolar=tripolar, cuts=(20,))), name
                if tripolar:
                    assert not m[0].any(), name
                if name != "all_land":
                    assert (m == 0).any() and (m == 1).any(), name
        m = T.coastline("open_south", shape, seed)
        both = (m[0] == 1) & (m[ny - 1] == 1)
        assert both.any() and m[0].mean() > 0.5 and m[ny - 1].mean() > 0.5          # a live y seam
        assert (m[:, nx - 1] == 0).any() and (m[:, 0] == 0).any() and ((m[:, nx - 1] == 1) & (m[:, 0] == 1)).any()   # and a live, partly closed x seam
        assert ((m[:, nx - 3:] == 0).all(axis=1) & (m[:, :2] == 0).all(axis=1) & (m[:, 2] == 1) & (m[:, nx - 4] == 1)).any()
        for name in ("speckle", "channels"):
            for vec in (2, 4):
                assert T.mixed_words(T.coastline(name, shape, seed), vec) >= 0.10, (name, vec)
        assert abs((T.coastline("speckle", shape, seed) == 0).mean() - 0.35) < 0.05
        for name in ("checker", "lakes", "speckle"):
            assert T.closed_in_cells(T.coastline(name, shape, seed)).any(), name
        m = T.coastline("lakes", shape, seed)
        assert m[ny // 2, nx - 1] == m[ny // 2, 0] == 1 and m[ny - 1].any() and m[0].any() and (m == 0).mean() > 0.98
        assert (T.coastline("one_land_cell", shape, seed) == 0).sum() == 1
        assert np.argwhere(T.coastline("one_land_cell", shape, seed) == 0)[0][1] % 2 == 1
        assert not T.coastline("all_land", shape, seed).any()
        m = T.coastline("fold", shape, seed, tripolar=True)
        top, mirror = m[ny - 1], m[ny - 1, ::-1]
        assert (top != mirror).any()                                   # a seam pair with exactly one land partner
        assert top[nx // 2 - 1] != top[nx // 2] and top[0] != top[nx - 1]   # the middle pair and the end pair among them
        assert (m[ny - 3:, nx // 4] == 0).all()
        m = T.coastline("on_the_cuts", shape, seed, cuts=(20,))
        for wi in T.BACKWARD_WINDOWS:
            if wi + 4 < nx:                                            # land begins and ends on both sides of the cut
                for a, b in ((wi - 1, wi), (wi, wi + 1)):
                    assert ((m[:, a] == 0) & (m[:, b] == 1)).any() and ((m[:, a] == 1) & (m[:, b] == 0)).any(), (wi, a, b)
        for a, b in ((19, 20), (20, 21)):
            assert ((m[a] == 0) & (m[b] == 1)).any() and ((m[a] == 1) & (m[b] == 0)).any(), (a, b)


def test_the_coefficient_recipes():
    shape = (97, 118)
    kw, ks = T.kappa_with_zeros(shape)
    assert kw.max() == 1.0 and ks.max() == 1.0 and (kw == 0).sum() == 54 and (ks == 0).all(axis=1).sum() == 1
    wet = T.coastline("one_land_cell", shape, 0)
    assert ((kw == 0) & (np.roll(kw, -1, axis=1) == 0) & (wet == 1)).any()      # wet cells whose west and east faces kappa closes
    for indq in (False, True):
        gv = T.cgrid_coast_vars("speckle", shape, 3, independent_q=indq)
        assert not np.array_equal(gv["wet_mask_t"], gv["wet_mask_q"])
        assert gv["kappa_aniso"].min() > 0 and gv["kappa_iso"].max() == 1.0
    t, q = (T.cgrid_coast_vars("speckle", shape, 3)[k] for k in ("wet_mask_t", "wet_mask_q"))
    assert np.array_equal(q, t * np.roll(t, -1, 0) * np.roll(t, -1, 1) * np.roll(t, (-1, -1), (0, 1)))


def test_the_land_treatments():
    wet = T.coastline("speckle", (40, 64), 1)
    f = T.random_field((2, 40, 64), 5)
    assert np.array_equal(np.isnan(T.treat_land(f, wet, "nan")), np.broadcast_to(wet == 0, f.shape))
    assert np.isfinite(T.treat_land(f, wet, "finite")).all()
    x = T.treat_land(f, wet, "mixed", 4)
    nanland = np.isnan(x) & (wet == 0)
    assert 0.3 < nanland.sum() / (2 * (wet == 0).sum()) < 0.7 and 1 <= (np.isnan(x[0]) & (wet == 1)).sum() <= 3
