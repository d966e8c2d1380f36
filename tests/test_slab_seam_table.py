"""The slab-seam table (tests/test_gpu_slab_seams.py) without a GPU: every row has on its seam what it claims, every backward kernel form has
a witness on a ring with a live seam, and the exemptions of the seam-must-matter test are exactly the seam-closed rows."""
import numpy as np

from gcm_filters_amd import testing as T
from test_gpu_slab_seams import CASES, EXEMPT, SeamCase, grid_and_roll, rolled_mask, seam_faces


def test_ids_are_unique_and_the_table_is_there():
    assert len({c.id for c in CASES}) == len(CASES) >= 150
    assert all(isinstance(c, SeamCase) for c in CASES)


def test_roll_rows_moves_row_minus_r_onto_row_zero():
    f = np.arange(5 * 3, dtype=float).reshape(5, 3)
    (g, b), gv = T.roll_rows(-2, [f, np.stack([f, -f])], {"a": f})
    assert np.array_equal(g[0], f[2]) and np.array_equal(g[-1], f[1]) and np.array_equal(b[1, 0], -f[2]) and np.array_equal(gv["a"], g)
    assert g.flags.c_contiguous
    assert T.live_seam_faces(np.array([[1, 1, 0], [0, 0, 0], [1, 0, 0]])) == 1
    assert T.live_seam_faces(np.ones((3, 3)), np.array([[0, 1, 1], [1, 1, 1], [1, 1, 1]])) == 2
    assert T.live_seam_faces(np.array([[1, 1, 1, 1], [1, 1, 0, 1]]), mom5=True) == 2      # (x is periodic: columns 3 and 0 are neighbours)


def test_every_row_has_on_its_seam_what_it_claims():
    for c in CASES:
        if not c.coast.partition(":")[0]:      # no coastline ("", or the B-grid's ":irr": irregular metrics, still no mask)
            assert c.live and not c.closed_in and c.grid in ("REGULAR", "REGULAR_AREA_WEIGHTED", "VECTOR_B_GRID"), c.id
            continue
        if c.grid == "VECTOR_C_GRID":
            gv, roll = grid_and_roll(c)
            t = np.roll(gv["wet_mask_t"], roll, axis=0)
            assert c.live and T.live_seam_faces(t) > 0, c.id
            continue
        wet, kappa_s = rolled_mask(c)
        ny = c.shape[0]
        live = seam_faces(c)
        assert (live > 0) == c.live, (c.id, live)
        closed = T.closed_in_cells(wet)
        if c.closed_in:
            assert closed[0 if c.closed_in == "first" else ny - 1].any(), (c.id, c.closed_in)
        if c.seam_nans:
            halo = 8
            assert sum(bool(wet[j].any()) for j in (0, ny - 1, halo - 1, ny - halo)) == 4, c.id
        if c.coast.startswith("on_the_cuts"):
            assert ny % c.halo == 0 and c.cuts == (c.halo,) and c.overlap, c.id


def test_the_rows_the_table_was_checked_on():
    """The counts the table's comments quote (96 x 128, seed 55)."""
    by_id = {c.id: c for c in CASES}
    for cid, n in (("coast-IRREGULAR_WITH_LAND-open_south-r0", 117), ("coast-IRREGULAR_WITH_LAND-open_south-r47", 51),
                   ("coast-IRREGULAR_WITH_LAND-speckle-r0", 54), ("coast-IRREGULAR_WITH_LAND-channels-r49", 7),
                   ("coast-IRREGULAR_WITH_LAND-channels-r50", 7), ("coast-IRREGULAR_WITH_LAND-lakes-r0", 2),
                   ("coast-IRREGULAR_WITH_LAND-checker-odd", 64), ("coast-IRREGULAR_WITH_LAND-checker-r0", 0),
                   ("coast-IRREGULAR_WITH_LAND-speckle:kappa-row0", 0)):
        assert T.live_seam_faces(*rolled_mask(by_id[cid])) == n, cid
    wet, _ = rolled_mask(by_id["coast-MOM5U-checker-r0"])
    assert np.array_equal(T.closed_in_cells(wet), wet == 1)                   # every wet cell of the even checkerboard is closed in
    wet, _ = rolled_mask(by_id["coast-REGULAR_WITH_LAND_AREA_WEIGHTED-checker-odd"])
    faces = sum((wet * np.roll(wet, s, axis=a)).sum() for a in (0, 1) for s in (1,))
    assert faces == 64                                                       # the odd one's only open faces are those across the seam
    wet, ks = rolled_mask(by_id["coast-IRREGULAR_WITH_LAND-speckle:kappa-row0"])
    assert not ks[0].any() and T.live_seam_faces(wet) > 0                    # closed by kappa alone
    wet, ks = rolled_mask(by_id["coast-IRREGULAR_WITH_LAND-speckle:kappa-rowlast"])
    assert not ks[-1].any() and ks[0].all()
    for cid, row in (("coast-MOM5U-one_land_cell-r48", 0), ("coast-MOM5U-one_land_cell-r49", 95), ("coast-MOM5U-lakes-r32", 0),
                     ("coast-MOM5U-lakes-r33", 95)):
        wet, _ = rolled_mask(by_id[cid])
        want_wet = "lakes" in cid
        assert (wet[row] == (1 if want_wet else 0)).sum() == 1, cid
    assert "coast-MOM5U-checker-odd" not in by_id and seam_faces(by_id["coast-MOM5U-channels-r51"]) > 0
    wet, _ = rolled_mask(by_id["coast-MOM5U-channels-r51"])
    assert (wet[-2] == 1).sum() == 8                                         # the wall is the last row but one
    wet, _ = rolled_mask(by_id["coast-MOM5U-channels-r6"])
    assert wet[0].all()                                                      # a strait row is row 0


def test_every_backward_form_has_a_live_seam_witness():
    reached = {k: [c.id for c in CASES if k in c.reaches] for k in ("k_ringc", "k_ringcs", "k_ringcz", "k_ringcp")}
    for k, ids in reached.items():
        assert ids, f"{k} has no witness in the slab-seam table"
    for c in CASES:
        for k in c.reaches:
            assert c.live and c.backward and c.kernel.startswith(k + "<"), (c.id, k, c.kernel)
    nines = [c for c in CASES if "k_ringc" in c.reaches]
    assert all(r", 9, " in c.kernel and dict(c.expect).get("cut9") == 1 for c in nines)      # plain k_ringc: at nine levels


def test_the_exemptions_are_exactly_the_seam_closed_rows():
    assert {c.exempt for c in CASES if c.exempt} == set(EXEMPT)
    for c in CASES:
        assert bool(c.exempt) == (not c.live), c.id
        if c.exempt:
            assert not c.vec and c.coast
            assert seam_faces(c) == 0, c.id


def test_the_table_covers_what_it_promises():
    modes = {(c.grid, c.dt, c.ev) for c in CASES}
    for grid in ("REGULAR", "REGULAR_AREA_WEIGHTED", "REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5U", "MOM5T"):
        for dt, ev in (("f8", "auto"), ("f8", "reference"), ("f4", "auto"), ("f4", "backward")):
            assert (grid, dt, ev) in modes, (grid, dt, ev)
            if grid not in ("REGULAR", "REGULAR_AREA_WEIGHTED"):
                assert {"speckle", "channels"} <= {c.coast for c in CASES if (c.grid, c.dt, c.ev) == (grid, dt, ev)}, (grid, dt, ev)
    assert {"VECTOR_C_GRID", "VECTOR_B_GRID"} <= {c.grid for c in CASES}
    assert {c.halo for c in CASES if isinstance(c.halo, str)} == {"cut-1", "cut", "cut+1", "2cut-1", "2cut", "n"}
    assert {1, 3, 16} <= {c.nb for c in CASES}
    assert {c.land_values for c in CASES} == set(T.LAND_TREATMENTS)
    assert [c.id for c in CASES if c.land_values == "mixed"] == [c.id for c in CASES if c.seam_nans] == ["gaps-on-sent-rows"]
    assert {c.shape[0] for c in CASES if c.overlap and "overlap" in c.id} == {31, 32, 33}
    assert sum(c.rccl for c in CASES) <= 4 and {c.grid for c in CASES if c.rccl} == {"IRREGULAR_WITH_LAND", "MOM5U"}
    assert any(c.shape[1] == 132 for c in CASES) and any(c.shape[1] == 66 for c in CASES)
