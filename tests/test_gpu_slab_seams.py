"""The row-slab drivers on a ring of ONE rank whose seam is moved onto coastlines, gaps and halo edges, against the oracle.

``SlabFilter(..., rank=0, world=1, self_ring=True)`` keeps ghost rows and exchanges them with itself across row ny-1 / row 0: the whole slab
choreography (the Python forward loop of ``apply_local``, ``_apply_backward``, ``gcmf_slab_apply_backward``,
``gcmf_slab_apply_backward_vec``, the edge / interior split of the overlapped exchange, ``zero_land`` on received ghost rows) in one process.
``testing.land_mask`` makes row 0 land, so on every land-aware kind that seam is a closed face and ghost rows full of garbage pass.  Here every
grid plane and the field are rolled by ``r`` rows (``testing.roll_rows``) before anything is built, which puts the seam on the feature a row of
the table names; the oracle gets the rolled planes as its global grid.

Every case
* filters a DECOY batch first (other seeds, finite everywhere) through the same ``SlabFilter``: a ghost row or state plane that is not
  refreshed then holds plausible wrong numbers, not the allocator's zeros;
* must give the oracle's NaN pattern and an error within ``test_gpu_dispatch_edges.errors()``'s bound for its dtype and scheme;
* scalar kinds: the native driver (``gcmf_slab_apply_backward``) and the Python choreography must give the same bits, and both the bits of
  ``Filter.apply`` of the same evaluation on the same rolled grid (levels are the same arithmetic however they are cut: the claim of
  host_blocks.py, test_gpu_exchange.py and test_gpu_cut_contract.py) -- f64 backward and the forward scheme; f32 backward within 1e-5;
* vector kinds: 1e-13 (f64) / 1e-5 (f32) of the one-plan result.

``test_the_seam_matters`` runs every case with a live seam with the exchange turned into a no-op: the result must then be wrong by at least
100 x the case's bound on a row within ``halo`` of the seam -- a case that passes with stale ghost rows checks nothing.

``CASES`` imports without a GPU (tests/test_slab_seam_table.py checks what each row claims about its seam).
"""
from __future__ import annotations

import functools
import re
import warnings
from dataclasses import dataclass
from typing import Tuple, Union

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from test_gpu_dispatch_edges import _t, errors

FLUX_KINDS = ("IRREGULAR_WITH_LAND", "MOM5U")
MASK_KIND = "REGULAR_WITH_LAND_AREA_WEIGHTED"
NO_MASK = ("REGULAR", "REGULAR_AREA_WEIGHTED", "VECTOR_B_GRID")
SCALAR_KINDS = ("REGULAR", "REGULAR_AREA_WEIGHTED", "REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5U",
                "MOM5T")
SEED = 55
# seam-closed rows of the table: no flux crosses row ny-1 / row 0, so stale ghost rows cannot show -- exempt from test_the_seam_matters
EXEMPT = {
    "all_land": "no wet cell at all",
    "checker-even": "checkerboard on an even ny: every wet cell is closed in (k_land_fix alone), no flux anywhere",
    "lake-on-seam-row": "the one-cell lake is the only wet cell of the seam rows, and it is closed in",
    "kappa-closed": "the all-zero row of kappa_s is row 0: kappa alone closes every face across the seam",
}


@dataclass(frozen=True)
class SeamCase:
    id: str
    grid: str
    dt: str                              # f8 | f4
    ev: str                              # SlabFilter(evaluation=...): auto | reference | backward
    coast: str                           # testing.coastline name ("name:kappa": with testing.kappa_with_zeros; C-grid "name:indq"); "" = a kind without a mask
                                         # a vector kind with a last variant ":irr" ("name:indq:irr", B-grid ":irr"): testing.vector_grid_vars_irregular
    roll: Union[int, str]                # rows the planes and the field are rolled by; "kappa0" / "kappa-1": the all-zero row of kappa_s -> row 0 / row ny-1
    halo: Union[int, str]                # an int, or relative to the backward cut of THIS plan: "cut-1", "cut", "cut+1", "2cut-1", "2cut"; "n" = n_steps
    kernel: str                          # regex sf.engine.plan.last_kernel() must match
    shape: Tuple[int, int] = (96, 128)
    nb: int = 1
    n_steps: int = 24
    land_values: str = "nan"             # testing.LAND_TREATMENTS
    seam_nans: bool = False              # a NaN in one wet cell on each of rows 0, ny-1, halo-1, ny-halo
    overlap: bool = False                # sf.overlap = True: the edge / interior split wherever ro >= 4 * halo
    options: Tuple = ()                  # sf.engine.plan.set_option(name, value)
    cuts: Tuple = ()                     # `on_the_cuts`: strip cuts
    rccl: bool = False                   # also through exchange="native" (RCCL, a communicator of one rank)
    expect: Tuple = ()                   # what the case is meant to reach: see _check_expect
    live: bool = True                    # claim: some face between row ny-1 and row 0 carries flux
    closed_in: str = ""                  # claim: a closed-in wet cell on the "first" / "last" owned row
    exempt: str = ""                     # key of EXEMPT: why the seam is closed
    reaches: Tuple = ()                  # backward kernel forms this case is the live-seam witness for
    scheme: str = "forward"              # f32 error policy of test_gpu_dispatch_edges.errors()

    @property
    def vec(self):
        return self.grid in T.VECTOR_GRIDS

    @property
    def backward(self):
        """The slab is meant to evaluate backwards (scalar kinds)."""
        return (not self.vec and (self.ev == "backward" or (self.ev == "auto" and self.dt == "f8")) and self.halo != "cut-1"
                and dict(self.expect).get("backward", 1) == 1)


CASES = []


def add(c: SeamCase):
    assert c.id not in {x.id for x in CASES}, c.id
    assert bool(c.exempt) == (not c.live) and (not c.exempt or c.exempt in EXEMPT), c.id
    CASES.append(c)


FWD = r"k_(ring|scalar_multi|flux_multi2|scalar_step)<"


def _kernel(grid, dt, ev, halo="cut"):
    """The loosest honest regex: the family of kernels a (kind, dtype, evaluation) runs on a slab; the witnesses below name one form."""
    ty = "double" if dt == "f8" else "float"
    if grid == "VECTOR_C_GRID":
        return r"k_cgrid_(ring|stream2c)<" if (ev != "reference" and halo >= 4) else r"k_cgrid_(ringf|stream2|stream|step)<"
    if grid == "VECTOR_B_GRID":
        return r"k_bgrid_stream2c<" if (ev != "reference" and halo >= 4) else r"k_bgrid_(stream2|stream|step)<"
    back = (ev == "backward" or (ev == "auto" and dt == "f8")) and halo != "cut-1"
    return rf"k_ringc[szp]?<{ty}, " if back else FWD + ty


MODES = (("f8", "auto"), ("f8", "reference"), ("f4", "auto"), ("f4", "backward"))


def _shape(dt, ev):
    return (96, 256) if (dt, ev) == ("f4", "backward") else (96, 128)      # f32 backward windows hold 240 columns: two of them


def _every_kind():
    """Every (kind, dtype, evaluation) on `speckle` (seam on row 0) and `channels` rolled so that a strait row becomes row 0."""
    k = 0
    for grid in SCALAR_KINDS:
        for dt, ev in MODES:
            back = ev == "backward" or (ev, dt) == ("auto", "f8")
            for coast, roll in ((("", 0),) if grid in NO_MASK else (("speckle", 0), ("channels", -6))):
                k += 1
                add(SeamCase(f"kind-{grid}-{dt}-{ev}-{coast or 'nomask'}", grid, dt, ev, coast, roll, "cut" if back else (8, 5)[k % 2],
                             _kernel(grid, dt, ev), shape=_shape(dt, ev), nb=(1, 3)[k % 2], land_values=("nan", "finite")[(k // 2) % 2],
                             scheme="scalar_backward" if (dt, ev) == ("f4", "backward") else "forward"))
    # vector kinds: halo 3 = the Python forward loop, halo 4 = gcmf_slab_apply_backward_vec; C-grid f32 with 4 and with 8 levels (16 blocks per
    # state: the packed message), also with a wet_mask_q of its own
    for coast, roll in (("speckle", 0), ("channels", -6), ("speckle:indq", 0), ("channels:indq", -6)):
        for dt, nb, halo in (("f4", 4, 3), ("f4", 4, 4), ("f4", 8, 4), ("f8", 3, 4)):
            if ":" in coast and (dt, nb) != ("f4", 4):
                continue
            add(SeamCase(f"kind-VECTOR_C_GRID-{dt}-nb{nb}-h{halo}-{coast}", "VECTOR_C_GRID", dt, "auto", coast, roll, halo,
                         _kernel("VECTOR_C_GRID", dt, "auto", halo), shape=(96, 128), nb=nb, land_values="finite",
                         expect=_t(vec_backward=1 if halo >= 4 else 0), scheme="cgrid_backward" if (dt == "f4" and halo >= 4) else "forward"))
    # (B-grid f32 state evaluates backwards only when asked to, like the scalar kinds)
    for dt, ev, nb, halo in (("f8", "auto", 2, 3), ("f8", "auto", 2, 4), ("f4", "backward", 3, 4), ("f4", "auto", 3, 4)):
        back = halo >= 4 and (dt, ev) != ("f4", "auto")
        add(SeamCase(f"kind-VECTOR_B_GRID-{dt}-{ev}-nb{nb}-h{halo}", "VECTOR_B_GRID", dt, ev, "", -6, halo,
                     _kernel("VECTOR_B_GRID", dt, ev if back else "reference", halo), shape=(96, 128), nb=nb, land_values="finite",
                     expect=_t(vec_backward=1 if back else 0), scheme="bgrid_backward" if (back and dt == "f4") else "forward"))
    # the same drivers cutting and rolling metric planes that differ from one another and vary along x (testing.vector_grid_vars_irregular):
    # on the spherical fixture a ghost row of a coefficient plane read one column off, or one plane sent for another, is the same number
    for dt, nb, halo in (("f4", 4, 3), ("f4", 4, 4), ("f8", 3, 4)):
        add(SeamCase(f"kind-VECTOR_C_GRID-{dt}-nb{nb}-h{halo}-speckle:indq:irr", "VECTOR_C_GRID", dt, "auto", "speckle:indq:irr", 0, halo,
                     _kernel("VECTOR_C_GRID", dt, "auto", halo), shape=(96, 128), nb=nb, land_values="finite",
                     expect=_t(vec_backward=1 if halo >= 4 else 0), scheme="cgrid_backward" if (dt == "f4" and halo >= 4) else "forward"))
    for dt, ev, nb, halo in (("f8", "auto", 2, 3), ("f8", "auto", 2, 4), ("f4", "backward", 3, 4), ("f4", "auto", 3, 4)):
        back = halo >= 4 and (dt, ev) != ("f4", "auto")
        add(SeamCase(f"kind-VECTOR_B_GRID-{dt}-{ev}-nb{nb}-h{halo}-irr", "VECTOR_B_GRID", dt, ev, ":irr", -6, halo,
                     _kernel("VECTOR_B_GRID", dt, ev if back else "reference", halo), shape=(96, 128), nb=nb, land_values="finite",
                     expect=_t(vec_backward=1 if back else 0), scheme="bgrid_backward" if (back and dt == "f4") else "forward"))


# (coastline, roll as a function of ny, live seam, closed-in cell on the first / last owned row, exemption) at 96 x 128, seed 55
def _coast_rows(ny):
    return (
        ("open_south", 0, True, "", ""),                       # 117 live faces across the seam
        ("open_south", -(ny // 2 - 1), True, "", ""),          # the mid-grid land band straddles the seam, 51 live
        ("speckle", 0, True, "", ""),                          # 54 live
        ("checker", 0, False, "first", "checker-even"),        # every wet cell closed in
        ("channels", -6, True, "", ""),                        # a strait row is row 0
        ("channels", -(ny // 2 + 1), True, "first", ""),       # the zonal wall is the first owned row: 7 live, a closed-in cell on row 0
        ("channels", -(ny // 2 + 2), True, "last", ""),        # ... the last owned row
        ("lakes", 0, True, "", ""),                            # the lake across the seam, 2 live
        ("lakes", -(ny // 3), False, "first", "lake-on-seam-row"),
        ("lakes", -(ny // 3) - 1, False, "last", "lake-on-seam-row"),
        ("one_land_cell", -(ny // 2), True, "", ""),           # the land cell on row 0
        ("one_land_cell", -(ny // 2) - 1, True, "", ""),       # ... on row ny-1
        ("all_land", 0, False, "", "all_land"),
    )


def _coast_table():
    """The flux kinds and one land-mask kind carry the whole coastline table in f64 (backward, halo = the deepest launch)."""
    k = 0
    for grid in FLUX_KINDS + (MASK_KIND,):
        kern = _kernel(grid, "f8", "auto")
        for coast, roll, live, closed, exempt in _coast_rows(96):
            k += 1
            if grid == "MOM5U" and (coast, closed) == ("channels", "last"):
                # MOM5 masks the faces along y with wet * E(wet) of their southern row (seam_faces): with the wall ON row ny-1 the seam is
                # closed.  One row further the wall is the last row but one, the seam live, and the wall's faces are inside the rows sent
                roll, closed = roll - 1, ""
            how = "finite" if coast == "all_land" else ("nan", "finite")[k % 2]      # (all_land with NaN on land has no finite cell)
            add(SeamCase(f"coast-{grid}-{coast}-r{-roll}", grid, "f8", "auto", coast, roll, "cut", kern, nb=(1, 3)[(k // 2) % 2], land_values=how,
                         live=live, closed_in=closed, exempt=exempt))
        # an odd ny: the only open faces of the whole checkerboard are the 64 across the seam (MOM5: no two wet cells side by side, so none
        # at all -- the even checkerboard over again)
        if grid != "MOM5U":
            add(SeamCase(f"coast-{grid}-checker-odd", grid, "f8", "auto", "checker", 0, "cut", kern, shape=(95, 128), nb=3))
        # rectangles on both sides of owned rows `halo` and ny - halo, where the overlap split cuts (ny a multiple of the halo); rolled: across the seam
        for roll in (0, -8, -9):
            add(SeamCase(f"coast-{grid}-on_the_cuts-r{-roll}", grid, "f8", "auto", "on_the_cuts", roll, 8, kern, shape=(96, 128), nb=(1, 3)[-roll % 2],
                         cuts=(8,), overlap=True, expect=_t(backward=1)))
    # the seam closed by kappa alone; and the same zero row one row further: the last owned row's southern faces, the seam itself live
    kern = _kernel("IRREGULAR_WITH_LAND", "f8", "auto")
    add(SeamCase("coast-IRREGULAR_WITH_LAND-speckle:kappa-row0", "IRREGULAR_WITH_LAND", "f8", "auto", "speckle:kappa", "kappa0", "cut", kern, nb=3,
                 live=False, exempt="kappa-closed"))
    add(SeamCase("coast-IRREGULAR_WITH_LAND-speckle:kappa-rowlast", "IRREGULAR_WITH_LAND", "f8", "auto", "speckle:kappa", "kappa-1", "cut", kern, nb=1))


def _halo_edges():
    for grid, dt, ev, coast, roll, closed in (("IRREGULAR_WITH_LAND", "f8", "auto", "speckle", 0, ""), ("IRREGULAR_WITH_LAND", "f8", "auto", "channels", -49, "first"),
                                              ("REGULAR_WITH_LAND", "f8", "auto", "speckle", 0, ""), ("IRREGULAR_WITH_LAND", "f4", "backward", "speckle", 0, "")):
        for halo in ("cut-1", "cut+1", "2cut-1", "2cut", "n"):
            # cut-1: the slab gives up the backward evaluation; n: exactly one exchange (the input's ghost rows)
            exp = _t(backward=0) if halo == "cut-1" else _t(backward=1, exchanges=1) if halo == "n" else _t(backward=1)
            add(SeamCase(f"halo-{grid}-{dt}-{coast}-{halo}", grid, dt, ev, coast, roll, halo, _kernel(grid, dt, ev, halo), shape=_shape(dt, ev),
                         nb=3 if halo in ("cut+1", "n") else 1, expect=exp, closed_in=closed, rccl=(grid, dt, halo, coast) == ("IRREGULAR_WITH_LAND", "f8", "n", "speckle"),
                         scheme="scalar_backward" if dt == "f4" and halo != "cut-1" else "forward"))
    # exchange="native" (RCCL) on the two flux kinds at halo = the deepest launch and at halo = n_steps (a communicator per case is slow)
    for grid in FLUX_KINDS:
        for halo in (("cut", "n") if grid == "MOM5U" else ("cut",)):
            add(SeamCase(f"rccl-{grid}-{halo}", grid, "f8", "auto", "open_south", 0, halo, _kernel(grid, "f8", "auto"), nb=2, rccl=True,
                         expect=_t(backward=1, **({"exchanges": 1} if halo == "n" else {}))))
    # a requested halo of 64 on 40 rows is clipped to the slab: the ghost zone is the whole grid
    for dt, ev in (("f8", "auto"), ("f4", "auto"), ("f8", "reference")):
        add(SeamCase(f"halo-whole-grid-{dt}-{ev}", "IRREGULAR_WITH_LAND", dt, ev, "speckle", 0, 64, _kernel("IRREGULAR_WITH_LAND", dt, ev), shape=(40, 128), nb=3,
                     expect=_t(halo=40)))
    # the ro >= 4 * halo edge of the overlap split: ny = 4 halo - 1 (no split), 4 halo, 4 halo + 1 -- backward and forward
    for dt, ev in (("f8", "auto"), ("f4", "auto")):
        for ny in (31, 32, 33):
            add(SeamCase(f"overlap-{dt}-ny{ny}", "IRREGULAR_WITH_LAND", dt, ev, "speckle", 0, 8, _kernel("IRREGULAR_WITH_LAND", dt, ev), shape=(ny, 128), nb=1,
                         overlap=True, expect=_t(overlapped=1 if ny >= 32 else 0, **({"backward": 1} if dt == "f8" else {}))))
    # gaps on rows that are sent: NaN on half the land, three NaN in wet cells, and one on each of rows 0, ny-1, halo-1, ny-halo
    add(SeamCase("gaps-on-sent-rows", "IRREGULAR_WITH_LAND", "f8", "auto", "speckle", 0, "cut", _kernel("IRREGULAR_WITH_LAND", "f8", "auto"), nb=3,
                 land_values="mixed", seam_nans=True, expect=_t(backward=1)))


def _kernel_forms():
    """Each backward form on a ring with a live seam.  The forms are the planner's choice (csrc/gcmf_ringc_cut.hpp ringc_cut): an f64 flux slab
    of 96 x 128 takes zipped pairs, without them the early-exit form; a packed column wins on short slabs of 16 fields in launches of five or
    seven levels (n_steps 12 = 7 + 5: last_kernel() names the deepest launch); nine levels: 27 = 3 x 9 on 216 rows with a ghost zone of 12."""
    I = "IRREGULAR_WITH_LAND"
    add(SeamCase("form-ringcz", I, "f8", "auto", "speckle", 0, "cut", r"k_ringcz<double, \d, ", nb=1, reaches=("k_ringcz",), expect=_t(backward=1)))
    add(SeamCase("form-ringcs", I, "f8", "auto", "channels", -6, "cut", r"k_ringcs<double, \d, ", nb=3, options=_t(ringc_zip=0), reaches=("k_ringcs",),
                 expect=_t(backward=1)))
    add(SeamCase("form-ringcp-flux", I, "f8", "auto", "speckle", 0, "cut", r"k_ringcp<double, 2, 7, ", shape=(48, 128), nb=16, n_steps=12,
                 options=_t(ringc_zip=0), reaches=("k_ringcp",), expect=_t(backward=1)))
    add(SeamCase("form-ringcp-mask", "REGULAR_WITH_LAND", "f8", "auto", "channels", -6, "cut", r"k_ringcp<double, \d, 7, ", shape=(48, 128), nb=16,
                 n_steps=12, reaches=("k_ringcp",), expect=_t(backward=1)))
    add(SeamCase("form-ringcp-f4", I, "f4", "backward", "speckle", 0, "cut", r"k_ringcp<float, ", shape=(96, 256), nb=3, reaches=("k_ringcp",),
                 expect=_t(backward=1), scheme="scalar_backward"))
    nine = dict(shape=(216, 64), nb=2, n_steps=27)
    add(SeamCase("form-nines-ringc", I, "f8", "auto", "speckle", 0, 12, r"k_ringc<double, 2, 9, ", options=_t(ringc_zip=0), reaches=("k_ringc",),
                 expect=_t(backward=1, cut9=1), **nine))
    add(SeamCase("form-nines-ringcz", I, "f8", "auto", "channels", -6, 12, r"k_ringcz<double, 9, ", reaches=("k_ringcz",), expect=_t(backward=1, cut9=1), **nine))
    # nx % 4 == 0 with a ragged second window; nx = 66: no backward cut on a grid with land (land_ok wants nx % 4 == 0)
    add(SeamCase("width-132", I, "f8", "auto", "open_south", 0, "cut", _kernel(I, "f8", "auto"), shape=(96, 132), nb=3, expect=_t(backward=1)))
    add(SeamCase("width-66", I, "f8", "auto", "open_south", 0, 8, FWD + "double", shape=(96, 66), nb=1, expect=_t(backward=0)))


_every_kind()
_coast_table()
_halo_edges()
_kernel_forms()


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (shared between the tests of a case, computed once, never written to)
# ------------------------------------------------------------------------------------------------------------------------------
def grid_and_roll(c: SeamCase):
    """The UNROLLED grid variables (f64) of a case and its roll as a number of rows."""
    name, _, variant = c.coast.partition(":")
    irregular = variant.split(":")[-1] == "irr"      # "name:irr", "name:indq:irr"; the B-grid, which has no mask: ":irr"
    variant = variant.split(":")[0]
    if irregular:
        gv = T.vector_grid_vars_irregular(c.grid, c.shape, coast=name, independent_q=variant == "indq", coast_seed=SEED)
    elif c.grid == "VECTOR_C_GRID":
        gv = T.cgrid_coast_vars(name, c.shape, SEED, independent_q=variant == "indq")
    elif c.vec:
        gv = dict(T.vector_grid_vars(c.grid, c.shape))
    else:
        gv = T.scalar_grid_vars(c.grid, c.shape)
        if name:
            gv["wet_mask"] = T.coastline(name, c.shape, seed=SEED, cuts=c.cuts)
        if variant == "kappa":
            gv["kappa_w"], gv["kappa_s"] = T.kappa_with_zeros(c.shape)
    roll = c.roll
    if isinstance(roll, str):
        js = int(np.nonzero((gv["kappa_s"] == 0).all(axis=1))[0][0])
        roll = -js if roll == "kappa0" else -js - 1
    return gv, roll


def seam_faces(c: SeamCase):
    """Faces between row ny-1 and row 0 of a scalar case that carry flux (testing.live_seam_faces by the kind's own rule)."""
    wet, kappa_s = rolled_mask(c)
    return T.live_seam_faces(wet, kappa_s, mom5=c.grid.startswith("MOM5"))


def rolled_mask(c: SeamCase):
    """(wet mask, kappa_s or None) of a scalar case as the slab sees them."""
    gv, roll = grid_and_roll(c)
    _, gv = T.roll_rows(roll, [], gv)
    return gv.get("wet_mask"), (gv["kappa_s"] if c.coast.endswith(":kappa") else None)


def _fields(c: SeamCase, gv, seed0, how):
    mk = lambda s: np.stack([T.random_field(c.shape, s + 2 * l) for l in range(c.nb)])
    if c.vec:
        return [mk(seed0), mk(seed0 + 1)]
    f = mk(seed0)
    return [T.treat_land(f, gv["wet_mask"], how, SEED) if "wet_mask" in gv else f]


@functools.lru_cache(maxsize=None)
def _inputs_cached(key):
    c, halo = key
    from oracle import gcmf_oracle as O

    gv, roll = grid_and_roll(c)
    fields = _fields(c, gv, 100, c.land_values)
    decoy = _fields(c, gv, 700, "finite")
    fields, gvr = T.roll_rows(roll, fields, gv)
    decoy, _ = T.roll_rows(roll, decoy, gv)
    ny = c.shape[0]
    if c.seam_nans:
        wet = gvr["wet_mask"]
        for j in sorted({0, ny - 1, halo - 1, ny - halo}):
            ii = np.nonzero(wet[j])[0]
            if ii.size:
                fields[0][:, j, ii[(7 * j + 3) % ii.size]] = np.nan
    gvr = {k: v.astype(c.dt) for k, v in gvr.items()}
    fields = [f.astype(c.dt) for f in fields]
    decoy = [f.astype(c.dt) for f in decoy]
    dx = T.grid_dx_min(c.grid, gvr) if O.DIMENSIONAL[c.grid] else 1.0
    spec = O.make_spec(4.0 * dx, dx, "GAUSSIAN", n_steps=c.n_steps)
    f64 = [x.astype("f8") for x in fields]
    gv64 = {k: v.astype("f8") for k, v in gvr.items()}
    with np.errstate(all="ignore"):
        truth = O.filter_func_vec(spec, c.grid, *f64, gv64) if c.vec else (O.filter_func(spec, c.grid, f64[0], gv64),)
        ref32 = None
        if c.dt == "f4":
            ref32 = O.filter_func_vec(spec, c.grid, *fields, gvr) if c.vec else (O.filter_func(spec, c.grid, fields[0], gvr),)
    out = dict(gv=gvr, fields=fields, decoy=decoy, dx=dx, truth=truth, ref32=ref32)
    for v in list(gvr.values()) + fields + decoy + list(truth) + list(ref32 or ()):
        v.setflags(write=False)
    return out


def inputs(c: SeamCase, halo: int):
    # (only `seam_nans` inputs depend on the halo)
    return _inputs_cached((c, halo if c.seam_nans else 0))


def _result(c: SeamCase, inp, got):
    """The dict test_gpu_dispatch_edges.errors() reads; the Laplacian is not this module's subject (its slots hold the oracle's own)."""
    return dict(got=got, truth=inp["truth"], ref32=inp["ref32"], lap=inp["truth"], ltruth=inp["truth"], lref32=inp["ref32"])


# ------------------------------------------------------------------------------------------------------------------------------
# running a case
# ------------------------------------------------------------------------------------------------------------------------------
def make_slab(c: SeamCase, inp, halo, exchange="p2p"):
    from gcm_filters_amd.distributed import SlabFilter

    fk = dict(filter_scale=4.0 * inp["dx"], dx_min=inp["dx"], filter_shape="GAUSSIAN", n_steps=c.n_steps)
    sf = SlabFilter(c.grid, inp["gv"], fk, c.shape[0], c.shape[1], halo=halo, dtype=np.dtype(c.dt), device=0, rank=0, world=1, self_ring=True,
                    exchange=exchange, evaluation=c.ev)
    assert sf.exchange_kind == exchange and sf.n_steps == c.n_steps, (c.id, sf.exchange_kind, sf.n_steps)
    sf.overlap = c.overlap
    for k, v in c.options:
        sf.engine.plan.set_option(k, v)
    return sf


def close_slab(sf):
    import torch
    torch.cuda.synchronize()
    if sf.p2p is not None:
        sf.p2p.close()
    if sf.comm is not None:
        sf.comm.close()
    sf.engine.plan.close()


def resolve_halo(c: SeamCase):
    """The halo of a case in rows.  A halo relative to the backward cut is read from the plan itself: a probe slab with as many ghost rows as
    the filter has steps says how deep the deepest launch of THIS plan and polynomial is."""
    if isinstance(c.halo, int):
        return c.halo, None
    if c.halo == "n":
        return c.n_steps, None
    inp = inputs(c, 8)
    probe = make_slab(c, inp, c.n_steps)
    try:
        assert probe.backward_cut, (c.id, "no backward evaluation on this plan: the case has no cut to sit on")
        deep = max(probe.backward_cut)
    finally:
        close_slab(probe)
    return {"cut-1": deep - 1, "cut": deep, "cut+1": deep + 1, "2cut-1": 2 * deep - 1, "2cut": 2 * deep}[c.halo], deep


def apply_after_decoy(c: SeamCase, sf, inp, native, count=None):
    """Filter the decoy batch, then the case's batch, through the same SlabFilter; returns the second result (host, f64) and the kernel."""
    sf.native_driver = native
    sf.apply_local(sf.scatter_from_global(inp["decoy"]))
    sf.synchronize()
    sf.engine.plan.last_kernel()
    before = sf.exchanges
    if count is not None:           # exchanges posted for the overlap with an interior launch = _exchange_start calls not made by _exchange
        whole, start = sf._exchange, sf._exchange_start

        def counted_whole(tensors):
            count["whole"] += 1
            return whole(tensors)

        def counted_start(tensors):
            count["start"] += 1
            return start(tensors)

        sf._exchange, sf._exchange_start = counted_whole, counted_start
    got = [t.cpu().numpy().copy() for t in sf.apply_local(sf.scatter_from_global(inp["fields"]))]
    sf.synchronize()
    if count is not None:
        del sf._exchange, sf._exchange_start
    assert not sf.p2p_timed_out()
    return got, sf.engine.plan.last_kernel(), sf.exchanges - before


def one_plan(c: SeamCase, inp, ev):
    from gcm_filters_amd import Filter, FilterShape, GridType
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flt = Filter(filter_scale=4.0 * inp["dx"], dx_min=inp["dx"], n_steps=c.n_steps, filter_shape=FilterShape.GAUSSIAN, grid_type=GridType[c.grid],
                     grid_vars=inp["gv"], evaluation=ev)
    assert flt.n_steps == c.n_steps
    return flt.apply_to_vector(*inp["fields"]) if c.vec else (flt.apply(inp["fields"][0]),)


def _check_expect(c: SeamCase, sf, deep, nex, count):
    for what, want in c.expect:
        if what == "backward":
            assert bool(sf.backward_cut) == bool(want), (c.id, sf.halo, sf.backward_cut)
            if want and deep is not None:
                assert max(sf.backward_cut) == deep, (c.id, "the cut moved with the halo", sf.backward_cut, deep)
        elif what == "exchanges":
            assert nex == want, (c.id, nex)
        elif what == "halo":
            assert sf.halo == want and sf.rows_alloc == 3 * want, (c.id, sf.halo, sf.rows_alloc)
        elif what == "cut9":
            assert max(sf._cut_for(c.nb)) == 9, (c.id, sf._cut_for(c.nb))
        elif what == "vec_backward":
            assert sf._vec_backward.get(c.nb, 0) == want, (c.id, sf._vec_backward)
        elif what == "overlapped":
            assert (count["start"] - count["whole"] > 0) == bool(want), (c.id, count, sf.rows_owned, sf.halo)
        else:
            raise KeyError(what)


def _same_nan(got, want, what):
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert np.array_equal(np.isnan(g), np.isnan(w)), what


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_slab_seam(c):
    from gcm_filters_amd.kernels import clear_plan_cache

    halo, deep = resolve_halo(c)
    inp = inputs(c, halo)
    sf = make_slab(c, inp, halo)
    results = {}
    try:
        assert sf.halo == min(halo, c.shape[0])
        if c.backward:
            assert sf.backward_cut and max(sf._cut_for(c.nb)) <= sf.halo, (c.id, sf.backward_cut, sf.halo)
        native_first = not c.vec or dict(c.expect).get("vec_backward") == 1
        count = {"whole": 0, "start": 0}
        got, kernel, nex = apply_after_decoy(c, sf, inp, native_first)
        results["native" if native_first else "python"] = got
        if not c.vec and sf.backward_cut:
            # the application above ran inside libgcmf in one call (gcmf_slab_apply_backward); the Python choreography gives the same bits
            again, kernel2, nex2 = apply_after_decoy(c, sf, inp, False, count)
            assert nex2 == nex, (c.id, nex, nex2)
            assert re.search(c.kernel, kernel2), (c.id, kernel2)
            results["python"] = again
        elif not c.vec:
            got, kernel, nex = apply_after_decoy(c, sf, inp, False, count)      # (the forward loop again, counting its overlapped exchanges)
            results["python"] = got
        _check_expect(c, sf, deep, nex, count)
    finally:
        close_slab(sf)
    if c.rccl:
        sfn = make_slab(c, inp, halo, exchange="native")
        try:
            results["rccl"], kernel3, nex3 = apply_after_decoy(c, sfn, inp, True)
            assert nex3 == nex and re.search(c.kernel, kernel3), (c.id, nex3, kernel3)
        finally:
            close_slab(sfn)
    r = _result(c, inp, got)
    e, bound, _, _ = errors(c, r)
    print(f"\n{c.id}: halo {halo} cut {sf.backward_cut} {kernel} exchanges {nex} error {e:.3e} (bound {bound:.3e})")
    assert re.search(c.kernel, kernel), (c.id, kernel)
    for how, res in results.items():
        _same_nan(res, inp["truth"], (c.id, how, kernel, "NaN pattern differs from the oracle's"))
        e, bound, _, _ = errors(c, _result(c, inp, res))
        assert e <= bound, (c.id, how, kernel, e, bound)
    for how, res in results.items():
        if how != "native" and "native" in results and not c.vec:
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(res, results["native"])), (c.id, how, "bits differ from the native driver's")
    # the one-plan path on the same rolled grid
    try:
        ev = c.ev if (c.vec or sf.backward_cut or c.dt == "f4") else "reference"      # (a slab without a backward cut runs the forward scheme)
        one = one_plan(c, inp, ev)
    finally:
        clear_plan_cache()
    _same_nan(got, one, (c.id, "NaN pattern differs from the one-plan path's"))
    if not c.vec and not (c.dt == "f4" and c.ev == "backward"):
        for how, res in results.items():
            for a, b in zip(res, one):
                d = np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max()
                assert np.array_equal(a, b, equal_nan=True), (c.id, how, kernel, "not the bits of the one-plan path", float(d))
    else:
        tol = 1e-5 if c.dt == "f4" else 1e-13
        for a, b in zip(got, one):
            ok = ~np.isnan(b)
            if ok.any():
                assert np.abs(a[ok] - b[ok]).max() <= tol * np.abs(b[ok]).max(), (c.id, kernel)


# ------------------------------------------------------------------------------------------------------------------------------
# the seam must matter
# ------------------------------------------------------------------------------------------------------------------------------
_RATIOS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.live], ids=[c.id for c in CASES if c.live])
def test_the_seam_matters(c, monkeypatch):
    """With the exchange a no-op the ghost rows keep the decoy's data (allocated memory of this SlabFilter, read stale): the result must be
    wrong by at least 100 x the case's bound on a row within `halo` of the seam, or the case checks nothing about the seam."""
    from gcm_filters_amd.distributed import SlabFilter

    halo, _ = resolve_halo(c)
    inp = inputs(c, halo)
    sf = make_slab(c, inp, halo)
    try:
        sf.native_driver = False
        sf.apply_local(sf.scatter_from_global(inp["decoy"]))
        sf.synchronize()
        monkeypatch.setattr(SlabFilter, "_exchange", lambda self, tensors: None)
        monkeypatch.setattr(SlabFilter, "_exchange_start", lambda self, tensors: "stub")
        monkeypatch.setattr(SlabFilter, "_exchange_finish", lambda self, ticket: None)
        got = [t.cpu().numpy().copy() for t in sf.apply_local(sf.scatter_from_global(inp["fields"]))]
        sf.synchronize()
    finally:
        close_slab(sf)
    _, bound, _, _ = errors(c, _result(c, inp, got))
    h = min(sf.halo, c.shape[0] // 2)
    worst = 0.0
    for g, w in zip(got, inp["truth"]):
        g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
        fin = ~np.isnan(w)
        scale = np.abs(w[fin]).max()
        d = np.where(np.isnan(g) != np.isnan(w), np.inf, np.abs(np.nan_to_num(g) - np.nan_to_num(w))) / scale
        worst = max(worst, float(d[..., :h, :].max()), float(d[..., -h:, :].max()))
    ratio = worst / bound
    _RATIOS[c.id] = ratio
    print(f"\n{c.id}: without the exchange the rows beside the seam are off by {worst:.3e} = {ratio:.3e} x the bound {bound:.3e}; "
          f"smallest ratio so far {min(_RATIOS.values()):.3e} ({min(_RATIOS, key=_RATIOS.get)})")
    assert ratio >= 100.0, (c.id, worst, bound)
