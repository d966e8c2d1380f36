"""Every launchable kernel at the edges of the predicates that select it, against the oracle (oracle/gcmf_oracle.py).

The rest of the GPU suite mostly checks equivalence (kernel A gives kernel B's bits) on shapes well inside each kernel's admission
predicate.  This module is a table: each case names a grid, dtype, shape, batch, n_steps, evaluation and the plan options / tuning /
plan-creation env vars that steer it, the kernel it must reach (a regex on ``Plan.last_kernel()``) and, where it matters, the launch
geometry (``Plan.last_kernel_geometry()``) that shows it sits on the intended side of the edge.  Each case runs the filter (and the
Laplacian) and compares with the oracle:

* f64: relative error <= 1e-12 against the largest absolute value of the oracle's result, identical NaN pattern; bit-equality where the
  suite already holds a family to bits under ``evaluation="reference"`` (REGULAR, land-mask and B-grid kinds);
* f32: the truth is the oracle in f64 on the same values cast up; the kernel's error against it is at most c x the error of the oracle's
  own f32 path plus a small floor, c from the policy the suite states (test_gpu_clenshaw.py): 1.5 x for the forward scheme, 0.8 x for
  C-grid backward, 4 x for B-grid backward; the f32 scalar backward kernels at most 2.5 x the forward scheme's error plus 2e-6 of the
  result's largest value.

The edges come from the predicates in csrc/: ``multi_supported`` / ``cgrid_multi_supported`` / ``bgrid_multi_supported`` /
``cgrid_ring_supported`` admit ``rows >= S + 2`` (tripolar scalar: ``rows >= 3S + 2``), and only ``nx % VEC == 0`` in x; the backward
scalar kernels cut x into windows of WI = 64 VEC - 2M useful columns (112 for f64 at S <= 8, 108 at S = 9, 240 for f32).

``CASES`` imports without a GPU: tests/test_kernel_inventory.py checks that every kernel in csrc/ is reached by a case here.
"""
from __future__ import annotations

import math
import re
import warnings
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest

from gcm_filters_amd import testing as T

BIT_EXACT = {"REGULAR", "REGULAR_AREA_WEIGHTED", "REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED",
             "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "VECTOR_B_GRID"}
WI_F64, WI_F64_9, WI_F32 = 112, 108, 240       # useful columns of a backward scalar window (gcmf_api.hip launch_ringc)
KIND_REG, KIND_MASK, KIND_FLUX = 0, 5, 2        # the KIND template argument in kernel names (K_REG, K_MASK, K_FLUX; csrc/gcmf_internal.hpp)
SCALAR_KIND = {"REGULAR": KIND_REG, "REGULAR_WITH_LAND": KIND_MASK}
LAND_KINDS = {"REGULAR_WITH_LAND", "REGULAR_WITH_LAND_AREA_WEIGHTED", "IRREGULAR_WITH_LAND", "MOM5U", "MOM5T",
              "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "TRIPOLAR_POP_WITH_LAND"}


@dataclass(frozen=True)
class Case:
    id: str
    grid: str
    dt: str
    shape: Tuple[int, int]
    kernel: str                         # regex that Plan.last_kernel() must match
    nb: int = 0                         # 0: one unbatched field
    n_steps: int = 24
    ev: str = "auto"
    tuning: Tuple = ()                  # Plan.set_tuning(**dict(tuning))
    options: Tuple = ()                 # Plan.set_option(name, value) for each pair
    env: Tuple = ()                     # plan-creation env vars (monkeypatch.setenv, then clear_plan_cache)
    not_kernel: Optional[str] = None    # regex last_kernel() must NOT match (the refused side of an edge)
    geom: Tuple = ()                    # required entries of Plan.last_kernel_geometry()
    scheme: str = "forward"             # f32 error policy: forward | scalar_backward | cgrid_backward | bgrid_backward
    reaches: Tuple = ()                 # kernel names (without "gcmf::") this case is the inventory's witness for
    land: bool = True                   # False: an all-ocean wet_mask (no land fix-up, so no nx % 4 condition on the backward evaluation)
    coast: str = ""                     # a coastline of testing.COASTLINES instead of the fixture mask ("name", "name:kappa": with
                                        # testing.kappa_with_zeros, C-grid "name:indq": an independent wet_mask_q); tests/test_gpu_coastlines.py
    land_values: str = "nan"            # the values on land of a `coast` case: testing.LAND_TREATMENTS
    metrics: str = ""                   # "irregular": a vector kind on testing.vector_grid_vars_irregular (tests/test_gpu_vector_metrics.py)

    def kernels(self):
        """The kernels this case reaches: `reaches`, else the one its regex names (a regex over several names names none)."""
        m = re.match(r"(k_[a-z_0-9]+)[<\[]", self.kernel)
        return self.reaches or ((m.group(1),) if m else ())


def _t(**kw):
    return tuple(sorted(kw.items()))


CASES = []


def add(c: Case):
    assert c.id not in {x.id for x in CASES}, c.id
    CASES.append(c)


# ---- rows: S+1 (refused), S+2 (the bound), S+3, 2S+1, 2S+2 -- the S ghost rows of a strip wrap across the periodic y seam ----------
def _rows_family():
    nx = 64
    for dt in ("f8", "f4"):
        ty = "double" if dt == "f8" else "float"
        S = 8
        # forward static-ring kernel k_ring in its reg / maskz / flux forms (multi_s=S; the first launch of a filter is not a ring launch)
        for grid in ("REGULAR", "REGULAR_WITH_LAND", "IRREGULAR_WITH_LAND"):
            for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
                deep = rf"k_ring<{ty}, double, \d, {S}, "
                add(Case(f"rows-ring-{grid}-{dt}-{rows}", grid, dt, (rows, nx), r"k_(ring|scalar_multi|flux_multi2|scalar_step)<" if rows == S + 1 else deep,
                         ev="reference", tuning=_t(multi_s=S, clenshaw=0), not_kernel=deep if rows == S + 1 else None,
                         reaches=("k_ring",) if rows > S + 1 else ()))
    # the general blocked kernel k_scalar_multi (reg / mask / flux forms): depths below the ring kernels' 5 (ring_supported and
    # flux_multi2_supported both need S >= 5), so no env var is needed to reach its flux form
    S = 4
    for dt in ("f8", "f4"):
        ty = "double" if dt == "f8" else "float"
        for grid in ("REGULAR", "REGULAR_WITH_LAND", "IRREGULAR_WITH_LAND"):
            for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
                deep = rf"k_scalar_multi<{ty}, double, \d, {S}, "
                add(Case(f"rows-multi-{grid}-{dt}-{rows}", grid, dt, (rows, 64), r"k_" if rows == S + 1 else deep, ev="reference",
                         tuning=_t(multi_s=S, clenshaw=0), not_kernel=deep if rows == S + 1 else None,
                         reaches=("k_scalar_multi",) if rows > S + 1 else ()))
    # backward f64: k_ringc (plain), k_ringcs (early exit), k_ringcz (strips zipped in pairs) at depth S = ringc_smax
    S = 8
    for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
        deep_any = rf"k_ringc[sz]?<double, (\d, )?{S}, "
        refused = rows == S + 1
        for form, opts, env in (("ringc", _t(ringc_smax=S, ringc_zip=0), _t(GCMF_RINGC_XE_ROWS="0")),
                                ("ringcs", _t(ringc_smax=S, ringc_zip=0), ()),
                                ("ringcz", _t(ringc_smax=S, ringc_zip=1), ())):
            want = {"ringc": rf"k_ringc<double, 2, {S}, ", "ringcs": rf"k_ringcs<double, {S}, ", "ringcz": rf"k_ringcz<double, {S}, "}[form]
            add(Case(f"rows-{form}-f8-{rows}", "IRREGULAR_WITH_LAND", "f8", (rows, nx), r"k_" if refused else want, options=opts, env=env,
                     not_kernel=deep_any if refused else None, reaches=() if refused else (f"k_{form}",)))
        for grid in ("REGULAR", "REGULAR_WITH_LAND"):
            want = rf"k_ringc<double, {SCALAR_KIND[grid]}, {S}, "
            add(Case(f"rows-ringc-{grid}-f8-{rows}", grid, "f8", (rows, nx), r"k_" if refused else want, options=_t(ringc_smax=S),
                     not_kernel=deep_any if refused else None, reaches=() if refused else ("k_ringc",)))
    # f32 state: at most seven levels per backward launch, but clenshaw_cut offers the backward evaluation only where multi_supported(pl, 8)
    # holds (gcmf_api_blocks.hip), so the row bound is 8 + 2 = 10 here too
    S = 7
    for rows in (9, 10, 11, 2 * S + 1, 2 * S + 2):
        refused = rows == 9
        add(Case(f"rows-ringc-f4-{rows}", "IRREGULAR_WITH_LAND", "f4", (rows, nx), r"k_" if refused else rf"k_ringcs?<float, (2, )?{S}, ",
                 ev="backward", options=_t(ringc_smax=8), not_kernel=rf"k_ringc[sz]?<float, (\d, )?{S}, " if refused else None,
                 scheme="scalar_backward", reaches=() if refused else ("k_ringc",)))
    # vector kernels: C-grid f64 (S <= 4), f32 batched levels k_cgrid_ring (S = cgrid_ring_smax = 6) and k_cgrid_ringf (S = 5), B-grid
    for dt, S, nb, ev, want, opts, scheme in (
            ("f8", 4, 3, "reference", r"k_cgrid_stream2<double, double, 2, 4, ", (), "forward"),
            ("f8", 4, 3, "auto", r"k_cgrid_stream2c<double, 2, 4, ", (), "forward"),
            ("f4", 6, 4, "auto", r"k_cgrid_ring<float, 6, ", _t(cgrid_ring_smax=6), "cgrid_backward"),
            ("f4", 5, 4, "reference", r"k_cgrid_ringf<float, 5, ", (), "forward")):
        fam = re.match(r"(k_[a-z_0-9]+)", want).group(1)
        for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
            refused = rows == S + 1
            add(Case(f"rows-{fam}-{dt}-{ev}-{rows}", "VECTOR_C_GRID", dt, (rows, nx), r"k_cgrid_" if refused else want, nb=nb, ev=ev,
                     options=opts, not_kernel=want if refused else None, scheme=scheme, reaches=() if refused else (fam,)))
    # single-level vector fields: the wave-private coefficient rings (PRIV = true; GCMF_VEC_PRIV=0 gives the lock-step form the batched
    # cases above run)
    S = 4
    for grid, dt, want in (("VECTOR_C_GRID", "f8", r"k_cgrid_stream2c<double, 2, 4, \d, true>"),
                           ("VECTOR_C_GRID", "f4", r"k_cgrid_stream2c<float, 2, 4, \d, true>"),
                           ("VECTOR_B_GRID", "f8", r"k_bgrid_stream2c<double, 2, 4, \d, true>")):
        fam = re.match(r"(k_[a-z_0-9]+)", want).group(1)
        for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
            refused = rows == S + 1
            add(Case(f"rows-priv-{grid}-{dt}-{rows}", grid, dt, (rows, 64), r"k_" if refused else want, not_kernel=want if refused else None,
                     tuning=_t(clenshaw=2, multi_s=8), scheme="cgrid_backward" if dt == "f4" else "forward", reaches=() if refused else (fam,)))
    for dt, ev, want, scheme in (("f8", "reference", r"k_bgrid_stream2<double, double, 2, 4, ", "forward"),
                                 ("f8", "auto", r"k_bgrid_stream2c<double, 2, 4, ", "forward"),
                                 ("f4", "backward", r"k_bgrid_stream2c<float, 2, 4, ", "bgrid_backward")):
        S = 4
        fam = re.match(r"(k_[a-z_0-9]+)", want).group(1)
        for rows in (S + 1, S + 2, S + 3, 2 * S + 1, 2 * S + 2):
            refused = rows == S + 1
            add(Case(f"rows-{fam}-{dt}-{ev}-{rows}", "VECTOR_B_GRID", dt, (rows, nx), r"k_bgrid_" if refused else want, nb=3, ev=ev,
                     tuning=_t(clenshaw=2, multi_s=8) if ev == "auto" else (), not_kernel=want if refused else None, scheme=scheme,
                     reaches=() if refused else (fam,)))
    # tripolar: the seam's top S rows -- rows 3S+1 (refused), 3S+2, 3S+3; the seam inside the launch (k_ringcz, zip_fold) and in
    # k_fold_band (zip_fold=0, and the forward scheme)
    S = 8
    for rows in (3 * S + 1, 3 * S + 2, 3 * S + 3):
        refused = rows == 3 * S + 1
        add(Case(f"rows-tripolar-fwd-f8-{rows}", "TRIPOLAR_POP_WITH_LAND", "f8", (rows, nx), r"k_" if refused else rf"k_ring<double, double, {KIND_FLUX}, {S}, ",
                 ev="reference", tuning=_t(multi_s=S, clenshaw=0), not_kernel=rf"k_ring<double, double, \d, {S}, " if refused else None,
                 reaches=() if refused else ("k_ring",)))
        add(Case(f"rows-tripolar-zip-f8-{rows}", "TRIPOLAR_POP_WITH_LAND", "f8", (rows, nx), r"k_" if refused else rf"k_ringcz<double, {S}, ",
                 options=_t(ringc_smax=S, zip_fold=1), not_kernel=rf"k_ringc[sz]?<double, (\d, )?{S}, " if refused else None,
                 reaches=() if refused else ("k_ringcz",)))
        add(Case(f"rows-tripolar-band-f8-{rows}", "TRIPOLAR_POP_WITH_LAND", "f8", (rows, nx), r"k_" if refused else rf"k_ringcs?<double, (2, )?{S}, ",
                 options=_t(ringc_smax=S, zip_fold=0, ringc_zip=0), not_kernel=rf"k_ringc[sz]?<double, (\d, )?{S}, " if refused else None,
                 reaches=() if refused else ("k_ringc",)))
        add(Case(f"rows-tripolar-reg-f8-{rows}", "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", "f8", (rows, nx),
                 r"k_" if refused else rf"k_ring<double, double, {KIND_MASK}, {S}, ", ev="reference", tuning=_t(multi_s=S, clenshaw=0),
                 not_kernel=rf"k_ring<double, double, \d, {S}, " if refused else None, reaches=() if refused else ("k_ring",)))


# ---- tall and narrow: 8 ghost columns wrap around x more than once ------------------------------------------------------------
def _narrow_family():
    for dt, nxs in (("f8", (2, 4, 6, 8)), ("f4", (4, 8, 12))):
        for grid in T.SCALAR_GRIDS:
            for k, nx in enumerate(nxs):
                rows = (64, 97, 150, 200)[k]
                ev = "backward" if dt == "f4" and k % 2 else "auto"
                if dt == "f8" and nx % 4 and grid in LAND_KINDS:
                    # no backward evaluation where land must be fixed up and nx % 4 != 0 (land_ok): the forward kernels, still blocked
                    want = r"k_(ringc[sz]?|ring|scalar_multi)<double, "
                else:
                    want = r"k_ringc[sz]?<" if (dt == "f8" or ev == "backward") else r"k_(ring|flux_multi2)<"
                add(Case(f"narrow-{grid}-{dt}-{nx}", grid, dt, (rows, nx), want, ev=ev,
                         scheme="scalar_backward" if want.startswith("k_ringc") and dt == "f4" else "forward"))
        vec = 2 if dt == "f8" else 4
        for nx in (vec, 2 * vec):
            add(Case(f"narrow-cgrid-{dt}-{nx}", "VECTOR_C_GRID", dt, (120, nx),
                     r"k_cgrid_stream2c<double" if dt == "f8" else r"k_cgrid_ring<float", nb=3,
                     scheme="forward" if dt == "f8" else "cgrid_backward"))
            add(Case(f"narrow-bgrid-{dt}-{nx}", "VECTOR_B_GRID", dt, (120, nx),
                     r"k_bgrid_stream2c<double, " if dt == "f8" else r"k_bgrid_stream2<float, ", nb=3))


# ---- x windows: nwx = ceil(nx / WI) at WI - VEC, WI, WI + VEC, 2 WI - VEC, 2 WI + VEC --------------------------------------------
def _window_family():
    # (f64: an all-ocean mask -- with land the backward evaluation needs nx % 4 == 0, which WI +- 2 is not; nine levels need >= 64 rows)
    for tag, dt, wi, vec, rows, ev, opts, want in (
            ("f8s8", "f8", WI_F64, 2, 40, "auto", _t(ringc_smax=8, ringc_zip=0, ringc9=0), r"k_ringcs?<double, (2, )?8, "),
            ("f8s9", "f8", WI_F64_9, 2, 72, "auto", _t(ringc_zip=0), r"k_ringc<double, 2, 9, "),
            ("f4", "f4", WI_F32, 4, 40, "backward", _t(ringc_smax=8), r"k_ringcs?<float, (2, )?8, ")):
        for nx in (wi - vec, wi, wi + vec, 2 * wi - vec, 2 * wi + vec):
            add(Case(f"xwin-{tag}-{nx}", "IRREGULAR_WITH_LAND", dt, (rows, nx), want, n_steps=36, ev=ev, options=opts, land=dt == "f4",
                     geom=_t(nwx=math.ceil(nx / wi)), scheme="scalar_backward" if dt == "f4" else "forward"))


# ---- strips and packed runs that do not divide evenly; the early-exit form on both sides of ringc_xe_rows ---------------------------
def _strip_family():
    H = 10
    for r in (1, 2, 3):
        rows = 4 * H + r
        add(Case(f"strip-ringc-last{r}", "IRREGULAR_WITH_LAND", "f8", (rows, 128), r"k_ringcs?<double, (2, )?8, ",
                 tuning=_t(multi_s=8, strip_rows=H), options=_t(ringc_smax=8, ringc_zip=0), geom=_t(H=H, nstrips=5)))
        add(Case(f"strip-ring-last{r}", "REGULAR_WITH_LAND", "f8", (rows, 128), rf"k_ring<double, double, {KIND_MASK}, 8, ",
                 ev="reference", tuning=_t(multi_s=8, strip_rows=H, clenshaw=0), geom=_t(H=H, nstrips=5)))
        add(Case(f"strip-cgrid-last{r}", "VECTOR_C_GRID", "f8", (rows, 128), r"k_cgrid_stream2c<double, 2, 4, ", nb=2,
                 tuning=_t(multi_s=8, strip_rows=H)))
    # packed batches (k_ringcp): the batch is one column of nb * nrows rows per window, cut into runs of q rows; taken where that beats
    # whole strips, i.e. where whole strips need more than one round of 1024 waves.  Short grids, wide enough for that, with q chosen by the
    # launcher's cost model (gcmf_ringc_impl.hpp) NOT dividing nrows: runs cross field boundaries.
    # (host arrays above ~32 MB are cut into chunks of fields before they reach the launcher: these stay below)
    for nb, rows, nx, q in ((2, 65, 29568, 44), (3, 57, 19712, 35), (7, 50, 8512, 27)):
        assert rows % q
        add(Case(f"packed-nb{nb}", "REGULAR", "f8", (rows, nx), rf"k_ringcp<double, {KIND_REG}, 8, ", nb=nb, options=_t(pack_batch=1),
                 geom=_t(H=q), reaches=("k_ringcp",)))
    # ringc_xe_rows = 64: strips of H0 < 64 rows MAY take k_ringcs; at S = 6, H0 = 63 does (76-row early-exit march against 84)
    for H, want in ((63, r"k_ringcs<double, 6, "), (64, r"k_ringc<double, 2, 6, "), (65, r"k_ringc<double, 2, 6, ")):
        add(Case(f"xe-rows-{H}", "IRREGULAR_WITH_LAND", "f8", (3 * H, 64), want, tuning=_t(multi_s=8, strip_rows=H),
                 options=_t(ringc_smax=6, ringc_zip=0), geom=_t(H=H)))


# ---- fallback and general kernels ---------------------------------------------------------------------------------------------
def _fallback_family():
    for grid, want in (("IRREGULAR_WITH_LAND", r"k_flux_multi2<double, double, 8>"), ("REGULAR", r"k_scalar_multi<double, double, 0, 8"),
                       ("REGULAR_WITH_LAND", r"k_scalar_multi<double, double, \d, 8"), ("MOM5T", r"k_flux_multi2<double, double, 8>")):
        add(Case(f"noring-{grid}", grid, "f8", (60, 128), want, ev="reference", tuning=_t(multi_s=8, clenshaw=0), env=_t(GCMF_RING="0")))
    add(Case("noring-f4-flux", "IRREGULAR_WITH_LAND", "f4", (60, 128), r"k_flux_multi2<float, double, 8>", ev="reference",
             options=_t(ring_flux_f32=0)))
    # area-weighted plans where ring_supported refuses: (a) the land-mask kind whose land cannot be kept out of the state (land_ok
    # needs nx % 4 == 0), so every launch of the mask stencil runs the general kernel; (b) the first launch of a filter, which the
    # static-ring kernels take only when the caller fixes isolated cells up afterwards (ring_first) -- n_steps = 8 is that launch alone
    add(Case("area-mask-noring", "REGULAR_WITH_LAND_AREA_WEIGHTED", "f8", (60, 126), rf"k_scalar_multi<double, double, 1, 8, ",
             ev="reference", tuning=_t(multi_s=8, clenshaw=0), not_kernel=r"k_ring<"))
    add(Case("area-reg-first", "REGULAR_AREA_WEIGHTED", "f8", (60, 128), rf"k_scalar_multi<double, double, {KIND_REG}, 8, ",
             n_steps=8, ev="reference", tuning=_t(multi_s=8, clenshaw=0), not_kernel=r"k_ring<"))
    add(Case("step-scalar-f8", "IRREGULAR_WITH_LAND", "f8", (60, 128), r"k_scalar_step<double, double, ", tuning=_t(multi_s=1)))
    add(Case("step-scalar-odd-f4", "MOM5U", "f4", (60, 127), r"k_scalar_step<float, "))
    for dt in ("f8", "f4"):
        ty = "double" if dt == "f8" else "float"
        add(Case(f"tile-cgrid-{dt}", "VECTOR_C_GRID", dt, (60, 128), rf"k_cgrid_step<{ty}, ", nb=2, env=_t(GCMF_CGRID_TILE="1")))
        add(Case(f"tile-bgrid-{dt}", "VECTOR_B_GRID", dt, (60, 128), rf"k_bgrid_step<{ty}, ", nb=2, tuning=_t(multi_s=1),
                 env=_t(GCMF_CGRID_TILE="1")))
        add(Case(f"odd-cgrid-{dt}", "VECTOR_C_GRID", dt, (60, 127), rf"k_cgrid_step<{ty}, "))
        add(Case(f"odd-bgrid-{dt}", "VECTOR_B_GRID", dt, (60, 127), rf"k_bgrid_step<{ty}, "))
        add(Case(f"single-cgrid-{dt}", "VECTOR_C_GRID", dt, (60, 128), rf"k_cgrid_stream<{ty}, ", tuning=_t(multi_s=1)))
        add(Case(f"single-bgrid-{dt}", "VECTOR_B_GRID", dt, (60, 128), rf"k_bgrid_stream<{ty}, ", tuning=_t(multi_s=1)))
    add(Case("nozigzag", "IRREGULAR_WITH_LAND", "f8", (200, 256), r"k_ringc[sz]?<double, ", env=_t(GCMF_ZIGZAG="0")))
    add(Case("single-launch", "IRREGULAR_WITH_LAND", "f8", (64, 128), r"k_ringc_one<", options=_t(single_launch=1)))


# ---- the on-chip (resident) kernel: a small grid, a tall narrow one ------------------------------------------------------------------
def _resident_family():
    # res_supported: a halo of K = 8 (else 4) levels needs nx >= 2K + 16 -- 24 is the narrowest grid on chip, 22 falls back to the strips
    add(Case("resident-small", "IRREGULAR_WITH_LAND", "f8", (96, 160), r"k_resident<", env=_t(GCMF_RESIDENT="1")))
    for grid in ("IRREGULAR_WITH_LAND", "REGULAR_WITH_LAND"):
        add(Case(f"resident-narrow-{grid}-24", grid, "f8", (400, 24), r"k_resident<", n_steps=30, env=_t(GCMF_RESIDENT="1")))
        add(Case(f"resident-narrow-{grid}-22", grid, "f8", (400, 22), r"k_", n_steps=30, not_kernel=r"k_resident<", env=_t(GCMF_RESIDENT="1")))
    add(Case("resident-narrow-f4", "IRREGULAR_WITH_LAND", "f4", (400, 24), r"k_", not_kernel=r"k_resident<", env=_t(GCMF_RESIDENT="1")))


_rows_family()
_narrow_family()
_window_family()
_strip_family()
_fallback_family()
_resident_family()


# ------------------------------------------------------------------------------------------------------------------------------
# running a case
# ------------------------------------------------------------------------------------------------------------------------------
def _coast_inputs(c: Case):
    """Inputs of a case with a coastline: the mask (and kappa / the C-grid's second mask) from gcm_filters_amd.testing, seeded by the
    case's id; strip cuts for `on_the_cuts` from the case's strip_rows."""
    name, _, variant = c.coast.partition(":")
    seed = zlib.crc32(c.id.encode()) % 10007
    if c.grid == "VECTOR_C_GRID":
        if c.metrics == "irregular":
            gv = T.vector_grid_vars_irregular(c.grid, c.shape, coast=name, independent_q=variant == "indq", coast_seed=seed)
        else:
            gv = T.cgrid_coast_vars(name, c.shape, seed, independent_q=variant == "indq")
        fields = [np.stack([T.random_field(c.shape, s + 2 * l) for l in range(c.nb)]) if c.nb else T.random_field(c.shape, s)
                  for s in (42, 43)]
    else:
        gv = T.scalar_grid_vars(c.grid, c.shape)
        cuts = tuple(v for k, v in c.tuning if k == "strip_rows") + tuple(v for k, v in c.geom if k == "H")
        gv["wet_mask"] = T.coastline(name, c.shape, seed, tripolar=c.grid.startswith("TRIPOLAR"), cuts=cuts)
        if variant == "kappa":
            gv["kappa_w"], gv["kappa_s"] = T.kappa_with_zeros(c.shape)
        f = np.stack([T.random_field(c.shape, 100 + l) for l in range(c.nb)]) if c.nb else T.random_field(c.shape, 100)
        fields = [T.treat_land(f, gv["wet_mask"], c.land_values, seed)]
    gv = {k: v.astype(c.dt) for k, v in gv.items()}
    return [x.astype(c.dt) for x in fields], gv


def _inputs(c: Case):
    if c.coast:
        return _coast_inputs(c)
    rng_shape = ((c.nb,) if c.nb else ()) + c.shape
    if c.grid in T.VECTOR_GRIDS:
        gv = T.vector_grid_vars_irregular(c.grid, c.shape) if c.metrics == "irregular" else T.vector_grid_vars(c.grid, c.shape)
        fields = [np.stack([T.random_field(c.shape, s + 2 * l) for l in range(c.nb)]) if c.nb else T.random_field(c.shape, s)
                  for s in (42, 43)]
    else:
        gv = T.scalar_grid_vars(c.grid, c.shape)
        if not c.land:
            gv["wet_mask"] = np.ones(c.shape)
        f = np.stack([T.random_field(c.shape, 100 + l) for l in range(c.nb)]) if c.nb else T.random_field(c.shape, 100)
        if "wet_mask" in gv:
            f = np.where(np.broadcast_to(gv["wet_mask"], rng_shape) == 0, np.nan, f)
        fields = [f]
    gv = {k: v.astype(c.dt) for k, v in gv.items()}
    return [x.astype(c.dt) for x in fields], gv


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = ~np.isnan(want)
    scale = np.abs(want[fin]).max() if fin.any() else 1.0
    return float(np.abs(got[fin] - want[fin]).max() / scale) if fin.any() and scale > 0 else 0.0


def run_case(c: Case, monkeypatch=None):
    """Run one case on cuda:0; returns dict(kernel, geom, results) -- the filter's and the Laplacian's outputs and the oracle's (f64 on the
    same values, and for f32 cases also the oracle's own f32 path)."""
    from gcm_filters_amd import Filter, FilterShape, GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
    from oracle import gcmf_oracle as O

    for k, v in c.env:
        monkeypatch.setenv(k, v)
    clear_plan_cache()
    fields, gv = _inputs(c)
    vec = c.grid in T.VECTOR_GRIDS
    dx = T.grid_dx_min(c.grid, gv) if O.DIMENSIONAL[c.grid] else 1.0
    plan = ALL_KERNELS[GridType[c.grid]](**gv)._plan(_lib.dtype_code(c.dt), c.shape)
    try:
        if c.tuning:
            plan.set_tuning(**dict(c.tuning))
        for k, v in c.options:
            plan.set_option(k, v)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=c.n_steps, filter_shape=FilterShape.GAUSSIAN, grid_type=GridType[c.grid],
                         grid_vars=gv, evaluation=c.ev)
        got = flt.apply_to_vector(*fields) if vec else (flt.apply(fields[0]),)
        geom = plan.last_kernel_geometry()
        kernel = plan.last_kernel()
        lap = ALL_KERNELS[GridType[c.grid]](**gv)(*fields)
        lap = lap if isinstance(lap, tuple) else (lap,)
    finally:
        clear_plan_cache()
    fs = flt.filter_spec
    spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
    f64 = [x.astype("f8") for x in fields]
    gv64 = {k: v.astype("f8") for k, v in gv.items()}
    olap = O.make_laplacian(c.grid, gv64)
    with np.errstate(all="ignore"):
        truth = O.filter_func_vec(spec, c.grid, *f64, gv64) if vec else (O.filter_func(spec, c.grid, f64[0], gv64),)
        ltruth = olap(*f64)
        ltruth = ltruth if isinstance(ltruth, tuple) else (ltruth,)
        ref32 = lref32 = None
        if c.dt == "f4":
            ref32 = O.filter_func_vec(spec, c.grid, *fields, gv) if vec else (O.filter_func(spec, c.grid, fields[0], gv),)
            l32 = O.make_laplacian(c.grid, gv)(*fields)
            lref32 = l32 if isinstance(l32, tuple) else (l32,)
    return dict(kernel=kernel, geom=geom, got=got, truth=truth, ref32=ref32, lap=lap, ltruth=ltruth, lref32=lref32)


def errors(c: Case, r):
    """(error of the filter, error bound, error of the Laplacian, its bound) -- all relative to the oracle's largest value."""
    e = max(_rel(g, w) for g, w in zip(r["got"], r["truth"]))
    el = max(_rel(g, w) for g, w in zip(r["lap"], r["ltruth"]))
    if c.dt == "f8":
        return e, 1e-12, el, 1e-12
    e_ref = max(_rel(g, w) for g, w in zip(r["ref32"], r["truth"]))
    el_ref = max(_rel(g, w) for g, w in zip(r["lref32"], r["ltruth"]))
    bound = {"forward": 1.5 * e_ref + 1e-6, "cgrid_backward": 0.8 * e_ref + 2e-7, "bgrid_backward": 4.0 * e_ref + 2e-7,
             "scalar_backward": 2.5 * e_ref + 2e-6}[c.scheme]
    return e, bound, el, 1.5 * el_ref + 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_dispatch_edge(c, monkeypatch, tmp_path):
    if dict(c.env).get("GCMF_RESIDENT") == "1":
        monkeypatch.setenv("GCMF_RESIDENT_LOCK_DIR", str(tmp_path))
    r = run_case(c, monkeypatch)
    kernel, geom = r["kernel"], r["geom"]
    for g, w in zip(r["got"], r["truth"]):
        assert g.shape == w.shape
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, kernel, "NaN pattern differs")
    for g, w in zip(r["lap"], r["ltruth"]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, "Laplacian NaN pattern differs")
    e, bound, el, lbound = errors(c, r)
    assert e <= bound, (c.id, kernel, e, bound)
    assert el <= lbound, (c.id, "Laplacian", el, lbound)
    if c.dt == "f8" and c.ev == "reference" and c.grid in BIT_EXACT:
        for g, w in zip(r["got"], r["truth"]):
            assert np.array_equal(g, w, equal_nan=True), (c.id, kernel, "not bit-equal to the oracle")
    assert re.search(c.kernel, kernel), (c.id, kernel, geom)
    if c.not_kernel:
        assert not re.search(c.not_kernel, kernel), (c.id, kernel)
    for k, v in c.geom:
        assert geom.get(k) == v, (c.id, kernel, k, geom)


# ------------------------------------------------------------------------------------------------------------------------------
# the on-chip kernel's upper edge: the tallest grid gcmf_resident_supported admits (res_geometry finds no tile geometry above it)
# ------------------------------------------------------------------------------------------------------------------------------
def _check_against_oracle(c: Case, r):
    for g, w in zip(r["got"], r["truth"]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (c.id, r["kernel"], "NaN pattern differs")
    e, bound, el, lbound = errors(c, r)
    assert e <= bound and el <= lbound, (c.id, r["kernel"], e, bound, el, lbound)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["IRREGULAR_WITH_LAND", "REGULAR_WITH_LAND"])
def test_resident_tallest_admitted_grid(grid, monkeypatch, tmp_path):
    """nx = 32: bisect the rows of plans for the largest grid Plan.resident_supported (gcmf_resident_supported) admits for the whole
    polynomial; GCMF_RESIDENT=1 must run it on chip (k_resident) and the next row up on the strips, both equal to the oracle."""
    from gcm_filters_amd import GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache

    monkeypatch.setenv("GCMF_RESIDENT_LOCK_DIR", str(tmp_path))
    nx, n_steps = 32, 24

    def admitted(rows):
        gv = {k: np.ones((rows, nx)) for k in T.FIXTURE_ARG_ORDER[grid]}
        gv["wet_mask"] = T.land_mask((rows, nx))
        try:
            return ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, (rows, nx)).resident_supported(0, rows, n_steps)
        finally:
            clear_plan_cache()

    lo, hi = 64, 1 << 17        # admitted, refused (a few hundred rows per tile at most, 256 workgroups)
    assert admitted(lo) and not admitted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if admitted(mid) else (lo, mid)
    print(f"\n{grid} nx {nx}: on chip up to {lo} rows, {hi} refused")
    for rows, on_chip in ((lo, True), (hi, False)):
        c = Case(f"resident-tallest-{grid}-{rows}", grid, "f8", (rows, nx), r"k_resident<" if on_chip else r"k_", n_steps=n_steps,
                 env=_t(GCMF_RESIDENT="1"), not_kernel=None if on_chip else r"k_resident<")
        r = run_case(c, monkeypatch)
        assert re.search(c.kernel, r["kernel"]) and not (c.not_kernel and re.search(c.not_kernel, r["kernel"])), (rows, r["kernel"])
        _check_against_oracle(c, r)


# ------------------------------------------------------------------------------------------------------------------------------
# the 32-bit byte-offset guards of k_cgrid_ring (rows * nx * 4 < 2^32) and k_cgrid_ringf (rows * nx * 8 < 2^32)
# ------------------------------------------------------------------------------------------------------------------------------
OFFSET_CASES = [
    # (id, bytes per cell the guard counts, evaluation, n_steps, kernel below the bound, fallback above it, f32 error policy)
    ("ringf", 8, "reference", 10, r"k_cgrid_ringf<float, 5, ", r"k_cgrid_stream2<float, double, ", "forward"),
    ("ring", 4, "auto", 12, r"k_cgrid_ring<float, 6, ", r"k_cgrid_stream2c<float, ", "cgrid_backward"),
]


def _cgrid_on_device(rows, nx, nb, seed):
    """VECTOR_C_GRID f32 grid variables (testing.vector_grid_vars' spherical recipe, one tensor per distinct plane) and two batched
    random fields, built on cuda:0."""
    import torch
    dev = "cuda"
    lat0, lat1 = -70.0, 70.0
    lat_u = torch.linspace(lat0 + 0.5 * (lat1 - lat0) / rows, lat1 - 0.5 * (lat1 - lat0) / rows, rows, dtype=torch.float64, device=dev)
    lat_v = torch.linspace(lat0 + (lat1 - lat0) / rows, lat1, rows, dtype=torch.float64, device=dev)
    dxu = (T.EARTH_RADIUS * torch.cos(lat_u / 360 * 2 * np.pi)).float()
    dxv = (T.EARTH_RADIUS * torch.cos(lat_v / 360 * 2 * np.pi)).float()
    dy_val = float(dxu.max())
    plane = lambda col: col[:, None].expand(rows, nx).contiguous()
    dx_u, dx_v = plane(dxu), plane(dxv)
    del dxu, dxv, lat_u, lat_v
    dy = torch.full((rows, nx), dy_val, dtype=torch.float32, device=dev)
    mask = torch.ones((rows, nx), dtype=torch.float32, device=dev)
    mask[: rows // 2, : nx // 2] = 0
    ones = torch.ones((rows, nx), dtype=torch.float32, device=dev)
    gv = {"wet_mask_t": mask, "wet_mask_q": mask, "dxT": dx_u, "dyT": dy, "dxCu": dx_u, "dyCu": dy, "dxCv": dx_v, "dyCv": dy,
          "dxBu": dx_v, "dyBu": dy, "area_u": dx_u * dy, "area_v": dx_v * dy, "kappa_iso": ones, "kappa_aniso": ones}
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.rand((nb, rows, nx), generator=g, dtype=torch.float32, device=dev)
    v = torch.rand((nb, rows, nx), generator=g, dtype=torch.float32, device=dev)
    dx_min = min(float(dx_u.min()), float(dx_v.min()), dy_val)
    return gv, u, v, dx_min


def _seam_rows(t, m):
    """Rows [ny - m, ny) followed by rows [0, m) of the last two axes' planes: a band across the periodic y seam, to host."""
    import torch
    return torch.cat([t[..., -m:, :], t[..., :m, :]], dim=-2).cpu().numpy()


def _run_cgrid_offset(rows, nx, ev, n_steps, m):
    """Filter a device-built (rows, nx) C-grid f32 batch of 2 levels; returns (kernel, the seam band of the inputs / grid / result)."""
    import torch
    from gcm_filters_amd import Filter, GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS

    gv, u, v, dx = _cgrid_on_device(rows, nx, 2, 7)
    plan = ALL_KERNELS[GridType.VECTOR_C_GRID](**gv)._plan(_lib.F32, (rows, nx))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=n_steps, grid_type=GridType.VECTOR_C_GRID, grid_vars=gv, evaluation=ev)
    gu, gw = flt.apply_to_vector(u, v)
    torch.cuda.synchronize()
    kernel = plan.last_kernel()
    band = dict(u=_seam_rows(u, m), v=_seam_rows(v, m), got=(_seam_rows(gu, m), _seam_rows(gw, m)),
                gv={k: _seam_rows(t, m) for k, t in gv.items()}, spec=flt.filter_spec)
    return kernel, band


def _free_device():
    import gc
    import torch
    from gcm_filters_amd.kernels import clear_plan_cache
    gc.collect()
    clear_plan_cache()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("oc", OFFSET_CASES, ids=[o[0] for o in OFFSET_CASES])
def test_cgrid_32bit_offset_guard(oc, side):
    """nx = 4 (nx % 4 == 0 is the only width condition), so the largest rows * nx below a guard's bound is bound - 4 cells and the next
    admissible height reaches it: `below` must run the guarded kernel, `above` the 64-bit fallback.  Only the rows beside the periodic y
    seam -- row ny - 1 holds a level's highest offsets -- are copied back and compared with the oracle run on the band of the top m and
    bottom m rows (every column); the band's cut edges are wrong after n steps (plus the stencil's reach in the coefficient planes), so
    only rows more than n_steps + 2 from them are compared.  Memory: measured per cell on a 2^22-cell copy of the same setup and scaled
    (about 240 bytes per cell: ~128 GB for the k_cgrid_ringf pair at 2^29 cells, ~247 GB for the k_cgrid_ring pair at 2^30 cells, which
    one MI355X does not hold 1.5 x of).  Skipped when less than 1.5 x the need is free; everything is freed before the test returns."""
    import torch
    from oracle import gcmf_oracle as O

    name, bpc, ev, n_steps, below, above, scheme = oc
    nx = 4
    cells = (1 << 32) // bpc                     # the guard: rows * nx * bpc < 2^32, i.e. rows * nx < cells
    rows = cells // nx - 1 if side == "below" else cells // nx
    m = n_steps + 8
    _free_device()
    probe_rows = (1 << 22) // nx
    free0 = torch.cuda.mem_get_info()[0]
    try:
        kernel, _ = _run_cgrid_offset(probe_rows, nx, ev, n_steps, m)
        assert re.search(below, kernel), kernel  # (the probe is far inside the guard)
        per_cell = (free0 - torch.cuda.mem_get_info()[0]) / (probe_rows * nx)
    finally:
        _free_device()
    need = per_cell * rows * nx
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * need:
        pytest.skip(f"{name} {side}: needs ~{need / 1e9:.0f} GB on the device, {free / 1e9:.0f} GB free (< 1.5 x)")
    try:
        kernel, band = _run_cgrid_offset(rows, nx, ev, n_steps, m)
        used = free - torch.cuda.mem_get_info()[0]
    finally:
        _free_device()
    print(f"\n{name} {side}: rows {rows} x nx {nx} = {rows * nx} cells, {kernel}, {used / 1e9:.1f} GB used")
    if side == "below":
        assert re.search(below, kernel), kernel
    else:
        assert not re.search(r"k_cgrid_ring", kernel) and re.search(above, kernel), kernel
    fs = band["spec"]
    spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
    gv32 = band["gv"]
    gv64 = {k: x.astype("f8") for k, x in gv32.items()}
    with np.errstate(all="ignore"):
        truth = O.filter_func_vec(spec, "VECTOR_C_GRID", band["u"].astype("f8"), band["v"].astype("f8"), gv64)
        ref32 = O.filter_func_vec(spec, "VECTOR_C_GRID", band["u"], band["v"], gv32)
    keep = slice(n_steps + 3, 2 * m - (n_steps + 3))     # rows m - 5 .. m + 4 of the band: ny - 5 .. ny - 1 and 0 .. 4 of the grid
    got = [np.asarray(g, np.float64)[..., keep, :] for g in band["got"]]
    truth = [t[..., keep, :] for t in truth]
    ref32 = [t[..., keep, :] for t in ref32]
    assert all(np.isfinite(g).all() for g in got)
    e = max(_rel(g, w) for g, w in zip(got, truth))
    e_ref = max(_rel(g, w) for g, w in zip(ref32, truth))
    bound = {"forward": 1.5 * e_ref + 1e-6, "cgrid_backward": 0.8 * e_ref + 2e-7}[scheme]
    assert e <= bound, (name, side, kernel, e, e_ref)
