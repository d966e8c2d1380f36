"""The device-pointer contract of include/gcmf.h, on planes the CALLER owns: views into a larger buffer instead of the plan's own staged
planes (host-pointer calls) or tight, allocator-padded tensors (the rest of the device-side suite).

A. Every case of the dispatch-edge table (tests/test_gpu_dispatch_edges.py: CASES, _inputs, the resident-lock handling) runs
   ``Plan.apply`` / ``Plan.laplacian`` with ``device_ptrs=True`` on planes inside a POISONED ARENA -- two flat device buffers, one for the
   inputs and one for the outputs, laid out ``guard | plane | guard [| plane | guard]`` (a guard is at least 16 rows of the plane plus
   4 KiB; the batch is contiguous inside a plane) -- in three layouts:

     aligned       every plane on a 16-byte boundary; poison = a NaN with a payload of its own, compared as integers
     in-shifted    the input planes one element off (8 bytes f64, 4 bytes f32); poison = 1e300 / 3e38, which nan_to_num does not hide
     out-shifted   the output planes one element off (8 bytes for f64 results, 4 for f32 ones); poison = the NaN

   and, for the four grids of test_gpu_parity.py::test_out_f32_option, ``out_f32=True`` with the 4-byte shift.  The baseline is the
   same call on tight, separately allocated tensors; its kernel must be the one the table names.  Every layout must give the
   baseline's result (np.array_equal, equal_nan), leave no poison inside the output planes, leave every byte of both buffers outside the
   output planes as it was (the input planes included), and run the table's kernel -- or, off the 16-byte boundary, the fallback its
   launcher documents (FALLBACKS, one row per launcher predicate that looks at the CALLER's planes).  No family needed a tolerance.

   Two predicates the launchers also have, ``c2al16`` (gcmf_cgrid_stream2.hip) and ``b2al16`` (gcmf_bgrid_stream2.hip), look at the plan's
   own coefficient planes only, which the library allocates: no caller can put them on their unaligned side, so they have no row.
   The k_ring* / k_ringc* families, k_scalar_multi, k_flux_multi2, k_[cb]grid_stream2[c], k_fold_band, k_land_fix and k_resident have no
   alignment predicate: they take element-aligned planes as they are (plain vector loads, which the hardware serves at element alignment).

   Which launch of a schedule sees the caller's planes: the first reads ``in`` (the backward evaluation: every launch does), the last
   writes ``out``; ``last_kernel()`` names the LAST of the deepest launches.  So a fallback shows in the name only where that launch
   touches the shifted plane -- the single-step schedules and the Laplacian when ``out`` is shifted, k_cgrid_ring when ``in`` is -- and a
   predicate's witness is chosen accordingly (``ringf-two-launches`` below is a case of this module for that reason: in the table's
   k_cgrid_ringf cases the last launch is a shallower one).

B. The calls the table does not reach -- GCMF_MASK_FROM_NAN, GCMF_FACES_FROM_NAN, gcmf_apply_bank (also on the tripolar POP grid, the
   seam band beside and after the strips), gcmf_apply_bank_gaps and a stacked plan -- in the same arena with the same assertions.
   ``gap_load4`` (k_pre_isolated's gap form, gcmf_precompute.hip) decides per entry from the address of ``field``: (field & 15) == 0
   takes the 16-byte loads, anything else the element loads.  nx % 4 == 0 and f64, so in the layouts ``aligned`` and ``out-shifted`` every
   entry's plane starts on a 16-byte boundary (the aligned arm) and in ``in-shifted`` every one starts 8 bytes off it (the unaligned
   arm).  The arm cannot be seen from outside: the test asserts the addresses and that all layouts give the same bits.

C. ``out`` overlapping ``in`` (or another ``out`` plane) as a BYTE RANGE is refused with GCMF_ERR_INVALID_ARG before anything is written.

D. With device pointers the work is ordered on the caller's stream: a delay, an asynchronous upload of the input, the call, a copy of
   the result, and overwrites of input and output are queued back to back on a fresh stream with ONE synchronisation at the end; the
   copy must hold the bits of the same call made on the default stream with synchronisation around it.
"""
from __future__ import annotations

import re
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest

from gcm_filters_amd import testing as T
from test_gpu_dispatch_edges import CASES, Case, _inputs, _t

pytestmark = pytest.mark.gpu

LAYOUTS = ("aligned", "in-shifted", "out-shifted")
NAN_BITS = {8: 0x7FF8DEAD0BADBEEF, 4: 0x7FC5A5A5}                         # quiet NaNs with payloads no arithmetic produces
FINITE_BITS = {8: int(np.float64(1e300).view(np.int64)), 4: int(np.float32(3e38).view(np.int32))}
OUT_F32_GRIDS = ("IRREGULAR_WITH_LAND", "REGULAR_WITH_LAND", "VECTOR_C_GRID", "VECTOR_B_GRID")   # test_gpu_parity.py::test_out_f32_option


# ------------------------------------------------------------------------------------------------------------------------------
# the arena
# ------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """One flat device buffer ``guard | plane 0 | guard [| plane 1 | guard ...]`` of one dtype, every element poisoned.  shift: elements
    the planes start off a 16-byte boundary.  A plane is a contiguous (nb, ny, nx) view."""

    def __init__(self, shape3, nplanes, np_dt, shift, poison_bits):
        import torch
        np_dt = np.dtype(np_dt)
        self.esz = np_dt.itemsize
        self.tdt = {8: torch.float64, 4: torch.float32}[self.esz]
        self.idt = {8: torch.int64, 4: torch.int32}[self.esz]
        nb, ny, nx = shape3
        self.shape3, self.n, per16 = tuple(shape3), nb * ny * nx, 16 // self.esz
        guard = -(-(16 * nx * self.esz + 4096) // 16) * per16           # elements: >= 16 rows + 4 KiB, a multiple of 16 bytes
        slot = -(-self.n // per16) * per16                              # a plane's slot, rounded up to 16 bytes
        self.buf = torch.empty(guard + nplanes * (slot + guard) + per16, dtype=self.tdt, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.bits = self.buf.view(self.idt)
        self.poison = poison_bits[self.esz]
        self.bits.fill_(self.poison)
        self.starts = [shift + guard + k * (slot + guard) for k in range(nplanes)]
        self.planes = [self.buf[s:s + self.n].view(self.shape3) for s in self.starts]
        for p in self.planes:
            assert p.is_contiguous() and p.data_ptr() % 16 == (shift * self.esz) % 16
        self.saved = None

    def load(self, fields):
        import torch
        for p, f in zip(self.planes, fields):
            p.copy_(torch.from_numpy(np.ascontiguousarray(f).reshape(self.shape3)))

    def snapshot(self):
        self.saved = self.bits.clone()

    def ptrs(self):
        return [p.data_ptr() for p in self.planes]

    def _where(self, idx):
        """Element `idx` of the buffer relative to the nearest plane, for a message."""
        for k, s in enumerate(self.starts):
            if s <= idx < s + self.n:
                b, r = divmod(idx - s, self.shape3[1] * self.shape3[2])
                return f"plane {k} entry {b} row {r // self.shape3[2]} col {r % self.shape3[2]}"
        k = min(range(len(self.starts)), key=lambda q: min(abs(idx - self.starts[q]), abs(idx - self.starts[q] - self.n)))
        s = self.starts[k]
        return f"{s - idx} elements BEFORE plane {k}" if idx < s else f"{idx - s - self.n} elements AFTER the end of plane {k} (nx = {self.shape3[2]})"

    def changed(self, outside_only):
        """None, or where the first element that differs from the snapshot lies (outside_only: the planes themselves may change)."""
        import torch
        diff = self.bits != self.saved
        if outside_only:
            for s in self.starts:
                diff[s:s + self.n] = False
        if not bool(diff.any()):
            return None
        idx = int(torch.nonzero(diff)[0])
        return f"{int(diff.sum())} elements changed, the first {self._where(idx)}"

    def poison_left(self):
        return sum(int((self.bits[s:s + self.n] == self.poison).sum()) for s in self.starts)


def run_in_arena(call, fields, layout, out_shape3, out_dt, n_out, what="", after=None):
    """call(in_ptrs, out_ptrs) with `fields` (host arrays, one per input plane) and `n_out` output planes laid out as `layout` says;
    asserts the arena's invariants and returns the output planes as host arrays.  after(input arena, output arena): run behind the
    call (test_the_arena_notices_strays plays a faulty kernel with it)."""
    import torch
    assert layout in LAYOUTS
    poison = FINITE_BITS if layout == "in-shifted" else NAN_BITS
    shape3 = (1,) * (3 - fields[0].ndim) + tuple(fields[0].shape)
    ain = Arena(shape3, len(fields), fields[0].dtype, 1 if layout == "in-shifted" else 0, poison)
    aout = Arena(out_shape3, n_out, out_dt, 1 if layout == "out-shifted" else 0, poison)
    ain.load(fields)
    ain.snapshot()
    aout.snapshot()
    torch.cuda.synchronize()
    call(ain.ptrs(), aout.ptrs())
    if after is not None:
        after(ain, aout)
    torch.cuda.synchronize()
    bad = ain.changed(outside_only=False)
    assert bad is None, (what, layout, "the input buffer was written", bad)
    bad = aout.changed(outside_only=True)
    assert bad is None, (what, layout, "the output buffer was written outside the planes", bad)
    left = aout.poison_left()
    assert left == 0, (what, layout, f"{left} elements of the output planes still hold the poison")
    return [p.cpu().numpy() for p in aout.planes], ain.ptrs(), aout.ptrs()


def tight(call, fields, out_shape3, out_dt, n_out):
    """The baseline: the same call on tight, separately allocated tensors."""
    import torch
    shape3 = (1,) * (3 - fields[0].ndim) + tuple(fields[0].shape)
    tin = [torch.from_numpy(np.ascontiguousarray(f).reshape(shape3)).cuda() for f in fields]
    tdt = torch.float64 if np.dtype(out_dt).itemsize == 8 else torch.float32
    tout = [torch.full(out_shape3, float("nan"), dtype=tdt, device="cuda") for _ in range(n_out)]
    call([t.data_ptr() for t in tin], [t.data_ptr() for t in tout])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tout]


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w, equal_nan=True):
            ne = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            first = tuple(int(i) for i in np.argwhere(ne)[0])
            raise AssertionError((what, f"component {k}: {int(ne.sum())} cells differ from the baseline, the first at {first}: "
                                        f"{g[first]!r} against {w[first]!r}"))


def test_the_arena_notices_strays():
    """The harness itself, with a faulty kernel played behind a correct call (one Laplacian of a small REGULAR plan): a store one vector
    past the last row, one row before the first, a store into the input or its guard, a cell left unwritten, and a result that a value
    from outside the plane went into -- each must fail the assertion that is there for it, in the layout whose poison it needs."""
    from gcm_filters_amd import GridType, _lib
    shape = ny, nx = (12, 20)
    plan = _lib.Plan(GridType.REGULAR.value, _lib.F64, ny, nx, [])
    try:
        f = T.random_field(shape, 7)
        call = lambda ins, outs: plan.laplacian(ins, outs, 1, device_ptrs=True)
        want = tight(call, [f], (1,) + shape, "f8", 1)

        def go(layout, after=None):
            got, _, _ = run_in_arena(call, [f], layout, (1,) + shape, "f8", 1, "stray", after)
            same(got, want, ("stray", layout))

        def store(which, offset, value=1.0):          # offset: elements from the start of plane 0
            def after(ain, aout):
                a = ain if which == "in" else aout
                a.buf[a.starts[0] + offset] = value
            return after

        def reads_the_guard(ain, aout):
            aout.planes[0][0, 0, 0] += 1e-300 * ain.buf[ain.starts[0] - 1]

        def skips_a_cell(ain, aout):
            aout.bits[aout.starts[0] + 5 * nx + 3] = aout.poison

        for layout in LAYOUTS:
            go(layout)
            with pytest.raises(AssertionError, match="outside the planes.*AFTER the end of plane 0"):
                go(layout, store("out", ny * nx + 1))
            with pytest.raises(AssertionError, match="outside the planes.*BEFORE plane 0"):
                go(layout, store("out", -nx))
            with pytest.raises(AssertionError, match="input buffer was written.*plane 0 entry 0 row 2 col 1"):
                go(layout, store("in", 2 * nx + 1))
            with pytest.raises(AssertionError, match="input buffer was written.*BEFORE plane 0"):
                go(layout, store("in", -1))
            with pytest.raises(AssertionError, match="still hold the poison"):
                go(layout, skips_a_cell)
            # (the finite poison: 1e300 * 1e-300 = 1 is added; the NaN poison: the cell turns NaN, with the poison's payload or without)
            seen = "differ from the baseline, the first at \\(0, 0, 0\\)"
            with pytest.raises(AssertionError, match=seen if layout == "in-shifted" else seen + "|still hold the poison"):
                go(layout, reads_the_guard)
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the fallback table: one row per launcher predicate that looks at the caller's planes
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fallback:
    predicate: str            # the predicate, and the file it lives in
    aligned: str              # regex: the kernel this launcher runs on 16-byte aligned planes
    unaligned: Optional[str]  # regex: what it runs instead (None: cannot be seen from outside)
    witness: Tuple[str, str]  # (case id, layout) that shows the unaligned side in last_kernel()


FALLBACKS = (
    Fallback("launch_kv (gcmf_scalar.hip)", r"k_scalar_step<\w+, \w+, \d, [24]>", r"k_scalar_step<\w+, \w+, \d, 1>", ("step-scalar-f8", "out-shifted")),
    Fallback("al16 / cgrid_stream_supported (gcmf_cgrid_stream.hip)", r"k_cgrid_stream<", r"k_cgrid_step<", ("single-cgrid-f8", "out-shifted")),
    Fallback("bal16 / bgrid_stream_supported (gcmf_bgrid_stream.hip)", r"k_bgrid_stream<", r"k_bgrid_step<", ("single-bgrid-f8", "out-shifted")),
    Fallback("crf_al16 / cgrid_ringf_supported (gcmf_cgrid_ringf.hip)", r"k_cgrid_ringf<float, ", r"k_cgrid_stream2<float, double, ",
             ("ringf-two-launches", "out-shifted")),
    # (sched_backward_vec also asks for at most five levels per launch when a plane of the call is unaligned: the launches that touch
    # neither `in` nor `out`... every backward launch reads `in`; with only `out` shifted the first launches stay on k_cgrid_ring, five deep)
    Fallback("cgrid_ring_args_aligned (gcmf_cgrid_ring.hip)", r"k_cgrid_ring<float, ", r"k_cgrid_stream2c<float, |k_cgrid_ring<float, [2-5], ",
             ("rows-k_cgrid_ring-f4-auto-8", "in-shifted")),
)
GAP_LOAD4 = "gap_load4's al16 == false arm (gcmf_precompute.hip, k_pre_isolated<.., GAPS>)"
HITS = {}          # predicate -> (case id, layout, kernel) seen on its unaligned side

# a case of this module's own: k_cgrid_ringf where the LAST of the deepest launches writes `out` (10 steps = 5 + 5)
EXTRA_CASES = [Case("ringf-two-launches", "VECTOR_C_GRID", "f4", (20, 64), r"k_cgrid_ringf<float, 5, ", nb=4, n_steps=10, ev="reference")]
ALL_CASES = list(CASES) + EXTRA_CASES
BY_ID = {c.id: c for c in ALL_CASES}

# Where the device path legitimately runs another kernel than the host path the table was written for: case id -> (regex, why).
DEVICE_KERNEL = {}


def allowed_kernels(baseline):
    """Regexes a shifted layout may run instead of `baseline` (the kernel the tight tensors ran)."""
    return [(f, f.unaligned) for f in FALLBACKS if f.unaligned and re.search(f.aligned, baseline)]


def note_kernels(c, layout, baseline, got):
    """The kernel of a layout against the baseline's: the same, or (off the boundary) the launcher's documented fallback."""
    if got == baseline:
        return
    assert layout != "aligned", (c.id, layout, got, "instead of", baseline)
    for f, rx in allowed_kernels(baseline):
        if re.search(rx, got):
            if not re.search(rx, baseline):
                HITS.setdefault(f.predicate, (c.id, layout, got))
            return
    raise AssertionError((c.id, layout, got, "is neither the baseline's kernel", baseline, "nor a documented fallback of its launcher"))


# ------------------------------------------------------------------------------------------------------------------------------
# A. the dispatch-edge table
# ------------------------------------------------------------------------------------------------------------------------------
class TableCase:
    """The plan of a dispatch-edge case built as test_gpu_dispatch_edges.run_case builds it (tuning, options, env), and its calls."""

    def __init__(self, c: Case, monkeypatch, tmp_path):
        from gcm_filters_amd import Filter, FilterShape, GridType, _lib
        from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
        from oracle import gcmf_oracle as O
        import torch

        if dict(c.env).get("GCMF_RESIDENT") == "1":
            monkeypatch.setenv("GCMF_RESIDENT_LOCK_DIR", str(tmp_path))
        for k, v in c.env:
            monkeypatch.setenv(k, v)
        clear_plan_cache()
        self.c = c
        fields, gv = _inputs(c)
        self.vec = c.grid in T.VECTOR_GRIDS
        self.nb = max(c.nb, 1)
        self.shape3 = (self.nb,) + tuple(c.shape)
        self.fields = [np.ascontiguousarray(f).reshape(self.shape3) for f in fields]
        dx = T.grid_dx_min(c.grid, gv) if O.DIMENSIONAL[c.grid] else 1.0
        lap = ALL_KERNELS[GridType[c.grid]](**gv)
        self.plan = lap._plan(_lib.dtype_code(c.dt), c.shape)
        if c.tuning:
            self.plan.set_tuning(**dict(c.tuning))
        for k, v in c.options:
            self.plan.set_option(k, v)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=c.n_steps, filter_shape=FilterShape.GAUSSIAN, grid_type=GridType[c.grid],
                         grid_vars=gv, evaluation=c.ev)
        spec = flt.filter_spec
        self.p = np.asarray(spec.p, dtype=np.float64)
        self.coef = 2 / spec.s_max if lap.is_dimensional else 2 / (spec.s_max * spec.dx_min_sq)   # (as kernels.py: Laplacian._call)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ncomp = len(self.fields)

    def apply(self, out_f32=False):
        c = self.c
        return lambda ins, outs: self.plan.apply(self.p, self.coef, ins, outs, self.nb, device_ptrs=True, stream=self.stream, out_f32=out_f32,
                                                 forward=c.ev == "reference", backward_f32=c.ev == "backward")

    def laplacian(self):
        return lambda ins, outs: self.plan.laplacian(ins, outs, self.nb, device_ptrs=True, stream=self.stream)

    def close(self):
        from gcm_filters_amd.kernels import clear_plan_cache
        clear_plan_cache()


def run_table_case(c: Case, layout, monkeypatch, tmp_path, out_f32=False):
    tc = TableCase(c, monkeypatch, tmp_path)
    try:
        plan = tc.plan
        out_dt = "f4" if out_f32 else "f8"
        plan.last_kernel()
        want = tight(tc.apply(out_f32), tc.fields, tc.shape3, out_dt, tc.ncomp)
        k0 = plan.last_kernel()
        lwant = tight(tc.laplacian(), tc.fields, tc.shape3, c.dt, tc.ncomp)
        l0 = plan.last_kernel()
        rx = DEVICE_KERNEL.get(c.id, (c.kernel,))[0]
        assert re.search(rx, k0), (c.id, "baseline", k0, plan.last_kernel_geometry())
        if c.not_kernel:
            assert not re.search(c.not_kernel, k0), (c.id, "baseline", k0)
        got, iptrs, optrs = run_in_arena(tc.apply(out_f32), tc.fields, layout, tc.shape3, out_dt, tc.ncomp, (c.id, "filter"))
        k1 = plan.last_kernel()
        lgot, _, loptrs = run_in_arena(tc.laplacian(), tc.fields, layout, tc.shape3, c.dt, tc.ncomp, (c.id, "Laplacian"))
        l1 = plan.last_kernel()
        esz_in, esz_out = np.dtype(c.dt).itemsize, np.dtype(out_dt).itemsize
        assert all(p % 16 == (esz_in if layout == "in-shifted" else 0) for p in iptrs)
        assert all(p % 16 == (esz_out if layout == "out-shifted" else 0) for p in optrs)
        assert all(p % 16 == (esz_in if layout == "out-shifted" else 0) for p in loptrs)
        same(got, want, (c.id, layout, "filter", k1))
        same(lgot, lwant, (c.id, layout, "Laplacian", l1))
        note_kernels(c, layout, k0, k1)
        note_kernels(c, layout, l0, l1)
        return k0, k1, l0, l1
    finally:
        tc.close()


@pytest.mark.parametrize("c", ALL_CASES, ids=[c.id for c in ALL_CASES])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_caller_planes(layout, c, monkeypatch, tmp_path):
    run_table_case(c, layout, monkeypatch, tmp_path)


@pytest.mark.parametrize("grid", OUT_F32_GRIDS)
def test_caller_planes_out_f32(grid, monkeypatch, tmp_path):
    """GCMF_OUT_F32: the f32 result planes 4 bytes off the 16-byte boundary (the grids and the shape of test_out_f32_option)."""
    vec = grid in T.VECTOR_GRIDS
    c = Case(f"out-f32-{grid}", grid, "f4", (64, 256), r"k_", nb=2 if vec else 0)
    run_table_case(c, "out-shifted", monkeypatch, tmp_path, out_f32=True)


# ------------------------------------------------------------------------------------------------------------------------------
# B. the calls the table does not reach
# ------------------------------------------------------------------------------------------------------------------------------
SHAPE_B, NSTEPS_B, NFIELD_B = (96, 160), 24, 3


def _scalar_plan(kind, shape=SHAPE_B, scales=(4.0,), n_steps=NSTEPS_B):
    """(plan, [p per scale], c, grid variables) of a float64 scalar grid; the plan is the caller's to close."""
    from gcm_filters_amd import Filter, GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, plan_cache_mode
    from oracle import gcmf_oracle as O
    gv = {k: v.astype("f8") for k, v in T.scalar_grid_vars(kind, shape).items()}
    cls = ALL_KERNELS[GridType[kind]]
    dx = T.grid_dx_min(kind, gv) if O.DIMENSIONAL[kind] else 1.0
    ps = []
    with warnings.catch_warnings(), plan_cache_mode("off"):
        warnings.simplefilter("ignore")
        for s in scales:
            spec = Filter(filter_scale=s * dx, dx_min=dx, n_steps=n_steps, grid_type=GridType[kind], grid_vars=gv).filter_spec
            ps.append(np.asarray(spec.p, dtype=np.float64))
    coef = 2 / spec.s_max if cls.is_dimensional else 2 / (spec.s_max * spec.dx_min_sq)
    planes = [np.ascontiguousarray(gv[k], dtype="f8") for k in cls.required_grid_args()]
    plan = _lib.Plan(GridType[kind].value, _lib.F64, shape[0], shape[1], planes)
    return plan, ps, coef, gv


def _gappy(seed, nfield=NFIELD_B, shape=SHAPE_B):
    from test_gpu_nan_mask import gappy_stack
    return gappy_stack(shape, nfield, seed=seed)


def _three_layouts(call, fields, out_shape3, what, n_out=1):
    """Baseline on tight tensors, then the three layouts: same bits, the arena's invariants; returns the input pointers per layout."""
    want = tight(call, fields, out_shape3, "f8", n_out)
    assert all(np.isfinite(w).any() for w in want)
    ptrs = {}
    for layout in LAYOUTS:
        got, iptrs, optrs = run_in_arena(call, fields, layout, out_shape3, "f8", n_out, what)
        same(got, want, (what, layout))
        ptrs[layout] = (iptrs, optrs)
    return want, ptrs


def test_mask_from_nan_on_caller_planes():
    import torch
    plan, (p,), coef, _ = _scalar_plan("REGULAR_WITH_LAND")
    stream = torch.cuda.current_stream().cuda_stream
    try:
        f = _gappy(71)
        call = lambda ins, outs: plan.apply(p, coef, ins, outs, NFIELD_B, device_ptrs=True, stream=stream, mask_from_nan=True)
        want, _ = _three_layouts(call, [f], f.shape, "mask_from_nan")
        assert np.array_equal(np.isnan(want[0]), np.isnan(f))
    finally:
        plan.close()


@pytest.mark.parametrize("kind", ["IRREGULAR_WITH_LAND", "MOM5U"])
def test_faces_from_nan_on_caller_planes(kind):
    """The fold's loads of the caller's field (gap_load4): 16-byte loads in `aligned` and `out-shifted`, where every entry's plane starts on a
    16-byte boundary, element loads in `in-shifted`, where every one starts 8 bytes off -- the address of `field` decides, per entry,
    and ny * nx * 8 is a multiple of 16 here.  Same bits either way."""
    import torch
    plan, (p,), coef, _ = _scalar_plan(kind)
    stream = torch.cuda.current_stream().cuda_stream
    ny, nx = SHAPE_B
    try:
        f = _gappy(72 + (kind == "MOM5U"))
        call = lambda ins, outs: plan.apply(p, coef, ins, outs, NFIELD_B, device_ptrs=True, stream=stream, faces_from_nan=True)
        want, ptrs = _three_layouts(call, [f], f.shape, ("faces_from_nan", kind))
        assert np.array_equal(np.isnan(want[0]), np.isnan(f))
        assert nx % 4 == 0 and (ny * nx * 8) % 16 == 0
        for layout in LAYOUTS:
            entry_ptrs = [ptrs[layout][0][0] + b * ny * nx * 8 for b in range(NFIELD_B)]
            assert all(q % 16 == (8 if layout == "in-shifted" else 0) for q in entry_ptrs), (layout, entry_ptrs)
        HITS.setdefault(GAP_LOAD4, (f"faces_from_nan-{kind}", "in-shifted", "k_pre_isolated"))
    finally:
        plan.close()


@pytest.mark.parametrize("kind, options", [("IRREGULAR_WITH_LAND", ()), ("TRIPOLAR_POP_WITH_LAND", _t(band_seq_cells=0)),
                                           ("TRIPOLAR_POP_WITH_LAND", _t(band_seq_cells=3000000))],
                         ids=["IRREGULAR_WITH_LAND", "TRIPOLAR_POP-band-beside", "TRIPOLAR_POP-band-after"])
def test_apply_bank_on_caller_planes(kind, options):
    """gcmf_apply_bank, three polynomials on three fields: `in` shifted, `out` shifted; on the tripolar grid k_fold_band's per-entry form
    beside the strips (on the plan's side stream) and after them."""
    import torch
    plan, ps, coef, gv = _scalar_plan(kind, scales=(2.0, 3.0, 4.5))
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for k, v in options:
            plan.set_option(k, v)
        P = np.stack(ps)
        f = np.stack([T.random_field(SHAPE_B, 300 + i) for i in range(NFIELD_B)])
        f = np.where(gv["wet_mask"] == 0, np.nan, f)
        call = lambda ins, outs: plan.apply_bank(P, coef, ins[0], outs[0], NFIELD_B, stream=stream)
        want, _ = _three_layouts(call, [f], (len(ps) * NFIELD_B,) + SHAPE_B, ("apply_bank", kind, options))
        assert plan.last_kernel_geometry().get("bank") == 3
        # the C ABI's own statement of the result: entry (j, i) is gcmf_apply with polynomial j on field i
        for j in (0, 2):
            one = tight(lambda ins, outs: plan.apply(ps[j], coef, ins, outs, NFIELD_B, device_ptrs=True, stream=stream), [f], f.shape, "f8", 1)
            assert np.array_equal(want[0][j * NFIELD_B:(j + 1) * NFIELD_B], one[0], equal_nan=True), (kind, j)
    finally:
        plan.close()


def test_apply_bank_gaps_on_caller_planes():
    import torch
    plan, ps, coef, _ = _scalar_plan("IRREGULAR_WITH_LAND", scales=(2.0, 3.0, 4.5))
    stream = torch.cuda.current_stream().cuda_stream
    try:
        P = np.stack(ps)
        f = _gappy(74)
        call = lambda ins, outs: plan.apply_bank(P, coef, ins[0], outs[0], NFIELD_B, stream=stream, faces_from_nan=True)
        want, _ = _three_layouts(call, [f], (len(ps) * NFIELD_B,) + SHAPE_B, "apply_bank_gaps")
        assert np.array_equal(np.isnan(want[0]), np.isnan(np.concatenate([f] * 3)))
    finally:
        plan.close()


def test_stacked_plan_on_caller_planes():
    """Plan.create_levels: three levels whose wet masks differ, six batch entries (entry b runs on level b % 3)."""
    import torch
    from gcm_filters_amd import GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS
    kind, nlev, nbatch = "IRREGULAR_WITH_LAND", 3, 6
    ny, nx = SHAPE_B
    single, (p,), coef, gv = _scalar_plan(kind)
    single.close()
    wet = np.stack([gv["wet_mask"]] * nlev)
    wet[1, 20:30, 40:70] = 0
    wet[2, 60:80, 100:104] = 0
    names = list(ALL_KERNELS[GridType[kind]].required_grid_args())
    planes = [wet if k == "wet_mask" else np.ascontiguousarray(gv[k]) for k in names]
    plan = _lib.Plan.create_levels(GridType[kind].value, _lib.F64, ny, nx, planes, [nlev if k == "wet_mask" else 1 for k in names], nlev)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        f = np.stack([T.random_field(SHAPE_B, 400 + i) for i in range(nbatch)])
        f = np.where(wet[np.arange(nbatch) % nlev] == 0, np.nan, f)
        call = lambda ins, outs: plan.apply(p, coef, ins, outs, nbatch, device_ptrs=True, stream=stream)
        _three_layouts(call, [f], f.shape, "stacked plan")
        assert plan.last_kernel_geometry().get("levels") == nlev
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the end of parts A and B: every predicate of the fallback table was seen on its unaligned side
# ------------------------------------------------------------------------------------------------------------------------------
def test_every_alignment_predicate_was_hit(monkeypatch, tmp_path):
    """From the kernels the tests above recorded (HITS); a predicate whose witness did not run in this session -- a selection with -k, a
    layout run on its own -- has its witness run here."""
    for f in FALLBACKS:
        if f.predicate not in HITS:
            cid, layout = f.witness
            with monkeypatch.context() as mp:
                run_table_case(BY_ID[cid], layout, mp, tmp_path)
        assert f.predicate in HITS, (f.predicate, "never ran on its unaligned side; witness", f.witness)
        cid, layout, kernel = HITS[f.predicate]
        assert layout != "aligned" and re.search(f.unaligned, kernel), (f.predicate, HITS[f.predicate])
    if GAP_LOAD4 not in HITS:
        test_faces_from_nan_on_caller_planes("IRREGULAR_WITH_LAND")
    assert HITS[GAP_LOAD4][1] == "in-shifted"
    print("\n" + "\n".join(f"{k}: {v}" for k, v in HITS.items()))


def test_fallback_table_names_cases():
    for f in FALLBACKS:
        assert f.witness[0] in BY_ID and f.witness[1] in LAYOUTS[1:], f


# ------------------------------------------------------------------------------------------------------------------------------
# C. overlapping `out` is refused as a byte range
# ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.678


def _status(fn, *a, **k):
    from gcm_filters_amd import _lib
    try:
        fn(*a, **k)
    except _lib.GcmfError as e:
        return e.status, e.message
    return _lib.OK, ""


@pytest.mark.parametrize("grid, dt", [("IRREGULAR_WITH_LAND", "f8"), ("VECTOR_C_GRID", "f4")], ids=["scalar-f8", "vector-f4"])
def test_overlapping_out_is_refused(grid, dt):
    """One sentinel-filled buffer; `in` and `out` are addresses inside it.  A refused call returns GCMF_ERR_INVALID_ARG, names the overlap
    and writes nothing.  The filter's result of an f32 plan is f64 (twice the bytes per cell), the Laplacian's has the plan dtype."""
    import torch
    from gcm_filters_amd import GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
    shape = ny, nx = (40, 64)
    vec = grid in T.VECTOR_GRIDS
    gv = T.vector_grid_vars(grid, shape) if vec else T.scalar_grid_vars(grid, shape)
    gv = {k: v.astype(dt) for k, v in gv.items()}
    clear_plan_cache()
    plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.dtype_code(dt), shape)
    ncomp, esz = (2 if vec else 1), np.dtype(dt).itemsize
    p = np.array([0.4, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01])
    R = 3 * ny * nx * 8                                   # bytes of the largest plane of these calls (three entries, f64)
    buf = torch.full((8 * R // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    bits = buf.view(torch.int64)
    sentinel_bits = int(np.float64(SENTINEL).view(np.int64))
    base = buf.data_ptr()
    row, entry = nx * esz, ny * nx * esz
    try:
        def calls(ins, outs, nb):
            yield "gcmf_apply", lambda: plan.apply(p, 0.1, ins[:ncomp], outs[:ncomp], nb, device_ptrs=True)
            yield "gcmf_laplacian", lambda: plan.laplacian(ins[:ncomp], outs[:ncomp], nb, device_ptrs=True)

        def refused(why, ins, outs, nb):
            for name, fn in calls(ins, outs, nb):
                st, msg = _status(fn)
                assert st == _lib.ERR_INVALID_ARG and "overlap" in msg and name in msg, (why, name, st, msg)
                torch.cuda.synchronize()
                assert bool((bits == sentinel_bits).all()), (why, name, "something was written")

        in0, in1, out0, out1 = base, base + 2 * R, base + 4 * R, base + 6 * R
        refused("out begins one row into in", [in0, in1], [in0 + row, out1], 1)
        refused("out begins at entry 1 of in", [in0, in1], [in0 + entry, out1], 3)
        refused("out ends inside in", [in0 + row, in1], [in0, out1], 1)
        if vec:
            refused("out[1] begins one row into in[1]", [in0, in1], [out0, in1 + row], 1)
            refused("out[0] overlaps in[1]", [in0, in1], [in1 + row, out1], 1)
            refused("out[0] overlaps in[1], batch", [in0, in1], [in1 + entry, out1], 3)
            refused("out[0] overlaps out[1]", [in0, in1], [out0, out0 + row], 1)
            refused("out[0] is out[1]", [in0, in1], [out0, out0], 1)
        st, msg = _status(plan.apply, p, 0.1, [in0, in1][:ncomp], [in0, in1][:ncomp], 1, device_ptrs=True)
        assert st == _lib.ERR_INVALID_ARG and "alias" in msg, (st, msg)             # (test_gpu_parity.py::test_in_place_is_rejected)
        # host pointers are held to the same rule
        host = np.full(4 * ny * nx, SENTINEL, dtype=dt)
        hp = host.ctypes.data
        far = [hp + 2 * entry, hp + 3 * entry]
        st, msg = _status(plan.laplacian, [hp, far[0]][:ncomp], [hp + row, far[1]][:ncomp], 1, device_ptrs=False)
        assert st == _lib.ERR_INVALID_ARG and "overlap" in msg, (st, msg)
        assert (host == np.asarray(SENTINEL, dtype=dt)).all()
    finally:
        clear_plan_cache()


def test_touching_planes_and_a_shared_input_stay_legal():
    """The check is on ranges, not wider: `out` may begin at the byte where `in` ends; and in[0] == in[1] -- nothing writes the input --
    gives what two copies of the field give."""
    import torch
    from gcm_filters_amd import Filter, GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
    shape = (40, 64)
    n = shape[0] * shape[1]
    plan, (p,), coef, gv = _scalar_plan("IRREGULAR_WITH_LAND", shape=shape)
    try:
        f = _wet_field(gv, shape, 600)
        call = lambda ins, outs: plan.apply(p, coef, ins, outs, 1, device_ptrs=True)
        want = tight(call, [f], (1,) + shape, "f8", 1)[0]
        assert np.isfinite(want).any()
        buf = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
        buf[:n].copy_(torch.from_numpy(f).reshape(-1))
        call([buf.data_ptr()], [buf.data_ptr() + n * 8])
        torch.cuda.synchronize()
        assert np.array_equal(buf[n:].cpu().numpy().reshape((1,) + shape), want, equal_nan=True)
        assert np.array_equal(buf[:n].cpu().numpy().reshape(shape), f, equal_nan=True)
    finally:
        plan.close()
    clear_plan_cache()
    try:
        (u, _), gvv = T.vector_case("VECTOR_C_GRID", shape)
        dx = T.grid_dx_min("VECTOR_C_GRID", gvv)
        vplan = ALL_KERNELS[GridType.VECTOR_C_GRID](**gvv)._plan(_lib.F64, shape)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=12, grid_type=GridType.VECTOR_C_GRID, grid_vars=gvv).filter_spec
        pv = np.asarray(spec.p, dtype=np.float64)
        for fn in (lambda ins, outs: vplan.apply(pv, 2 / spec.s_max, ins, outs, 1, device_ptrs=True),
                   lambda ins, outs: vplan.laplacian(ins, outs, 1, device_ptrs=True)):
            two = tight(fn, [u, u.copy()], (1,) + shape, "f8", 2)
            one = tight(lambda ins, outs: fn([ins[0], ins[0]], outs), [u], (1,) + shape, "f8", 2)
            assert all(np.isfinite(t).all() for t in two)
            same(one, two, "in[0] == in[1]")
    finally:
        clear_plan_cache()


# ------------------------------------------------------------------------------------------------------------------------------
# D. ordered on the caller's stream
# ------------------------------------------------------------------------------------------------------------------------------
DELAY_CYCLES = 20_000_000          # ~10 ms: only widens the window, the assertion holds for any delay


def _reference(call, fields, out_shapes, out_dt):
    """The call on the default stream with synchronisation around it."""
    import torch
    tdt = torch.float64 if out_dt == "f8" else torch.float32
    src = [torch.from_numpy(f).cuda() for f in fields]
    out = [torch.full(s, SENTINEL, dtype=tdt, device="cuda") for s in out_shapes]
    torch.cuda.synchronize()
    call(src, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _queue(st, call, pinned, src, out, delay=True):
    """Steps 1 .. 5 on stream `st`; returns the clones of the results (valid once `st` is synchronised)."""
    import torch
    with torch.cuda.stream(st):
        if delay:
            torch.cuda._sleep(DELAY_CYCLES)
        for s, h in zip(src, pinned):
            s.copy_(h, non_blocking=True)
        call(src, out, st.cuda_stream)
        res = [o.clone() for o in out]
        for o in out:
            o.fill_(SENTINEL)
        for s in src:
            s.zero_()
    return res


def _buffers(fields, out_shapes, out_dt):
    import torch
    tdt = torch.float64 if out_dt == "f8" else torch.float32
    pinned = [torch.from_numpy(np.ascontiguousarray(f)).pin_memory() for f in fields]
    src = [torch.full(tuple(f.shape), 7.0, dtype=h.dtype, device="cuda") for f, h in zip(fields, pinned)]
    out = [torch.full(s, SENTINEL, dtype=tdt, device="cuda") for s in out_shapes]
    return pinned, src, out


def ordered_on_a_stream(call, fields, out_shapes, out_dt="f8", what=""):
    """call(src tensors, out tensors, stream handle).  Returns the reference results."""
    import torch
    want = _reference(call, fields, out_shapes, out_dt)
    pinned, src, out = _buffers(fields, out_shapes, out_dt)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    res = _queue(st, call, pinned, src, out)
    st.synchronize()
    same([r.cpu().numpy() for r in res], want, (what, "queued on a stream between the caller's own work"))
    assert all(bool((o == SENTINEL).all()) for o in out) and all(bool((s == 0).all()) for s in src)
    return want


def _apply_call(plan, p, coef, nb, **flags):
    return lambda src, out, s: plan.apply(p, coef, [t.data_ptr() for t in src], [t.data_ptr() for t in out], nb, device_ptrs=True, stream=s, **flags)


def _wet_field(gv, shape, seed, nb=0):
    f = np.stack([T.random_field(shape, seed + i) for i in range(nb)]) if nb else T.random_field(shape, seed)
    return np.where(np.broadcast_to(gv["wet_mask"], f.shape) == 0, np.nan, f)


def test_stream_order_plain_strips():
    plan, (p,), coef, gv = _scalar_plan("IRREGULAR_WITH_LAND")
    try:
        plan.set_option("ringc_zip", 0)
        f = _wet_field(gv, SHAPE_B, 500)
        plan.last_kernel()
        ordered_on_a_stream(_apply_call(plan, p, coef, 1), [f], [SHAPE_B], what="plain strips")
        assert re.search(r"k_ringcs?<double, ", plan.last_kernel())
    finally:
        plan.close()


def test_stream_order_wet_row_tables():
    """The zipped strips cut from the wet rows: the FIRST eligible call of a plan builds the tables (it drains the caller's stream and
    uploads them with a blocking copy), later calls find them.  Here the first call of the plan is the queued one."""
    import torch
    shape = (192, 432)
    plan, (p,), coef, gv = _scalar_plan("IRREGULAR_WITH_LAND", shape=shape, n_steps=18)
    other, _, _, _ = _scalar_plan("IRREGULAR_WITH_LAND", shape=shape, n_steps=18)
    try:
        f = _wet_field(gv, shape, 510)
        for q in (plan, other):
            q.set_option("wet_rows", 2)
        call = _apply_call(plan, p, coef, 1)
        want = _reference(_apply_call(other, p, coef, 1), [f], [shape], "f8")       # (another plan: `plan` has not been called yet)
        assert "units" in other.last_kernel_geometry(), other.last_kernel_geometry()
        pinned, src, out = _buffers([f], [shape], "f8")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        first = _queue(st, call, pinned, src, out)           # builds the tables
        second = _queue(st, call, pinned, src, out, delay=False)
        st.synchronize()
        assert "units" in plan.last_kernel_geometry() and "k_ringcz<" in plan.last_kernel()
        same([first[0].cpu().numpy()], want, "the call that builds the wet-row tables")
        same([second[0].cpu().numpy()], want, "the call after it")
    finally:
        plan.close()
        other.close()


@pytest.mark.parametrize("band_seq_cells", [0, 3000000], ids=["band-beside", "band-after"])
def test_stream_order_tripolar_seam_band(band_seq_cells):
    """zip_fold = 0: k_fold_band advances the seam's rows beside every strip launch on the plan's side stream (fork / join with events on
    the caller's stream) or after it."""
    plan, (p,), coef, gv = _scalar_plan("TRIPOLAR_POP_WITH_LAND")
    try:
        plan.set_option("zip_fold", 0)
        plan.set_option("band_seq_cells", band_seq_cells)
        f = _wet_field(gv, SHAPE_B, 520)
        ordered_on_a_stream(_apply_call(plan, p, coef, 1), [f], [SHAPE_B], what=("tripolar", band_seq_cells))
    finally:
        plan.close()


def test_stream_order_apply_bank_two_polynomial_sets():
    """Two gcmf_apply_bank calls with different coefficient tables back to back: the second upload waits for the first call's kernels."""
    plan, ps, coef, gv = _scalar_plan("IRREGULAR_WITH_LAND", scales=(2.0, 3.0, 4.5, 6.0))
    try:
        Pa, Pb = np.stack(ps[:2]), np.stack(ps[2:])
        f = _wet_field(gv, SHAPE_B, 530, nb=NFIELD_B)

        def call(src, out, s):
            plan.apply_bank(Pa, coef, src[0].data_ptr(), out[0].data_ptr(), NFIELD_B, stream=s)
            plan.apply_bank(Pb, coef, src[0].data_ptr(), out[1].data_ptr(), NFIELD_B, stream=s)

        want = ordered_on_a_stream(call, [f], [(2, NFIELD_B) + SHAPE_B] * 2, what="apply_bank twice")
        assert not np.array_equal(want[0], want[1], equal_nan=True)
    finally:
        plan.close()


def test_stream_order_faces_from_nan():
    plan, (p,), coef, _ = _scalar_plan("IRREGULAR_WITH_LAND")
    try:
        f = _gappy(75)
        ordered_on_a_stream(_apply_call(plan, p, coef, NFIELD_B, faces_from_nan=True), [f], [f.shape], what="faces_from_nan")
    finally:
        plan.close()


def test_stream_order_on_chip_kernel(monkeypatch, tmp_path):
    monkeypatch.setenv("GCMF_RESIDENT", "1")
    monkeypatch.setenv("GCMF_RESIDENT_LOCK_DIR", str(tmp_path))
    plan, (p,), coef, gv = _scalar_plan("IRREGULAR_WITH_LAND")
    try:
        f = _wet_field(gv, SHAPE_B, 540)
        plan.last_kernel()
        ordered_on_a_stream(_apply_call(plan, p, coef, 1), [f], [SHAPE_B], what="on chip")
        assert "k_resident<" in plan.last_kernel(), plan.last_kernel()
    finally:
        plan.close()


def test_stream_order_cgrid_f32_batched_levels():
    from gcm_filters_amd import Filter, GridType, _lib
    from gcm_filters_amd.kernels import ALL_KERNELS, clear_plan_cache
    shape, nlev = SHAPE_B, 8
    clear_plan_cache()
    try:
        gv = {k: v.astype("f4") for k, v in T.vector_grid_vars("VECTOR_C_GRID", shape).items()}
        u = np.stack([T.random_field(shape, 42 + 2 * l) for l in range(nlev)]).astype("f4")
        v = np.stack([T.random_field(shape, 43 + 2 * l) for l in range(nlev)]).astype("f4")
        dx = T.grid_dx_min("VECTOR_C_GRID", gv)
        lap = ALL_KERNELS[GridType.VECTOR_C_GRID](**gv)
        plan = lap._plan(_lib.F32, shape)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=24, grid_type=GridType.VECTOR_C_GRID, grid_vars=gv).filter_spec
        p, coef = np.asarray(spec.p, dtype=np.float64), 2 / spec.s_max
        assert lap.is_dimensional
        plan.last_kernel()
        ordered_on_a_stream(_apply_call(plan, p, coef, nlev), [u, v], [(nlev,) + shape] * 2, what="C-grid f32 levels")
        assert "k_cgrid_ring<float, " in plan.last_kernel(), plan.last_kernel()
    finally:
        clear_plan_cache()


def test_two_streams_one_plan():
    """Call 1 on stream A behind a delay, call 2 on stream B right after it, another input and another polynomial, no host
    synchronisation until both are queued: the plan's work buffers and its polynomial on the device are shared, so call 2 must wait
    for call 1 (wait_for_work) and upload its coefficients only then (ensure_dev_p)."""
    import torch
    plan, (p1, p2), coef, gv = _scalar_plan("IRREGULAR_WITH_LAND", scales=(2.0, 6.0))
    try:
        plan.set_option("ringc_zip", 0)
        f1, f2 = _wet_field(gv, SHAPE_B, 550), _wet_field(gv, SHAPE_B, 551)
        want1 = _reference(_apply_call(plan, p1, coef, 1), [f1], [SHAPE_B], "f8")
        want2 = _reference(_apply_call(plan, p2, coef, 1), [f2], [SHAPE_B], "f8")
        assert not np.array_equal(want1[0], want2[0], equal_nan=True)
        b1, b2 = _buffers([f1], [SHAPE_B], "f8"), _buffers([f2], [SHAPE_B], "f8")
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        r1 = _queue(sa, _apply_call(plan, p1, coef, 1), *b1)
        r2 = _queue(sb, _apply_call(plan, p2, coef, 1), *b2, delay=False)
        sa.synchronize()
        sb.synchronize()
        same([r1[0].cpu().numpy()], want1, "call 1, stream A")
        same([r2[0].cpu().numpy()], want2, "call 2, stream B")
    finally:
        plan.close()
