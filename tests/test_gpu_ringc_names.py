"""What ``Plan.last_kernel()`` and ``Plan.last_kernel_geometry()`` report for the backward strip launches, character for character:
bench.py's traffic records and the dispatch tests key on these strings, and one helper (``kernel_name``, csrc/gcmf_internal.hpp) and one
launcher (``launch_ringc_sf``, csrc/gcmf_ringc_impl.hpp) now build them for every entry form.

A float64 IRREGULAR_WITH_LAND grid of 96 x 160 with land (the shape of tests/test_gpu_level_stack.py: nx % 4 == 0, 64 rows or more, so
nine levels run), two fields, through each entry form the dispatcher knows on such a plan -- an ordinary batch (as the library cuts
it: the packed column and the zipped strips; and as whole strips per field: ``k_ringcs``, ``k_ringc`` at nine levels), a stacked plan of
two levels, a ``FilterBank`` of two scales, ``FilterBank(nan_mask="auto")`` on gappy fields, and a lone field (the zipped strips) -- at
``n_steps`` 5 .. 9 (every depth as a single first launch) and 18 (two launches).  The strings below were recorded by running this file on
the commit before the dispatch table; what follows ``rows=<n>`` in the geometry is compared as the C ABI returns it.

Every case also has the bits of the route the existing tests hold it to (the fields one by one, the plain strips for the zipped ones, the
per-level plans, the loop over ``bank.filters``): the launch ran the right instantiation and not just a like-named one."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_filter_bank as FB
import test_gpu_gap_fold as GF
import test_gpu_level_stack as LS
from gcm_filters_amd import _lib
from test_gpu_nan_mask import gappy_stack

pytestmark = pytest.mark.gpu

KIND, SHAPE = "IRREGULAR_WITH_LAND", (96, 160)
SCALES = (2.0, 4.5)
N_STEPS = [5, 6, 7, 8, 9, 18]

# (case, n_steps) -> (last_kernel(), what follows "rows=96" in last_kernel_geometry())
EXPECTED = {
    ("batch", 5): ("gcmf::k_ringcp<double, 2, 5, true, true>", ""),
    ("batch", 6): ("gcmf::k_ringcz<double, 6, true, false>", ""),
    ("batch", 7): ("gcmf::k_ringcz<double, 7, true, false>", ""),
    ("batch", 8): ("gcmf::k_ringcz<double, 8, true, false>", ""),
    ("batch", 9): ("gcmf::k_ringcz<double, 9, true, false>", ""),
    ("batch", 18): ("gcmf::k_ringcz<double, 9, false, false>", ""),
    ("batch_strips", 5): ("gcmf::k_ringcs<double, 5, true>", ""),
    ("batch_strips", 6): ("gcmf::k_ringcs<double, 6, true>", ""),
    ("batch_strips", 7): ("gcmf::k_ringcs<double, 7, true>", ""),
    ("batch_strips", 8): ("gcmf::k_ringcs<double, 8, true>", ""),
    ("batch_strips", 9): ("gcmf::k_ringc<double, 2, 9, true>", ""),
    ("batch_strips", 18): ("gcmf::k_ringc<double, 2, 9, false>", ""),
    ("stacked", 5): ("gcmf::k_ringc<double, 2, 5, true>", " levels=2"),
    ("stacked", 6): ("gcmf::k_ringc<double, 2, 6, true>", " levels=2"),
    ("stacked", 7): ("gcmf::k_ringc<double, 2, 7, true>", " levels=2"),
    ("stacked", 8): ("gcmf::k_ringc<double, 2, 8, true>", " levels=2"),
    ("stacked", 9): ("gcmf::k_ringc<double, 2, 9, true>", " levels=2"),
    ("stacked", 18): ("gcmf::k_ringc<double, 2, 9, false>", " levels=2"),
    ("bank", 5): ("gcmf::k_ringc<double, 2, 5, true>", " bank=2"),
    ("bank", 6): ("gcmf::k_ringc<double, 2, 6, true>", " bank=2"),
    ("bank", 7): ("gcmf::k_ringc<double, 2, 7, true>", " bank=2"),
    ("bank", 8): ("gcmf::k_ringc<double, 2, 8, true>", " bank=2"),
    ("bank", 9): ("gcmf::k_ringc<double, 2, 9, true>", " bank=2"),
    ("bank", 18): ("gcmf::k_ringc<double, 2, 9, false>", " bank=2"),
    ("bank_gaps", 5): ("gcmf::k_ringc<double, 2, 5, true>", " levels=2 bank=2"),
    ("bank_gaps", 6): ("gcmf::k_ringc<double, 2, 6, true>", " levels=2 bank=2"),
    ("bank_gaps", 7): ("gcmf::k_ringc<double, 2, 7, true>", " levels=2 bank=2"),
    ("bank_gaps", 8): ("gcmf::k_ringc<double, 2, 8, true>", " levels=2 bank=2"),
    ("bank_gaps", 9): ("gcmf::k_ringc<double, 2, 9, true>", " levels=2 bank=2"),
    ("bank_gaps", 18): ("gcmf::k_ringc<double, 2, 9, false>", " levels=2 bank=2"),
    ("lone", 5): ("gcmf::k_ringcz<double, 5, true, false>", ""),
    ("lone", 6): ("gcmf::k_ringcz<double, 6, true, false>", ""),
    ("lone", 7): ("gcmf::k_ringcz<double, 7, true, false>", ""),
    ("lone", 8): ("gcmf::k_ringcz<double, 8, true, false>", ""),
    ("lone", 9): ("gcmf::k_ringcz<double, 9, true, false>", ""),
    ("lone", 18): ("gcmf::k_ringcz<double, 9, false, false>", ""),
}


def geometry_tail(plan):
    buf = C.create_string_buffer(256)
    _lib.check(_lib.load().gcmf_last_kernel_geometry(plan._h, buf, 256))
    text = buf.value.decode()
    head, sep, tail = text.partition(f"rows={SHAPE[0]}")
    assert sep and head.startswith("H="), text
    return tail


class Ran:
    """Reads the names between the call under test and the reference calls (which launch kernels of their own on the same plan)."""

    def __init__(self, plan):
        self.plan = plan
        plan.last_kernel()          # (reading it resets "the deepest kernel since the last read")

    def read(self):
        self.kernel, self.tail = self.plan.last_kernel(), geometry_tail(self.plan)


def batch(n):
    gv = FB.grid_vars(KIND, SHAPE)
    flt, f = LS.make_filter(KIND, gv, n), FB.field_for(SHAPE, lead=(2,))
    ran = Ran(FB.plan_of(KIND, SHAPE))
    got = flt.apply(f)
    ran.read()
    return ran, got, np.stack([flt.apply(f[k]) for k in range(2)])


def batch_strips(n):
    """The same batch with the zipped strips and the packed walk switched off: whole strips per field."""
    gv = FB.grid_vars(KIND, SHAPE)
    flt, f = LS.make_filter(KIND, gv, n), FB.field_for(SHAPE, lead=(2,))
    ran = Ran(FB.plan_of(KIND, SHAPE))
    try:
        ran.plan.set_option("ringc_zip", 0)
        ran.plan.set_option("pack_batch", 0)
        got = flt.apply(f)
        ran.read()
    finally:
        ran.plan.set_option("ringc_zip", 1)
        ran.plan.set_option("pack_batch", 1)
    return ran, got, np.stack([flt.apply(f[k]) for k in range(2)])


def lone(n):
    gv = FB.grid_vars(KIND, SHAPE)
    flt, f = LS.make_filter(KIND, gv, n), FB.field_for(SHAPE)
    ran = Ran(FB.plan_of(KIND, SHAPE))
    got = flt.apply(f)
    ran.read()
    try:
        ran.plan.set_option("ringc_zip", 0)
        want = flt.apply(f)
        assert "k_ringcz" not in ran.plan.last_kernel()
    finally:
        ran.plan.set_option("ringc_zip", 1)
    return ran, got, want


def stacked(n):
    gv = LS.level_grid_vars(KIND, SHAPE, 2)
    flt, f = LS.make_filter(KIND, gv, n), LS.fields_for(SHAPE, 2, 1)
    ran = Ran(LS.stacked_lap(KIND, gv)._stacked_plan())
    got = flt.apply(f)
    ran.read()
    return ran, got, LS.per_level(KIND, gv, f, n)


def bank(n):
    b, f = FB.make_bank(KIND, SHAPE, n, SCALES), FB.field_for(SHAPE, lead=(2,))
    ran = Ran(FB.plan_of(KIND, SHAPE))
    got = b.apply(f)
    ran.read()
    assert b.last_route == "bank"
    return ran, got, FB.loop_of(b, f)


def bank_gaps(n):
    gv = GF.grid_vars(KIND, SHAPE)
    b, f = FB.make_bank(KIND, SHAPE, n, SCALES, gv=gv, nan_mask="auto"), gappy_stack(SHAPE, 2, seed=40)
    ran = Ran(GF.plan_of(KIND, gv, SHAPE))
    got = b.apply(f)
    ran.read()
    assert b.last_route == "bank"
    return ran, got, FB.loop_of(b, f)


CASES = {"batch": batch, "batch_strips": batch_strips, "stacked": stacked, "bank": bank, "bank_gaps": bank_gaps, "lone": lone}


@pytest.mark.parametrize("n_steps", N_STEPS)
@pytest.mark.parametrize("case", list(CASES))
def test_names_and_geometry(monkeypatch, case, n_steps):
    monkeypatch.setenv("GCMF_STACK_LEVELS", "1")      # (two levels are stacked only when asked: tests/test_gpu_level_stack.py)
    ran, got, want = CASES[case](n_steps)
    print(f'    ("{case}", {n_steps}): ("{ran.kernel}", "{ran.tail}"),')
    assert (ran.kernel, ran.tail) == EXPECTED[(case, n_steps)]
    got, want = FB.host(got), FB.host(want)
    assert got.shape == want.shape and np.isfinite(got).any()
    assert np.array_equal(got, want, equal_nan=True), LS.rel_err(got, want)


def test_every_entry_form_and_depth_is_named():
    """The cases between them: k_ringc at 5 .. 9 levels as a first launch in each of its per-entry forms, and k_ringcz."""
    for case, tail in (("stacked", " levels=2"), ("bank", " bank=2"), ("bank_gaps", " levels=2 bank=2")):
        for S in (5, 6, 7, 8, 9):
            assert EXPECTED[(case, S)] == (f"gcmf::k_ringc<double, 2, {S}, true>", tail), (case, S)
        assert EXPECTED[(case, 18)] == ("gcmf::k_ringc<double, 2, 9, false>", tail), case
    assert all(EXPECTED[("lone", n)][0].startswith("gcmf::k_ringcz<double, ") for n in N_STEPS)
