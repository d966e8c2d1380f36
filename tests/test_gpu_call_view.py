"""A call carries what it sees of the grid in its own view, so nothing it does shows on the plan: the lock-free queries answer for the
plan itself while a flagged call runs on another thread, calls with different batches share a plan (the dask pattern:
``Filter._through_apply_ufunc`` calls ``apply`` from worker threads on one cached plan), a bank runs beside a flagged call, and a call
refused half-way leaves nothing behind.

IRREGULAR_WITH_LAND (``GCMF_FACES_FROM_NAN``) and REGULAR_WITH_LAND (``GCMF_MASK_FROM_NAN``) on (96, 160) float64, polynomials of 24
steps: nx % 4 == 0 and a backward cut exists.  Every comparison is bit for bit against the same call made alone.  The two threads of a
case race, so a case that passes proves nothing about a library that keeps per-call state on the plan -- one that fails does."""
import functools
import threading

import numpy as np
import pytest

from gcm_filters_amd import GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from test_gpu_filter_bank import make_bank
from test_gpu_level_stack import make_filter
from test_gpu_nan_mask import gappy_stack

pytestmark = pytest.mark.gpu

SHAPE, N_STEPS = (96, 160), 24
FLUX, MASK = "IRREGULAR_WITH_LAND", "REGULAR_WITH_LAND"
FLAG = {FLUX: "faces_from_nan", MASK: "mask_from_nan"}
NAN_MASK = {FLUX: "auto", MASK: True}


@functools.lru_cache(maxsize=None)
def grid_vars(kind, all_wet=False):
    gv = T.scalar_grid_vars(kind, SHAPE)
    if kind == FLUX:
        gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
    if all_wet:
        gv["wet_mask"] = np.ones_like(gv["wet_mask"])
    return gv


def plan_of(kind, gv):
    return ALL_KERNELS[GridType[kind]](**gv)._plan(_lib.F64, SHAPE)


def poly(kind, gv, n_steps=N_STEPS):
    """(p, c) as the Python driver hands them to gcmf_apply."""
    spec = make_filter(kind, gv, n_steps).filter_spec
    dimensional = ALL_KERNELS[GridType[kind]](**gv).is_dimensional
    return np.asarray(spec.p, dtype=np.float64), (2 / spec.s_max if dimensional else 2 / (spec.s_max * spec.dx_min_sq))


def queries(plan):
    return (plan.has_land(), tuple(plan.clenshaw_cut(N_STEPS, 1)), tuple(plan.clenshaw_cut(N_STEPS, 3)), tuple(plan.bank_cut(N_STEPS, 6)),
            plan.resident_supported(0, SHAPE[0], N_STEPS))


def run_threads(*targets):
    """Every target on its own thread; what they raised."""
    raised = []

    def guarded(fn):
        def run():
            try:
                fn()
            except BaseException as e:     # (reported by the caller: an exception in a thread is otherwise only printed)
                raised.append(e)
        return run
    threads = [threading.Thread(target=guarded(fn)) for fn in targets]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return raised


# ---- 1. the queries answer for the plan while a flagged call runs ---------------------------------------------------------------
@pytest.mark.parametrize("all_wet", [True, False], ids=["all-wet", "land"])
@pytest.mark.parametrize("kind", [FLUX, MASK])
def test_queries_during_a_flagged_call(kind, all_wet):
    import torch
    gv = grid_vars(kind, all_wet)
    plan = plan_of(kind, gv)
    p, c = poly(kind, gv)
    record = queries(plan)
    assert record[0] == (not all_wet) and record[1] and record[2], record
    x = torch.from_numpy(gappy_stack(SHAPE, 3, seed=21)).cuda()
    y = torch.empty_like(x)

    def flagged():
        plan.apply(p, c, [x.data_ptr()], [y.data_ptr()], 3, device_ptrs=True, **{FLAG[kind]: True})
        torch.cuda.synchronize()
        return y.cpu().numpy()
    alone = flagged()
    assert np.array_equal(np.isnan(alone), np.isnan(x.cpu().numpy()))      # (the flag took: NaN exactly in the gaps)
    assert queries(plan) == record
    done = threading.Event()
    wrong, differs, asked = [], [], [0]

    def caller():
        try:
            for k in range(8):
                if not np.array_equal(flagged(), alone, equal_nan=True):
                    wrong.append(k)
        finally:
            done.set()

    def asker():
        while not done.is_set() and asked[0] < 4000:
            q = queries(plan)
            asked[0] += 1
            if q != record:
                differs.append(q)
    raised = run_threads(caller, asker)
    print(f"{kind} all_wet={all_wet}: {asked[0]} rounds of queries beside 8 flagged calls, {len(differs)} differ")
    assert not raised, raised
    assert not differs, (record, differs[:3], len(differs), asked[0])
    assert not wrong, wrong
    assert queries(plan) == record


# ---- 2. different batches on one plan ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["unflagged", "flagged"])
@pytest.mark.parametrize("kind", [FLUX, MASK])
def test_different_batches_on_one_plan(kind, other):
    gv = grid_vars(kind)
    three, two = gappy_stack(SHAPE, 3, seed=22), gappy_stack(SHAPE, 2, seed=23)
    a = make_filter(kind, gv, N_STEPS, nan_mask=NAN_MASK[kind])
    b = make_filter(kind, gv, N_STEPS, nan_mask=NAN_MASK[kind] if other == "flagged" else False)
    want_a, want_b = a.apply(three), b.apply(two)
    wrong = []

    def work(flt, stack, want, who):
        def run():
            for k in range(6):
                if not np.array_equal(flt.apply(stack), want, equal_nan=True):
                    wrong.append((who, k))
        return run
    raised = run_threads(work(a, three, want_a, "flagged, batch 3"), work(b, two, want_b, f"{other}, batch 2"))
    assert not raised, raised          # (no GcmfError: "a stacked plan of 3 levels takes batches that are multiples of it", "a stacked plan")
    assert not wrong, wrong


# ---- 3. a bank beside a flagged call -----------------------------------------------------------------------------------------------
def test_bank_beside_a_flagged_call():
    gv = grid_vars(FLUX)
    bank = make_bank(FLUX, SHAPE, N_STEPS, gv=gv, nan_mask=False)
    flt = make_filter(FLUX, gv, N_STEPS, nan_mask="auto")
    fields = np.stack([T.random_field(SHAPE, 31 + k) for k in range(2)])
    fields[:, 0, :] = np.nan                                          # (the fixture's land row)
    gappy = gappy_stack(SHAPE, 3, seed=24)
    want_bank, want_flt = bank.apply(fields), flt.apply(gappy)
    assert bank.last_route == "bank"
    routes, wrong = [], []

    def banked():
        for k in range(6):
            got = bank.apply(fields)
            routes.append(bank.last_route)
            if not np.array_equal(got, want_bank, equal_nan=True):
                wrong.append(("bank", k))

    def flagged():
        for k in range(6):
            if not np.array_equal(flt.apply(gappy), want_flt, equal_nan=True):
                wrong.append(("flagged", k))
    raised = run_threads(banked, flagged)
    assert not raised, raised
    assert routes == ["bank"] * 6, routes            # (never "loop": gcmf_bank_cut answers for the plan, whatever runs beside)
    assert not wrong, wrong


# ---- 4. a refused call leaves nothing behind ---------------------------------------------------------------------------------------
def test_a_refused_call_leaves_nothing_behind():
    import torch
    gv = grid_vars(FLUX)
    plan = plan_of(FLUX, gv)
    off = make_filter(FLUX, gv, N_STEPS, nan_mask=False)
    stack = gappy_stack(SHAPE, 3, seed=25)
    lone = off.apply(stack[1])
    record = queries(plan)
    x = torch.from_numpy(stack).cuda()
    y = torch.empty_like(x)
    with pytest.raises(_lib.GcmfError) as e:         # refused INSIDE the call, the entries' planes in its view: three steps have no backward cut
        plan.apply(np.array([0.5, -0.3, 0.1, 0.05]), 0.2, [x.data_ptr()], [y.data_ptr()], 3, device_ptrs=True, faces_from_nan=True)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "no backward cut" in e.value.message
    assert queries(plan) == record
    assert np.array_equal(off.apply(stack[1]), lone, equal_nan=True)
    assert queries(plan) == record
