"""The contract of include/gcmf.h between the launch cut and the building blocks: gcmf_clenshaw_cut_batch returns the depths gcmf_apply uses
for a plan, a polynomial length and a batch, and a caller that runs those depths through gcmf_cheb_multi(GCMF_STEP_CLENSHAW) or
gcmf_slab_apply_backward gets gcmf_apply's bits.  SlabFilter (distributed.py), the row-block pipeline (host_blocks.py) and C callers rely on
it.  The plans below sit on both sides of every branch of clenshaw_cut (csrc/gcmf_api_blocks.hip): nine levels per launch on whole flux
grids (ringc9_ok), on whole tripolar grids whose launches advance the seam themselves (ringc_cut's fold strips: nx >= 256, nx % 4 == 0, 64 rows,
a batch of at most 64 fields that is not packed), on row slabs (option "slab_nines"), the cut search of cache-resident grids, the scalar
kinds behind plan->clenshaw = 2 and f32 state.  Results are held to gcmf_apply bit for bit and to the oracle (oracle/gcmf_oracle.py)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O

pytestmark = pytest.mark.gpu

SWEEP_N = list(range(1, 81)) + [127, 128, 129]
EQUIV_N = [5, 8, 9, 10, 16, 17, 27, 56, 63, 64, 65]
BATCHES = [1, 2, 16, 65]        # (65: one past the 64 fields k_ringcz's fold strips take)
SENTINEL = 12345.0

# id -> (grid, shape, dtype, Plan keywords, what to set on the plan, nines: "yes" = nine levels run in one launch (a lone field's 9 levels
# are cut [9]), "no" = never a 9, "may" = allowed)
PLANS = {
    "pop-200x392": ("TRIPOLAR_POP_WITH_LAND", (200, 392), _lib.F64, {}, {}, "yes"),
    "pop-64x256": ("TRIPOLAR_POP_WITH_LAND", (64, 256), _lib.F64, {}, {}, "yes"),
    "pop-63x256": ("TRIPOLAR_POP_WITH_LAND", (63, 256), _lib.F64, {}, {}, "no"),
    "pop-200x252": ("TRIPOLAR_POP_WITH_LAND", (200, 252), _lib.F64, {}, {}, "no"),
    "pop-200x390": ("TRIPOLAR_POP_WITH_LAND", (200, 390), _lib.F64, {}, {}, "no"),
    "irr-64x300": ("IRREGULAR_WITH_LAND", (64, 300), _lib.F64, {}, {}, "yes"),
    "irr-63x300": ("IRREGULAR_WITH_LAND", (63, 300), _lib.F64, {}, {}, "no"),
    "irr-720x1440": ("IRREGULAR_WITH_LAND", (720, 1440), _lib.F64, {}, {}, "may"),
    "tripreg-tuned": ("TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED", (128, 256), _lib.F64, {}, {"tuning": True}, "no"),
    "mom5u-tuned": ("MOM5U", (96, 160), _lib.F64, {}, {"tuning": True}, "yes"),
    "regland-tuned": ("REGULAR_WITH_LAND", (96, 160), _lib.F64, {}, {"tuning": True}, "no"),
    "irr-f32": ("IRREGULAR_WITH_LAND", (96, 160), _lib.F32, {}, {"clenshaw_f32": 1}, "no"),
    "mom5t-f32": ("MOM5T", (100, 72), _lib.F32, {}, {"clenshaw_f32": 1}, "no"),
    "irr-slab-nines0": ("IRREGULAR_WITH_LAND", (300, 392), _lib.F64, dict(row_begin=100, row_end=250, halo=9), {"slab_nines": 0}, "no"),
    "irr-slab-nines1": ("IRREGULAR_WITH_LAND", (300, 392), _lib.F64, dict(row_begin=100, row_end=250, halo=9), {"slab_nines": 1}, "yes"),
    "pop-top-slab": ("TRIPOLAR_POP_WITH_LAND", (200, 392), _lib.F64, dict(row_begin=100, row_end=200, halo=9), {"slab_nines": 1}, "no"),
    "irr-self-ring": ("IRREGULAR_WITH_LAND", (128, 256), _lib.F64, dict(halo=9, self_ring=True), {}, "no"),
}


def _grid(grid, shape, coast=""):
    f, gv = T.scalar_case(grid, shape)
    if coast:       # gcm_filters_amd.testing.coastline instead of the fixture mask
        gv["wet_mask"] = T.coastline(coast, shape, seed=33)
    return f, gv, ALL_KERNELS[GridType[grid]](**gv)


def _own_plan(pid):
    """A plan of this test's own (never the cached one Filter uses): tuning and options stay here."""
    grid, shape, dtype, kw, setup, _ = PLANS[pid]
    _, _, lap = _grid(grid, shape)
    planes = [np.asarray(a) for a in lap._planes]
    plan = _lib.Plan(GridType[grid].value, dtype, shape[0], shape[1], planes, **kw)
    if setup.get("tuning"):
        plan.set_tuning(multi_s=8, clenshaw=2)
    for k in ("slab_nines", "clenshaw_f32"):
        if k in setup:
            plan.set_option(k, setup[k])
    return plan


def _raw_cut(plan, n):
    buf = (C.c_int * 1024)()
    k = _lib.load().gcmf_clenshaw_cut(plan._h, int(n), buf, 1024)
    return [buf[i] for i in range(k)]


# ---- a. the shape of every cut -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pid", list(PLANS))
def test_cut_shape(pid):
    grid, shape, dtype, kw, setup, nines = PLANS[pid]
    plan = _own_plan(pid)
    try:
        for n in SWEEP_N:
            assert _raw_cut(plan, n) == plan.clenshaw_cut(n, 1), (pid, n)   # gcmf_clenshaw_cut = the batch-aware cut of one field
            for nb in BATCHES:
                cut = plan.clenshaw_cut(n, nb)
                if not cut:
                    continue
                assert sum(cut) == n, (pid, n, nb, cut)
                assert all(5 <= d <= 9 for d in cut), (pid, n, nb, cut)
                if nines == "no":
                    assert 9 not in cut, (pid, n, nb, cut)
                if dtype == _lib.F32:
                    assert cut[0] != 8, (pid, n, nb, cut)
        if nines == "yes":
            assert plan.clenshaw_cut(9, 1) == [9], (pid, plan.clenshaw_cut(9, 1))
        if nines == "no" and dtype == _lib.F64 and plan.clenshaw_cut(10, 1):
            assert plan.clenshaw_cut(9, 1) == [], pid      # (nine levels cannot be cut into launches of 5..8: the forward recurrence)
        if pid.startswith("pop-") and nines == "yes":
            # more fields than k_ringcz's fold strips take: the band of k_fold_band, eight levels at most
            assert max(plan.clenshaw_cut(63, 65)) == 8 and max(plan.clenshaw_cut(65, 65)) == 8
            assert plan.clenshaw_cut(9, 65) == []
        if pid in ("irr-f32", "mom5t-f32"):
            assert plan.clenshaw_cut(16), pid     # (the option is what turns the f32 backward evaluation on)
    finally:
        plan.close()


def test_no_ring_of_one_on_a_tripolar_grid():
    _, gv, lap = _grid("TRIPOLAR_POP_WITH_LAND", (200, 392))
    with pytest.raises(_lib.GcmfError):
        _lib.Plan(GridType.TRIPOLAR_POP_WITH_LAND.value, _lib.F64, 200, 392, [np.asarray(a) for a in lap._planes], halo=9, self_ring=True)


# ---- b. / c. the cut through the building blocks -------------------------------------------------------------------------------------

EQUIV = {   # id -> (compare with Filter.apply on the cached plan, oracle tolerance; None = NaN pattern only)
    "pop-200x392": (True, 1e-12),
    "pop-64x256": (True, 1e-12),
    "irr-64x300": (True, 1e-12),
    "mom5u-tuned": (False, 1e-12),
    "regland-tuned": (False, 1e-12),
    "irr-f32": (False, None),
}


def _filter(grid, gv, n):
    dx = T.grid_dx_min(grid, gv) if O.DIMENSIONAL[grid] else 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flt = Filter(filter_scale=4.0 * dx, dx_min=dx, n_steps=n, filter_shape=FilterShape.TAPER, grid_type=GridType[grid], grid_vars=gv)
    fs = flt.filter_spec
    p = np.asarray(fs.p, dtype=np.float64)
    c = 2 / fs.s_max if ALL_KERNELS[GridType[grid]].is_dimensional else 2 / (fs.s_max * fs.dx_min_sq)
    return flt, p, c


@functools.lru_cache(maxsize=None)
def _case(grid, shape, n, coast=""):
    """One field with NaN on land and in one wet cell, its filter, and the oracle's answer.  The fields of a batch are this one scaled by
    1 + 0.1 i: the oracle's answer scales with them, and a field that read another field's values would be off by far more than 1e-12."""
    f, gv, _ = _grid(grid, shape, coast)
    land = gv["wet_mask"] == 0
    f = np.where(land, np.nan, f)
    wet = np.argwhere(~land)
    j, i = wet[len(wet) // 3]
    f[j, i] = np.nan
    flt, p, c = _filter(grid, gv, n)
    fs = flt.filter_spec
    with np.errstate(all="ignore"):
        want = O.filter_func(O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq), grid, f, gv)
    return f, gv, flt, p, c, want


def _batch(f, nb):
    return np.stack([f * (1.0 + 0.1 * k) for k in range(nb)])


def _by_launches(plan, X, p, c, cut, nb, torch):
    """The levels as the launches of `cut` (gcmf_cheb_multi, GCMF_STEP_CLENSHAW) over the whole domain, then gcmf_land_fix."""
    n = len(p) - 1
    rows = X.shape[-2]
    s = torch.cuda.current_stream().cuda_stream
    pool = [torch.zeros_like(X) for _ in range(4)]
    out = torch.full(X.shape, SENTINEL, dtype=torch.float64, device=X.device)   # (the result is f64 whatever the state dtype)
    u = v = None
    lvl = 1
    for q, S in enumerate(cut):
        free = [b for b in pool if b is not u and b is not v]
        mode = _lib.STEP_CLENSHAW | (_lib.STEP_FIRST if q == 0 else 0) | (_lib.STEP_LAST if q == len(cut) - 1 else 0)
        pk = p[n - lvl - S + 1: n - lvl + 1][::-1]
        plan.cheb_multi(None if u is None else u.data_ptr(), None if v is None else v.data_ptr(), free[0].data_ptr(), free[1].data_ptr(),
                        X.data_ptr(), out.data_ptr(), pk, p[n], c, mode, nb, 0, rows, stream=s)
        u, v = free[0], free[1]
        lvl += S
    if plan.has_land():
        plan.land_fix(p, c, [X.data_ptr()], [out.data_ptr()], nb, stream=s)
    torch.cuda.synchronize()
    return out


def _by_slab_driver(plan, X, p, c, cut, nb, torch, resident):
    s = torch.cuda.current_stream().cuda_stream
    pool = [torch.zeros_like(X) for _ in range(4)]
    out = torch.full(X.shape, SENTINEL, dtype=torch.float64, device=X.device)   # (the result is f64 whatever the state dtype)
    plan.slab_apply_backward(None, None, None, None, p, c, cut, X.data_ptr(), [b.data_ptr() for b in pool], out.data_ptr(), nb, 0, 0,
                             stream=s, resident=resident)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def plans():
    made = {}
    yield made
    for pl in made.values():
        pl.close()


def _plan_for(pid, plans, gv):
    grid, shape, *_ = PLANS[pid]
    if EQUIV[pid][0]:
        return ALL_KERNELS[GridType[grid]](**gv)._plan(PLANS[pid][2], shape)      # Filter's own (cached) plan
    if pid not in plans:
        plans[pid] = _own_plan(pid)
    return plans[pid]


def _check_oracle(got, want, nb, tol):
    for k in range(nb):
        w = want * (1.0 + 0.1 * k)
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
        if tol is not None:
            ok = ~np.isnan(w)
            assert np.abs(got[k][ok] - w[ok]).max() <= tol * np.abs(w[ok]).max(), (k, np.abs(got[k][ok] - w[ok]).max())


@pytest.mark.parametrize("n", EQUIV_N)
@pytest.mark.parametrize("pid", list(EQUIV))
def test_cut_through_the_building_blocks_gives_gcmf_apply_bits(pid, n, plans):
    import torch
    grid, shape, dtype, *_ = PLANS[pid]
    use_filter, tol = EQUIV[pid]
    f, gv, flt, p, c, want = _case(grid, shape, n)
    plan = _plan_for(pid, plans, gv)
    tdt = torch.float64 if dtype == _lib.F64 else torch.float32
    s = torch.cuda.current_stream().cuda_stream
    one = plan.clenshaw_cut(n, 1)
    for nb in BATCHES:
        cut = plan.clenshaw_cut(n, nb)
        X = torch.from_numpy(_batch(f, nb)).to(tdt).cuda()
        if use_filter:
            with np.errstate(all="ignore"):
                ref = flt.apply(X).cpu().numpy()
        else:
            o = torch.empty(X.shape, dtype=torch.float64, device=X.device)
            plan.apply(p, c, [X.data_ptr()], [o.data_ptr()], nb, device_ptrs=True, stream=s)
            torch.cuda.synchronize()
            ref = o.cpu().numpy()
        _check_oracle(ref, want, nb, tol)
        if not cut:
            # (1..4 and 9 levels cannot be cut into launches of 5..8; f32 state never starts with eight levels)
            assert n < 5 or n == 9 or (dtype == _lib.F32 and n == 8), (pid, n, nb)
            continue
        got = _by_launches(plan, X, p, c, cut, nb, torch).cpu().numpy()
        assert np.array_equal(got, ref, equal_nan=True), (pid, n, nb, cut)
        # the lone field's cut on this batch: the same bits, or an error before any launch (a tripolar plan whose batch keeps the band)
        if one and one != cut:
            try:
                again = _by_launches(plan, X, p, c, one, nb, torch).cpu().numpy()
            except _lib.GcmfError as e:
                assert e.status == _lib.ERR_UNSUPPORTED and 9 in one, (pid, n, nb, one, e)
            else:
                assert np.array_equal(again, ref, equal_nan=True), (pid, n, nb, one)


@pytest.mark.parametrize("n", EQUIV_N)
@pytest.mark.parametrize("pid", list(EQUIV))
def test_cut_through_the_slab_driver_gives_gcmf_apply_bits(pid, n, plans):
    import torch
    grid, shape, dtype, *_ = PLANS[pid]
    use_filter, tol = EQUIV[pid]
    f, gv, flt, p, c, want = _case(grid, shape, n)
    plan = _plan_for(pid, plans, gv)
    tdt = torch.float64 if dtype == _lib.F64 else torch.float32
    s = torch.cuda.current_stream().cuda_stream
    one = plan.clenshaw_cut(n, 1)
    for nb in BATCHES:
        cut = plan.clenshaw_cut(n, nb)
        if not cut:
            continue
        X = torch.from_numpy(_batch(f, nb)).to(tdt).cuda()
        o = torch.empty(X.shape, dtype=torch.float64, device=X.device)
        plan.apply(p, c, [X.data_ptr()], [o.data_ptr()], nb, device_ptrs=True, stream=s)
        torch.cuda.synchronize()
        ref = o.cpu().numpy()
        for resident in (True, False):
            got = _by_slab_driver(plan, X, p, c, cut, nb, torch, resident).cpu().numpy()
            assert np.array_equal(got, ref, equal_nan=True), (pid, n, nb, cut, resident)
        _check_oracle(got, want, nb, tol)
        if one and one != cut:
            try:
                out = _by_slab_driver(plan, X, p, c, one, nb, torch, False)
            except _lib.GcmfError as e:
                assert e.status == _lib.ERR_UNSUPPORTED and 9 in one, (pid, n, nb, one, e)
            else:
                assert np.array_equal(out.cpu().numpy(), ref, equal_nan=True), (pid, n, nb, one)


def test_refused_depths_leave_no_result():
    """A nine-level launch on a tripolar plan whose batch keeps k_fold_band: an error from gcmf_cheb_multi and from the slab driver before
    anything is written (the output keeps its sentinel)."""
    import torch
    grid, shape = "TRIPOLAR_POP_WITH_LAND", (200, 392)
    f, gv, flt, p, c, want = _case(grid, shape, 63)
    plan = ALL_KERNELS[GridType[grid]](**gv)._plan(_lib.F64, shape)
    assert plan.clenshaw_cut(63, 1) == [9] * 7 and 9 not in plan.clenshaw_cut(63, 65)
    X = torch.from_numpy(_batch(f, 65)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    pool = [torch.zeros_like(X) for _ in range(4)]
    out = torch.full(X.shape, SENTINEL, dtype=torch.float64, device=X.device)   # (the result is f64 whatever the state dtype)
    with pytest.raises(_lib.GcmfError) as e:
        plan.cheb_multi(None, None, pool[0].data_ptr(), pool[1].data_ptr(), X.data_ptr(), out.data_ptr(), p[54:63][::-1], p[63], c,
                        _lib.STEP_CLENSHAW | _lib.STEP_FIRST, 65, 0, shape[0], stream=s)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "nine levels" in e.value.message, e.value
    with pytest.raises(_lib.GcmfError) as e:   # (rows short of the seam: the band, so no nines either)
        plan.cheb_multi(None, None, pool[0].data_ptr(), pool[1].data_ptr(), X.data_ptr(), out.data_ptr(), p[54:63][::-1], p[63], c,
                        _lib.STEP_CLENSHAW | _lib.STEP_FIRST, 1, 0, shape[0] - 1, stream=s)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.GcmfError) as e:
        plan.slab_apply_backward(None, None, None, None, p, c, [9] * 7, X.data_ptr(), [b.data_ptr() for b in pool], out.data_ptr(), 65, 0, 0,
                                 stream=s, resident=False)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "nine levels" in e.value.message, e.value
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- d. SlabFilter on one rank -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_steps", [63, 65])
@pytest.mark.parametrize("grid,exchange,self_ring", [("TRIPOLAR_POP_WITH_LAND", "auto", False), ("TRIPOLAR_POP_WITH_LAND", "p2p", False),
                                                     ("IRREGULAR_WITH_LAND", "p2p", True), ("IRREGULAR_WITH_LAND", "native", True),
                                                     ("IRREGULAR_WITH_LAND:open_south", "native", True)])
def test_slab_filter_of_one_rank(grid, exchange, self_ring, n_steps):
    """SlabFilter(rank=0, world=1) cuts a whole grid as gcmf_apply does for the batch in hand (the tripolar grid's nines depend on it) and a
    ring of one rank as the slab drivers do (nines by option "slab_nines"); either way Filter.apply's bits.  (A tripolar grid is not periodic
    in y: no ring of one there.)  With the fixture mask the face a ring of one exchanges across is closed (row 0 is land); the `open_south`
    coastline (gcm_filters_amd.testing.coastline) keeps it live."""
    from gcm_filters_amd.distributed import SlabFilter
    shape = (200, 392)
    grid, _, coast = grid.partition(":")
    f, gv, flt, p, c, want = _case(grid, shape, n_steps, coast)
    assert not coast or (gv["wet_mask"][0] * gv["wet_mask"][-1]).any()
    dx = T.grid_dx_min(grid, gv)
    fk = dict(filter_scale=4.0 * dx, dx_min=dx, n_steps=n_steps, filter_shape=FilterShape.TAPER)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sf = SlabFilter(grid, gv, fk, shape[0], shape[1], halo=9 if self_ring else None, dtype=np.float64, device=0, rank=0, world=1,
                        self_ring=self_ring, exchange=exchange)
    assert sf.n_steps == n_steps and sf.backward_cut
    for nb in (1, 2, 16):
        fb = _batch(f, nb)
        with np.errstate(all="ignore"):
            got = sf.apply_local(sf.scatter_from_global([fb]))[0].cpu().numpy()
            ref = flt.apply(fb)
        assert np.array_equal(got, ref, equal_nan=True), (grid, exchange, self_ring, n_steps, nb, sf._cut_for(nb))
        _check_oracle(got, want, nb, 1e-12)
    if grid.startswith("TRIPOLAR"):
        assert 9 in sf._cut_for(1)
        with pytest.raises(ValueError):
            SlabFilter(grid, gv, fk, shape[0], shape[1], halo=9, dtype=np.float64, device=0, rank=0, world=1, self_ring=True)
