"""``FilterBank``: one field filtered at many scales in one call.  On float64 IRREGULAR_WITH_LAND / MOM5U / MOM5T grids the scales are one
batch of the backward evaluation with a polynomial per entry (``gcmf_apply_bank``: ``k_ringc`` / ``k_land_fix`` in their per-entry
polynomial instantiations); everything else loops over ``bank.filters``.

The contract: ``bank.apply(f)[j]`` is what ``bank.filters[j].apply(f)`` returns -- bit for bit -- and that is the reference's
``filter_func`` with scale j's polynomial (the oracle, once per scale).  Shapes: (96, 160), two column windows that wrap, and (200, 520),
five windows and several strips.  Gates are those of tests/test_gpu_parity.py: identical NaN pattern and rel_err <= 1e-11 against the oracle.
Polynomials of 24, 14, 63 and 20 steps are cut into launches of (8 8 8), (8 6), (9 x 7) and (8 7 5) levels -- every depth from 5 to 9, read
from ``plan.bank_cut`` and asserted; a first launch is the deepest of its cut, so ``test_first_launches_of_every_depth`` runs the five- to
seven-level first launches through the plan option ``ringc_smax``."""
import functools
import warnings

import numpy as np
import pytest

from gcm_filters_amd import Filter, FilterBank, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS
from oracle import gcmf_oracle as O
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

KINDS = ["IRREGULAR_WITH_LAND", "MOM5U", "MOM5T"]
SMALL, BLOCKED = (96, 160), (200, 520)
N_STEPS = [24, 14, 63, 20]
THREE, FIVE = (2.0, 3.0, 4.5), (2.0, 2.6, 3.0, 4.5, 6.0)     # x dx_min


@functools.lru_cache(maxsize=None)
def grid_vars(kind, shape):
    return T.scalar_grid_vars(kind, shape)


def make_bank(kind, shape, n_steps, scales=THREE, gv=None, **kw):
    gv = grid_vars(kind, shape) if gv is None else gv
    dx = T.grid_dx_min(kind, gv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # ("n_steps below the default": the polynomials here are chosen for their launch cuts)
        return FilterBank(filter_scales=[s * dx for s in scales], dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=n_steps,
                          grid_type=GridType[kind], grid_vars=gv, **kw)


def plan_of(kind, shape, gv=None):
    """The cached ordinary plan the bank and its filters run on."""
    gv = grid_vars(kind, shape) if gv is None else gv
    return ALL_KERNELS[GridType[kind]](**gv)._plan(_lib.F64, shape)


def field_for(shape, seed=700, lead=()):
    """Random fields with NaN on the fixture mask's land row and FINITE values on the other land cells (the south-west quadrant): those
    evolve on their own polynomial, which differs per scale."""
    n = int(np.prod(lead, dtype=int)) if lead else 1
    f = np.stack([T.random_field(shape, seed + k) for k in range(n)]).reshape(tuple(lead) + shape)
    f[..., 0, :] = np.nan
    return f


@functools.lru_cache(maxsize=None)
def _oracle(kind, shape, n_steps, scale, seed):
    gv = grid_vars(kind, shape)
    dx = T.grid_dx_min(kind, gv)
    spec = O.filter_spec(scale * dx, dx, "TAPER", np.pi, 2, n_steps)
    with np.errstate(all="ignore"):
        return O.filter_func(spec, kind, field_for(shape, seed), gv)


def oracle_of(bank, kind, field, gv):
    """The reference's filter_func once per scale and 2-D slice, with the bank's own polynomials."""
    flat = field.reshape((-1,) + field.shape[-2:])
    out = []
    with np.errstate(all="ignore"):
        for fs in bank.filter_specs:
            spec = O.FilterSpec(fs.n_steps, fs.s_max, np.asarray(fs.p), fs.dx_min_sq)
            out.append(np.stack([O.filter_func(spec, kind, f, gv) for f in flat]).reshape(field.shape))
    return np.stack(out)


def check(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern")
    err = rel_err(got, want)
    print(f"{what}: rel_err {err:.3e}")
    assert err <= 1e-11, (what, err)


def loop_of(bank, field):
    outs = [f.apply(field) for f in bank.filters]
    return np.stack([o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in outs])


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- 1. oracle parity per scale -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("n_steps, scales", [(24, THREE), (14, THREE), (63, THREE), (20, THREE), (24, FIVE), (63, FIVE)])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_parity_per_scale(kind, n_steps, scales, shape):
    gv = grid_vars(kind, shape)
    bank = make_bank(kind, shape, n_steps, scales)
    plan = plan_of(kind, shape)
    M = len(scales)
    cut = plan.bank_cut(n_steps, M)
    assert cut and sum(cut) == n_steps and all(5 <= s <= 9 for s in cut), cut
    f = field_for(shape)
    plan.last_kernel()
    got = bank.apply(f)
    ran, geom = plan.last_kernel(), plan.last_kernel_geometry()
    assert bank.last_route == "bank" and bank.last_path == "strips"
    assert isinstance(got, np.ndarray) and got.shape == (M,) + shape and got.dtype == np.float64
    assert ran.startswith(f"gcmf::k_ringc<double, 2, {max(cut)}, "), (ran, cut)
    assert list(geom)[-1] == "bank" and geom["bank"] == M and geom["grid"].endswith(f"x{M}"), geom
    want = np.stack([_oracle(kind, shape, n_steps, s, 700) for s in scales])
    check(got, want, (kind, n_steps, scales, shape, ran, cut))
    # the land cells' own polynomial, per scale (k_land_fix's per-entry form)
    land = gv["wet_mask"] == 0
    land[0, :] = False
    assert land.sum() > 100 and np.isfinite(got[:, land]).all()
    check(got[:, land], want[:, land], (kind, n_steps, shape, "land"))
    for j in range(1, M):
        assert not np.array_equal(got[j][land], got[0][land]), j


def test_the_polynomials_run_every_depth_from_5_to_9():
    seen, first = set(), set()
    for shape in (SMALL, BLOCKED):
        plan = plan_of("IRREGULAR_WITH_LAND", shape)
        for n in N_STEPS:
            for M in (3, 5):
                cut = plan.bank_cut(n, M)
                seen |= set(cut)
                first.add(cut[0])
    assert seen == {5, 6, 7, 8, 9}, seen
    assert first == {8, 9}, first      # (five to seven levels as a first launch: the next test)


@pytest.mark.parametrize("smax", [5, 6, 7])
def test_first_launches_of_every_depth(smax):
    """However the levels are cut, the bits are the same: the five-, six- and seven-level FIRST launches against the default cut."""
    import torch
    kind, shape = "IRREGULAR_WITH_LAND", BLOCKED
    bank = make_bank(kind, shape, 5 * smax)
    plan = plan_of(kind, shape)
    f = torch.from_numpy(field_for(shape)).cuda()
    want = bank.apply(f).cpu().numpy()
    assert bank.last_route == "bank"
    try:
        plan.set_option("ringc_smax", smax)
        assert plan.bank_cut(5 * smax, 3) == [smax] * 5
        plan.last_kernel()
        got = bank.apply(f).cpu().numpy()
        assert bank.last_route == "bank" and plan.last_kernel().startswith(f"gcmf::k_ringc<double, 2, {smax}, "), smax
    finally:
        plan.set_option("ringc_smax", 0)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    assert np.array_equal(want, loop_of(bank, f), equal_nan=True)


# ---- 2. the bits of the loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
@pytest.mark.parametrize("n_steps", [24, 63])
@pytest.mark.parametrize("kind", KINDS)
def test_the_bits_of_the_loop(kind, n_steps, shape):
    import torch
    bank = make_bank(kind, shape, n_steps)
    f = torch.from_numpy(field_for(shape)).cuda()
    got = bank.apply(f)
    assert bank.last_route == "bank" and torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64
    assert tuple(got.shape) == (3,) + shape
    want = loop_of(bank, f)
    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), rel_err(got.cpu().numpy(), want)


@pytest.mark.parametrize("lead", [(), (2,), (2, 3)], ids=["1", "2", "2x3"])
@pytest.mark.parametrize("where", ["device", "numpy"])
def test_the_bits_of_the_loop_with_leading_axes(where, lead):
    import torch
    kind, shape = "MOM5T", BLOCKED
    bank = make_bank(kind, shape, 20, FIVE)
    f = field_for(shape, 710, lead)
    x = torch.from_numpy(f).cuda() if where == "device" else f
    plan_of(kind, shape).last_kernel()      # (reading it forgets the deepest launch so far)
    got = bank.apply(x)
    assert bank.last_route == "bank"
    assert (torch.is_tensor(got) and got.is_cuda) if where == "device" else isinstance(got, np.ndarray)
    assert tuple(got.shape) == (5,) + tuple(lead) + shape
    assert plan_of(kind, shape).last_kernel_geometry()["grid"].endswith(f"x{5 * max(1, int(np.prod(lead, dtype=int)))}")
    want = loop_of(bank, x)
    assert np.array_equal(host(got), want, equal_nan=True), rel_err(host(got), want)


# ---- 3. a NaN in a wet cell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BLOCKED], ids=["96x160", "200x520"])
def test_nan_in_a_wet_cell(shape):
    """The strips that meet the NaN are redone by the nan_to_num march, with their entries' own coefficients."""
    import torch
    kind, n_steps = "IRREGULAR_WITH_LAND", 24
    ny, nx = shape
    gv = grid_vars(kind, shape)
    bank = make_bank(kind, shape, n_steps)
    plan = plan_of(kind, shape)
    f = field_for(shape, 720, (2,))
    jw, iw = 3 * ny // 4, 3 * nx // 4
    assert gv["wet_mask"][jw, iw] == 1
    f[1, jw, iw] = np.nan
    x = torch.from_numpy(f).cuda()
    plan.ring_fallbacks()
    got = bank.apply(x).cpu().numpy()
    assert bank.last_route == "bank" and plan.ring_fallbacks() > 0     # the redo march ran
    want = loop_of(bank, x)
    assert np.array_equal(got, want, equal_nan=True), rel_err(got, want)
    assert np.isnan(got[:, 1, jw, iw]).all() and np.isfinite(got[:, 1, jw - 1:jw + 2, iw + 1]).all()
    check(got, oracle_of(bank, kind, f, gv), ("a NaN in a wet cell", shape))


# ---- 4. cutting --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [4, 2], ids=["4-entries", "2-entries"])
@pytest.mark.parametrize("where", ["device", "numpy"])
def test_sweeps_longer_than_the_bound_are_cut(monkeypatch, where, bound):
    """Five scales x three fields with at most four entries per call (one scale and all fields each) and at most two (a scale's fields in
    two calls): the cuts leave every entry in its place."""
    import torch
    kind, shape = "MOM5U", SMALL
    bank = make_bank(kind, shape, 14, FIVE)
    f = field_for(shape, 730, (3,))
    x = torch.from_numpy(f).cuda() if where == "device" else f
    whole = host(bank.apply(x))
    calls = []
    cls = _lib.Plan
    orig = cls.apply_bank
    monkeypatch.setattr(cls, "apply_bank", lambda self, p, c, s, o, n, **k: calls.append((len(p), n)) or orig(self, p, c, s, o, n, **k))
    monkeypatch.setenv("GCMF_BANK_ENTRIES", str(bound))
    got = host(bank.apply(x))
    assert bank.last_route == "bank"
    assert calls == ([(1, 3)] * 5 if bound == 4 else [(1, 2), (1, 1)] * 5), calls
    assert np.array_equal(got, whole, equal_nan=True)
    assert np.array_equal(got, loop_of(bank, x), equal_nan=True)


def test_two_tables_back_to_back_on_one_stream():
    """gcmf_apply_bank twice on one stream with DIFFERENT tables of one size and nothing in between: the second upload waits for the first
    call's kernels."""
    import torch
    kind, shape = "IRREGULAR_WITH_LAND", BLOCKED
    plan = plan_of(kind, shape)
    a, b = make_bank(kind, shape, 24, (2.0, 3.0, 4.5)), make_bank(kind, shape, 24, (5.0, 2.5, 3.5))
    Pa, Pb = (np.stack([np.asarray(s.p) for s in bk.filter_specs]) for bk in (a, b))
    c = 2 / a.filter_specs[0].s_max
    f = torch.from_numpy(field_for(shape, 740, (2,))).cuda()
    oa, ob = (torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    plan.apply_bank(Pa, c, f.data_ptr(), oa.data_ptr(), 2, stream=stream)
    plan.apply_bank(Pb, c, f.data_ptr(), ob.data_ptr(), 2, stream=stream)
    torch.cuda.synchronize()
    for P, o in ((Pa, oa), (Pb, ob)):
        for j in range(3):
            for i in range(2):
                one = torch.empty(shape, dtype=torch.float64, device="cuda")
                plan.apply(P[j], c, [f[i].data_ptr()], [one.data_ptr()], 1, device_ptrs=True, stream=stream)
                assert np.array_equal(o[j, i].cpu().numpy(), one.cpu().numpy(), equal_nan=True), (j, i)
    assert not np.array_equal(oa.cpu().numpy(), ob.cpu().numpy(), equal_nan=True)


# ---- 5. the C ABI's refusals -------------------------------------------------------------------------------------------------------------
def _status(fn, *a, **k):
    try:
        fn(*a, **k)
    except _lib.GcmfError as e:
        return e.status, e.message
    return _lib.OK, ""


def _planes(kind, gv, dt="f8"):
    return [np.ascontiguousarray(gv[k], dtype=dt) for k in ALL_KERNELS[GridType[kind]].required_grid_args()]


def test_c_abi_refusals(monkeypatch):
    import torch
    kind, shape = "IRREGULAR_WITH_LAND", SMALL
    ny, nx = shape
    gv = grid_vars(kind, shape)
    plan = plan_of(kind, shape)
    bank = make_bank(kind, shape, 24)
    P = np.stack([np.asarray(s.p) for s in bank.filter_specs])
    c = 2 / bank.filter_specs[0].s_max
    f = torch.from_numpy(field_for(shape, 750, (2,))).cuda()
    out = torch.empty((3, 2) + shape, dtype=torch.float64, device="cuda")
    src, dst = f.data_ptr(), out.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    before = torch.empty(shape, dtype=torch.float64, device="cuda")
    plan.apply(P[1], c, [f[0].data_ptr()], [before.data_ptr()], 1, device_ptrs=True, stream=stream)

    def refused(pl, why, *a, status=_lib.ERR_UNSUPPORTED, **k):
        st, msg = _status(pl.apply_bank, *a, **k)
        assert st == status and "gcmf_apply_bank" in msg and why in msg, (why, st, msg)

    # plans a bank does not run on
    g = T.scalar_grid_vars("REGULAR_WITH_LAND", shape)
    other = _lib.Plan(GridType.REGULAR_WITH_LAND.value, _lib.F64, ny, nx, _planes("REGULAR_WITH_LAND", g))
    refused(other, "another grid type", P, c, src, dst, 2)
    other.close()
    f32 = _lib.Plan(GridType[kind].value, _lib.F32, ny, nx, _planes(kind, gv, "f4"))
    refused(f32, "an f32 plan", P, c, src, dst, 2)
    f32.close()
    slab = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv), row_begin=0, row_end=ny // 2, halo=9)
    refused(slab, "a row slab", P, c, src, dst, 2)
    slab.close()
    ring = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv), self_ring=True, halo=9)
    refused(ring, "GCMF_PLAN_SELF_RING", P, c, src, dst, 2)
    ring.close()
    lev = [np.stack([a] * 2) if k == 0 else a for k, a in enumerate(_planes(kind, gv))]
    stacked = _lib.Plan.create_levels(GridType[kind].value, _lib.F64, ny, nx, lev, [2] + [1] * (len(lev) - 1), 2)
    refused(stacked, "a stacked plan", P, c, src, dst, 2)
    assert stacked.bank_cut(24, 6) == []
    stacked.close()
    # arguments and flags
    refused(plan, "host pointers", P, c, src, dst, 2, device_ptrs=False)
    for flag, name in [(_lib.FORWARD_RECURRENCE, "GCMF_FORWARD_RECURRENCE"), (_lib.MASK_FROM_NAN, "GCMF_MASK_FROM_NAN"),
                       (_lib.FACES_FROM_NAN, "GCMF_FACES_FROM_NAN"), (_lib.OUT_F32, "GCMF_OUT_F32")]:
        refused(plan, name, P, c, src, dst, 2, flags=flag)
    # no backward cut: fewer than five steps; nx no multiple of 4 on a grid with land; GCMF_CLENSHAW=0
    assert plan.bank_cut(4, 6) == [] and plan.bank_cut(24, 6) == [8, 8, 8]
    refused(plan, "fewer than five steps", P[:, :5], c, src, dst, 2)
    odd = (ny, nx + 2)
    godd = T.scalar_grid_vars(kind, odd)
    podd = _lib.Plan(GridType[kind].value, _lib.F64, odd[0], odd[1], _planes(kind, godd))
    assert (godd["wet_mask"] == 0).any() and podd.bank_cut(24, 6) == []
    fo = torch.zeros((2,) + odd, dtype=torch.float64, device="cuda")
    oo = torch.empty((3, 2) + odd, dtype=torch.float64, device="cuda")
    refused(podd, "not a multiple of 4", P, c, fo.data_ptr(), oo.data_ptr(), 2)
    podd.close()
    monkeypatch.setenv("GCMF_CLENSHAW", "0")
    off = _lib.Plan(GridType[kind].value, _lib.F64, ny, nx, _planes(kind, gv))
    monkeypatch.delenv("GCMF_CLENSHAW")
    assert off.bank_cut(24, 6) == []
    refused(off, "GCMF_CLENSHAW=0", P, c, src, dst, 2)
    off.close()
    # invalid arguments
    inv = dict(status=_lib.ERR_INVALID_ARG)
    refused(plan, "at least one polynomial", P[:0], c, src, dst, 2, **inv)
    refused(plan, "at least one step", P[:, :1], c, src, dst, 2, **inv)
    refused(plan, "null", P, c, 0, dst, 2, **inv)
    refused(plan, "null", P, c, src, 0, 2, **inv)
    refused(plan, "must not overlap", P, c, src, src, 2, **inv)
    refused(plan, "must not overlap", P, c, dst + 8 * ny * nx * 5, dst, 2, **inv)      # the input inside the output
    refused(plan, "must not overlap", P, c, src, src + 8 * ny * nx, 2, **inv)          # the output begins inside the input
    assert _status(plan.apply_bank, P, c, src, dst, 0) == (_lib.OK, "")
    torch.cuda.synchronize()
    # a real bank call, then gcmf_apply on the same plan: the bits it gave before (nothing of the bank stays behind)
    plan.apply_bank(P, c, src, dst, 2, stream=stream)
    assert plan.last_path() == "strips" and plan.last_timing()[1] == 3      # three strip launches
    after = torch.empty(shape, dtype=torch.float64, device="cuda")
    plan.apply(P[1], c, [f[0].data_ptr()], [after.data_ptr()], 1, device_ptrs=True, stream=stream)
    assert "bank" not in plan.last_kernel_geometry()
    assert np.array_equal(before.cpu().numpy(), after.cpu().numpy(), equal_nan=True)
    assert np.array_equal(out[1, 0].cpu().numpy(), after.cpu().numpy(), equal_nan=True)


# ---- 6. the loop route keeps the contract ---------------------------------------------------------------------------------------------------
def _per_scale(bank, *fields, vector=False):
    fl = [Filter(filter_scale=s, dx_min=bank.dx_min, filter_shape=bank.filter_shape, n_steps=bank.n_steps, grid_type=bank.grid_type,
                 grid_vars=bank.grid_vars, evaluation=bank.evaluation) for s in bank.filter_scales]
    if vector:
        res = [f.apply_to_vector(*fields) for f in fl]
        return np.stack([host(r[0]) for r in res]), np.stack([host(r[1]) for r in res])
    return np.stack([host(f.apply(*fields)) for f in fl])


def test_the_loop_route_keeps_the_contract(monkeypatch):
    shape = SMALL
    f = field_for(shape, 760, (2,))
    # a land-mask kind
    g = T.scalar_grid_vars("REGULAR_WITH_LAND", shape)
    bank = FilterBank(filter_scales=[2.0, 3.0, 4.5], dx_min=1.0, n_steps=24, grid_type=GridType.REGULAR_WITH_LAND, grid_vars=g)
    got = bank.apply(f)
    assert bank.last_route == "loop" and got.shape == (3, 2) + shape
    assert np.array_equal(got, _per_scale(bank, f), equal_nan=True)
    # float32 on a flux-form kind
    kind = "IRREGULAR_WITH_LAND"
    gv = grid_vars(kind, shape)
    g32 = {k: v.astype("f4") for k, v in gv.items()}
    bank = make_bank(kind, shape, 24, gv=g32)
    got = bank.apply(f.astype("f4"))
    assert bank.last_route == "loop" and got.shape == (3, 2) + shape and got.dtype == np.float64
    assert np.array_equal(got, _per_scale(bank, f.astype("f4")), equal_nan=True)
    # the forward recurrence
    bank = make_bank(kind, shape, 24, evaluation="reference")
    got = bank.apply(f)
    assert bank.last_route == "loop"
    assert np.array_equal(got, _per_scale(bank, f), equal_nan=True)
    check(got, oracle_of(bank, kind, f, gv), "evaluation=reference")
    # grid variables with a leading axis
    g3 = dict(gv, wet_mask=np.stack([gv["wet_mask"]] * 2))
    g3["wet_mask"][1, 60:64, 100:110] = 0
    bank = make_bank(kind, shape, 24, gv=g3)
    got = bank.apply(f)
    assert bank.last_route == "loop" and got.shape == (3, 2) + shape
    assert np.array_equal(got, _per_scale(bank, f), equal_nan=True)
    # one scale
    bank = make_bank(kind, shape, 24, (3.0,))
    got = bank.apply(f)
    assert bank.last_route == "loop" and got.shape == (1, 2) + shape
    assert np.array_equal(got, _per_scale(bank, f), equal_nan=True)
    # a vector Laplacian
    (u, v), gvec = T.vector_case("VECTOR_C_GRID", shape)
    dxv = T.grid_dx_min("VECTOR_C_GRID", gvec)
    bank = FilterBank(filter_scales=[2.0 * dxv, 3.0 * dxv], dx_min=dxv, n_steps=12,
                      grid_type=GridType.VECTOR_C_GRID, grid_vars=gvec)
    gu, gw = bank.apply_to_vector(u, v)
    assert bank.last_route == "loop" and gu.shape == gw.shape == (2,) + shape
    wu, wv = _per_scale(bank, u, v, vector=True)
    assert np.array_equal(gu, wu, equal_nan=True) and np.array_equal(gw, wv, equal_nan=True)
    # the switch, on a case the bank takes
    bank = make_bank(kind, shape, 24)
    fast = bank.apply(f)
    assert bank.last_route == "bank"
    monkeypatch.setenv("GCMF_FILTER_BANK", "0")
    slow = bank.apply(f)
    assert bank.last_route == "loop"
    assert np.array_equal(fast, slow, equal_nan=True)
    monkeypatch.setenv("GCMF_FILTER_BANK", "1")
    assert np.array_equal(bank.apply(f), fast, equal_nan=True) and bank.last_route == "bank"


# ---- 7. xarray -----------------------------------------------------------------------------------------------------------------------------
def test_xarray_dataarray(monkeypatch):
    from conftest import xarray_backend
    xr = xarray_backend("model", monkeypatch)
    kind, shape = "MOM5U", SMALL
    gv = grid_vars(kind, shape)
    gvx = {k: xr.DataArray(v, dims=["y", "x"]) for k, v in gv.items()}
    bank = make_bank(kind, shape, 24, gv=gvx)
    f = field_for(shape, 770, (3,))
    out = bank.apply(xr.DataArray(f, dims=["time", "y", "x"]), dims=["y", "x"])
    assert bank.last_route == "bank"
    assert tuple(out.dims) == ("time", "filter_scale", "y", "x") and out.data.shape == (3, 3) + shape
    want = loop_of(make_bank(kind, shape, 24), f)
    assert np.array_equal(np.moveaxis(np.asarray(out.data), 1, 0), want, equal_nan=True)
    # core dims anywhere in the input: moved to the end, the scales directly before them
    out = bank.apply(xr.DataArray(np.ascontiguousarray(f.transpose(1, 0, 2)), dims=["y", "time", "x"]), dims=["y", "x"])
    assert tuple(out.dims) == ("time", "filter_scale", "y", "x")
    assert np.array_equal(np.moveaxis(np.asarray(out.data), 1, 0), want, equal_nan=True)
    with pytest.raises(TypeError, match="one by one"):
        bank.apply(xr.Dataset(data_vars=dict(a=(("y", "x"), f[0]))), dims=["y", "x"])
