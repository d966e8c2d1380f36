"""The Python call path below `Filter.apply` (no GPU needed): `CallOptions`, the one value that carries a call's options from the filter
factories to the library binding; the staging helper of fields and `like`; the binding's shared flag word.  That the calls compute the
same bits as before is a GPU matter: tools/call_path_digest.py, profiles/call_options/."""
import itertools

import numpy as np
import pytest

from gcm_filters_amd import GridType, _lib
from gcm_filters_amd import filter as F
from gcm_filters_amd import kernels as K
from gcm_filters_amd.kernels import ALL_KERNELS, CallOptions

FLAGS = ("out_f32", "forward", "backward_f32", "mask_from_nan", "faces_from_nan", "adjoint")


def test_defaults_and_immutability():
    opts = CallOptions()
    assert opts == (None, False, False, False, False, False, False) and opts._fields == ("spec",) + FLAGS
    with pytest.raises(AttributeError):
        opts.forward = True
    assert opts.plain
    for name in FLAGS[1:]:
        assert not CallOptions(**{name: True}).plain, name
    assert CallOptions(spec=object(), out_f32=True).plain      # (the result's dtype is no route)
    gaps = CallOptions(spec="s", forward=True, faces_from_nan=True, adjoint=True)
    assert gaps.without_faces() == CallOptions(spec="s", forward=True, adjoint=True) and gaps.faces_from_nan


@pytest.mark.parametrize("bits", list(itertools.product((False, True), repeat=6)))
def test_flag_word(bits):
    device_ptrs, out_f32, forward, backward_f32, mask_from_nan, faces_from_nan = bits
    want = 0
    if device_ptrs:
        want |= _lib.DEVICE_PTRS
    if out_f32:
        want |= _lib.OUT_F32
    if forward:
        want |= _lib.FORWARD_RECURRENCE
    if backward_f32:
        want |= _lib.BACKWARD_F32
    if mask_from_nan:
        want |= _lib.MASK_FROM_NAN
    if faces_from_nan:
        want |= _lib.FACES_FROM_NAN
    assert _lib.apply_flags(*bits) == want
    assert (_lib.DEVICE_PTRS, _lib.OUT_F32, _lib.FORWARD_RECURRENCE, _lib.BACKWARD_F32, _lib.MASK_FROM_NAN, _lib.FACES_FROM_NAN) \
        == (0x1, 0x2, 0x4, 0x10, 0x20, 0x40)


def _stubbed(grid="REGULAR"):
    """A Laplacian without a plan whose _run_with records what reaches it."""
    lap = object.__new__(ALL_KERNELS[GridType[grid]])
    lap.seen = []
    lap._run_with = lambda fields, opts, like=None: lap.seen.append((fields, opts, like)) or "result"
    return lap


ALL_TOGETHER = dict(spec="spec", out_f32=True, forward=True, backward_f32=True, mask_from_nan=True, faces_from_nan=True, adjoint=True,
                    like=["like"])


@pytest.mark.parametrize("kw", [{}] + [{k: v} for k, v in ALL_TOGETHER.items()] + [ALL_TOGETHER], ids=lambda kw: "+".join(kw) or "none")
def test_run_hands_its_keywords_on_as_one_value(kw):
    lap, fields = _stubbed(), [np.zeros((4, 4))]
    assert lap._run(fields, **kw) == "result"
    (got_fields, opts, like), = lap.seen
    assert got_fields is fields and type(opts) is CallOptions
    assert opts == CallOptions(**{k: v for k, v in kw.items() if k != "like"})
    assert like is kw.get("like")


def test_check_raises_what_run_raised():
    spec = object()
    with pytest.raises(ValueError, match="needs `like`"):
        CallOptions(spec=spec, mask_from_nan=True, adjoint=True).check(GridType.REGULAR_WITH_LAND, False)
    with pytest.raises(ValueError, match="needs `like`"):
        CallOptions(spec=spec, faces_from_nan=True, adjoint=True).check(GridType.MOM5U, False)
    CallOptions(spec=spec, mask_from_nan=True, adjoint=True).check(GridType.REGULAR_WITH_LAND, True)
    CallOptions(spec=spec, faces_from_nan=True, adjoint=True).check(GridType.MOM5U, True)
    with pytest.raises(ValueError, match="adjoint needs a filter application"):
        CallOptions(adjoint=True).check(GridType.REGULAR_WITH_LAND, False)
    with pytest.raises(NotImplementedError, match="symmetrizer"):
        CallOptions(spec=spec, adjoint=True).check(GridType.VECTOR_B_GRID, False)
    with pytest.raises(ValueError, match="IRREGULAR_WITH_LAND, MOM5U, MOM5T"):
        CallOptions(spec=spec, faces_from_nan=True).check(GridType.REGULAR, False)
    with pytest.raises(ValueError, match=r"faces_from_nan needs a filter application \(without mask_from_nan\)"):
        CallOptions(spec=spec, faces_from_nan=True, mask_from_nan=True).check(GridType.REGULAR_WITH_LAND, False)
    with pytest.raises(ValueError, match="faces_from_nan needs a filter application"):
        CallOptions(faces_from_nan=True).check(GridType.MOM5T, False)
    with pytest.raises(ValueError, match="mask_from_nan needs a filter application on one of the grid types REGULAR_WITH_LAND, "
                                         "REGULAR_WITH_LAND_AREA_WEIGHTED, TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED"):
        CallOptions(spec=spec, mask_from_nan=True).check(GridType.IRREGULAR_WITH_LAND, False)
    with pytest.raises(ValueError, match="mask_from_nan needs a filter application"):
        CallOptions(mask_from_nan=True).check(GridType.REGULAR_WITH_LAND, False)
    for grid in GridType:      # one Laplacian, every flag off: any grid type takes it
        CallOptions().check(grid, False)
        CallOptions(spec=spec).check(grid, False)


def test_the_driver_checks_before_it_touches_the_laplacian():
    """(the Laplacians here have no planes, no plan: only the check can have run)"""
    lap = object.__new__(ALL_KERNELS[GridType.REGULAR])
    with pytest.raises(ValueError, match="IRREGULAR_WITH_LAND, MOM5U, MOM5T"):
        lap._run_with([np.zeros((8, 8))], CallOptions(spec=object(), faces_from_nan=True))
    lap = object.__new__(ALL_KERNELS[GridType.REGULAR_WITH_LAND])
    with pytest.raises(ValueError, match="needs `like`"):
        lap._run_with([np.zeros((8, 8))], CallOptions(spec=object(), mask_from_nan=True, adjoint=True), None)


def test_shift_and_coefficients():
    spec = F.FilterSpec(n_steps=3, s_max=8, p=[1, 0.5, 0.25, 0.125], dx_min_sq=0.25)
    opts = CallOptions(spec=spec)
    assert opts.shift(True) == 2 / 8
    assert opts.shift(False) == 2 / (8 * 0.25)
    p = opts.p
    assert p.dtype == np.float64 and p.flags.c_contiguous and p.tolist() == [1, 0.5, 0.25, 0.125]


def test_staging_on_the_host():
    a = np.arange(48, dtype=np.float64).reshape(6, 8)
    out, temporary = K._stage(a, _lib.F64)
    assert out is a and not temporary
    for src in (a.astype(np.float32), np.asfortranarray(a), np.arange(96, dtype=np.float64).reshape(6, 16)[:, ::2]):
        out, temporary = K._stage(src, _lib.F64)
        assert temporary and out is not src and out.dtype == np.float64 and out.flags.c_contiguous
        assert np.array_equal(out, src)
    out, temporary = K._stage(a, _lib.F32)
    assert temporary and out.dtype == np.float32 and np.array_equal(out, a.astype(np.float32))
    full = (2, 3, 6, 8)
    for src in (np.arange(144, dtype=np.float64).reshape(3, 6, 8), a):
        out, temporary = K._stage(src, _lib.F64, None, full)
        assert temporary and out.shape == full and out.dtype == np.float64 and out.flags.c_contiguous
        assert np.array_equal(out, np.broadcast_to(src, full))
    whole = np.zeros(full)
    out, temporary = K._stage(whole, _lib.F64, None, full)      # nothing to broadcast: passed through
    assert out is whole and not temporary


def test_staging_a_torch_host_tensor_gives_numpy():
    torch = pytest.importorskip("torch")
    t = torch.arange(48, dtype=torch.float32).reshape(6, 8)
    out, temporary = K._stage(t, _lib.F64)
    assert isinstance(out, np.ndarray) and temporary and out.dtype == np.float64 and np.array_equal(out, t.numpy())
    out, _ = K._stage(t.requires_grad_(False).double(), _lib.F64, None, (2, 6, 8))
    assert isinstance(out, np.ndarray) and out.shape == (2, 6, 8)


def test_staging_for_a_torch_device():
    """The rules of the device branch, on the one torch device there is without a GPU."""
    torch = pytest.importorskip("torch")
    cpu = torch.device("cpu")
    d = torch.arange(48, dtype=torch.float64).reshape(6, 8)
    out, temporary = K._stage(d, _lib.F64, cpu)
    assert out is d and not temporary
    for src in (d.float(), d.t().contiguous().t(), torch.arange(96, dtype=torch.float64).reshape(6, 16)[:, ::2]):
        out, temporary = K._stage(src, _lib.F64, cpu)
        assert temporary and out.dtype == torch.float64 and out.is_contiguous() and torch.equal(out, src.double())
    out, temporary = K._stage(np.ones((6, 8), dtype=np.float32), _lib.F64, cpu)      # a numpy `like` beside device fields
    assert temporary and torch.is_tensor(out) and out.dtype == torch.float64 and out.shape == (6, 8)
    out, temporary = K._stage(d, _lib.F64, cpu, (2, 3, 6, 8))
    assert temporary and out.shape == (2, 3, 6, 8) and out.is_contiguous() and torch.equal(out[1, 2], d)


class _Recorder:
    def __init__(self):
        self.calls = []

    def _run_with(self, fields, opts, like=None):
        self.calls.append((opts, like))
        return list(fields)


def test_the_factories_build_their_options_once(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(F._LaplacianMemo, "get", lambda self, args: rec)
    spec = F.FilterSpec(n_steps=3, s_max=8, p=[1, 0.5, 0.25, 0.125], dx_min_sq=1.0)
    x = np.zeros((4, 4))
    func = F._create_filter_func(spec, ALL_KERNELS[GridType.REGULAR], evaluation="backward")
    monkeypatch.setattr(K._PATH, "last", "strips", raising=False)
    assert func.last_path is None
    assert func(x) is x and func(x) is x
    assert func.last_path == "strips"
    assert func.adjoint(x) is x and func.adjoint_like(x, x) is x
    (fwd, l0), (fwd2, l1), (adj, l2), (adj2, l3) = rec.calls
    assert fwd is fwd2 and adj is adj2 and type(fwd) is CallOptions
    assert fwd == CallOptions(spec=spec, backward_f32=True) and adj == fwd._replace(adjoint=True) and not fwd.adjoint
    assert l0 is None and l1 is None and l2 is None and l3[0] is x
    # the flags of nan_mask, and the vector factory
    del rec.calls[:]
    F._create_filter_func(spec, ALL_KERNELS[GridType.REGULAR], evaluation="reference", nan_mask=True)(x)
    F._create_filter_func(spec, ALL_KERNELS[GridType.REGULAR], nan_mask="auto")(x)
    vec = F._create_filter_func_vec(spec, ALL_KERNELS[GridType.REGULAR])
    for out in (vec(x, x), vec.adjoint(x, x), vec(x, x)):
        assert isinstance(out, tuple) and len(out) == 2 and out[0] is x and out[1] is x
    opts = [c[0] for c in rec.calls]
    assert opts[0] == CallOptions(spec=spec, forward=True, mask_from_nan=True)
    assert opts[1] == CallOptions(spec=spec, mask_from_nan=True)       # ("auto" folds faces on the flux-form kinds only)
    assert opts[2] is opts[4] and opts[2] == CallOptions(spec=spec)
    assert opts[3] == CallOptions(spec=spec, adjoint=True)
    flux = F._create_filter_func(spec, ALL_KERNELS[GridType.MOM5U], nan_mask="auto")
    flux(x, *[None] * 6)
    assert rec.calls[-1][0] == CallOptions(spec=spec, faces_from_nan=True)
