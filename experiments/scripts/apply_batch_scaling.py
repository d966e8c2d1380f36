"""gcmf_apply per entry against the batch size: n_steps 63, 2400 x 3600 f64 IRREGULAR_WITH_LAND, device pointers, median of three blocks of
two calls.  Written to explain gcmf_apply_cov's 16-pair figure: batches of 6, 12 and 30 entries cost 1.1-1.2 ms per
entry where 3, 4, 8, 16 and 48 cost 0.67-0.69.
    python experiments/scripts/apply_batch_scaling.py"""
import os, sys, statistics, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("GCMF_RESIDENT", "0")
import numpy as np, torch
from gcm_filters_amd import Filter, FilterShape, GridType, _lib, testing as T
from gcm_filters_amd.kernels import ALL_KERNELS, CallOptions
KIND, SHAPE = "IRREGULAR_WITH_LAND", T.BASELINE_SHAPE
gv = T.scalar_grid_vars(KIND, SHAPE); gv["kappa_w"] = T.smooth_kappa(SHAPE, 11)
dx = T.grid_dx_min(KIND, gv)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    flt = Filter(filter_scale=8.0 * dx, dx_min=dx, filter_shape=FilterShape.TAPER, n_steps=63, grid_type=GridType[KIND], grid_vars=gv)
plan = ALL_KERNELS[GridType[KIND]](**gv)._plan(_lib.F64, SHAPE)
p, c = np.asarray(flt.filter_spec.p, dtype=np.float64), CallOptions(spec=flt.filter_spec).shift(False)
stream = torch.cuda.current_stream().cuda_stream
x = torch.rand((48,) + SHAPE, dtype=torch.float64, device="cuda"); out = torch.empty_like(x)
for nb in (1, 2, 3, 4, 6, 8, 12, 16, 18, 24, 30, 32, 48, 3, 1):
    fn = lambda: plan.apply(p, c, [x.data_ptr()], [out.data_ptr()], nb, device_ptrs=True, stream=stream)
    fn(); fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); fn(); e1.record(); e1.synchronize(); ms.append(e0.elapsed_time(e1) / 2)
    print(f"nbatch {nb:3d}: {statistics.median(ms):8.3f} ms = {statistics.median(ms) / nb:6.3f} ms per entry   kernel {plan.last_kernel()}", flush=True)
