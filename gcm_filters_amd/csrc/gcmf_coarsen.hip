// gcmf_coarsen_weights / gcmf_apply_coarsen (include/gcmf.h): the filter followed by weighted block means of its result, on the device.
//
// The pass is one streaming launch behind the schedule -- a further form of k_prepare, the name of the plane passes that run before and
// after a schedule (gcmf_scalar.hip has the copy / area form and the adjoint's two scalings), on its own parameter struct.  It reads
// the fine f64 plane and the weight plane once and writes one value per block; the rule and the order of the sums are those of
// gcmf_coarsen.hpp, which the host restatement coarsen_plane shares.
//
// Mapping to the hardware (bandwidth-bound):
//   * a workgroup of 256 threads owns the fine rows of ONE coarse row and a run of whole coarse cells along x; a thread owns VEC
//     neighbouring fine columns (VEC = 2: one 16-byte load per plane and row, 4 KiB fully coalesced per wave instruction; VEC = 1 where
//     nx is odd or a plane of the call is not on a 16-byte boundary) and marches north over the fy rows, summing each COLUMN in
//     registers -- so a 16-byte pair that straddles two blocks needs nothing special: its two columns simply belong to different cells;
//   * the column sums go to LDS, and one thread per coarse cell adds its fx columns from west to east;
//   * a block wider than a workgroup's columns (fx > 256 VEC - 1) is one workgroup's: it walks the block in chunks of 256 VEC columns, and
//     thread 0 carries the west-to-east sum from chunk to chunk.  Its parallelism is the number of coarse cells: (ny, nx) itself, one
//     block per entry, runs on as many workgroups as the call has entries.
//   * blockIdx.y is the entry; entry y reads weight level (lev0 + y) % nlev.
// No atomics: every sum has one owner and one order.
#include "gcmf_internal.hpp"
#include "gcmf_coarsen.hpp"

#include <cstring>

namespace gcmf {

struct CoarsenP {
  const double *fine;     // (entries, ny, nx)
  const double *w;        // (nlev, ny, nx); nullptr: every weight is 1
  double *coarse;         // (entries, cy, cx)
  double *wsum;           // the same shape, or nullptr
  int ny, nx, fy, fx, cy, cx;
  int cpt;                // coarse cells per workgroup along x (0: one cell, walked in chunks)
  int ntx;                // workgroups per coarse row
  int nlev, lev0;
};

constexpr int COARSEN_THREADS = 256;

template <int VEC> struct CoarsenLoad;
template <> struct CoarsenLoad<1> {
  static __device__ __forceinline__ void get(double (&d)[1], const double *p) { d[0] = *p; }
};
template <> struct CoarsenLoad<2> {
  static __device__ __forceinline__ void get(double (&d)[2], const double *p) {
    const double2 v = *reinterpret_cast<const double2 *>(p);
    d[0] = v.x;
    d[1] = v.y;
  }
};

template <int VEC>
__global__ __launch_bounds__(COARSEN_THREADS) void k_prepare(const CoarsenP P) {
  constexpr int TW = COARSEN_THREADS * VEC;   // fine columns of one chunk
  __shared__ double colp[TW], colw[TW];
  const int t = threadIdx.x;
  const int J = blockIdx.x / P.ntx, tx = blockIdx.x - J * P.ntx;
  const int y = blockIdx.y;
  const long long plane = (long long)P.ny * P.nx;
  const double *__restrict__ fine = P.fine + (long long)y * plane;
  const double *__restrict__ w = P.w ? P.w + (long long)((P.lev0 + y) % P.nlev) * plane : nullptr;
  // the workgroup's coarse cells [I0, I1) and fine columns [x0, x1)
  const int I0 = P.cpt ? tx * P.cpt : tx;
  const int I1 = P.cpt ? min(P.cx, I0 + P.cpt) : I0 + 1;
  const int x0 = I0 * P.fx, x1 = I1 * P.fx;
  const int j0 = J * P.fy, j1 = j0 + P.fy;
  double runp = 0.0, runw = 0.0;   // (one cell walked in chunks: thread 0's west-to-east sums)
  for (int a0 = x0 - x0 % VEC; a0 < x1; a0 += TW) {   // (a0: a multiple of VEC, so every pair below lies on a 16-byte boundary)
    const int c = a0 + t * VEC;                       // the thread's first column
    const bool active = c < x1 && c + VEC > x0;       // (x1 <= nx and VEC divides nx: an active pair ends inside its row)
    double cp[VEC], cw[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) cp[k] = cw[k] = 0.0;
    if (active) {
      const double *fr = fine + (long long)j0 * P.nx + c;
      const double *wr = w ? w + (long long)j0 * P.nx + c : nullptr;
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        double fv[VEC], wv[VEC];
        CoarsenLoad<VEC>::get(fv, fr);
        if (wr) {
          CoarsenLoad<VEC>::get(wv, wr);
          wr += P.nx;
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) wv[k] = 1.0;
        }
        fr += P.nx;
#pragma unroll
        for (int k = 0; k < VEC; ++k) coarsen_term(wv[k], fv[k], cp[k], cw[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      colp[t * VEC + k] = cp[k];
      colw[t * VEC + k] = cw[k];
    }
    __syncthreads();
    if (P.cpt) {   // whole cells in one chunk: a thread per cell
      for (int I = I0 + t; I < I1; I += COARSEN_THREADS) {
        double sp = 0.0, sw = 0.0;
        for (int i = I * P.fx - a0; i < (I + 1) * P.fx - a0; ++i) {
          sp = sp + colp[i];
          sw = sw + colw[i];
        }
        const long long Q = ((long long)y * P.cy + J) * P.cx + I;
        P.coarse[Q] = coarsen_mean(sp, sw);
        if (P.wsum) P.wsum[Q] = sw;
      }
    } else {
      if (t == 0) {
        const int lo = max(x0, a0) - a0, hi = min(x1, a0 + TW) - a0;
        for (int i = lo; i < hi; ++i) {
          runp = runp + colp[i];
          runw = runw + colw[i];
        }
      }
      __syncthreads();   // (the next chunk overwrites the columns)
    }
  }
  if (!P.cpt && t == 0) {
    const long long Q = ((long long)y * P.cy + J) * P.cx + I0;
    P.coarse[Q] = coarsen_mean(runp, runw);
    if (P.wsum) P.wsum[Q] = runw;
  }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// fine: (nent, ny, nx) f64 on the device; coarse / wsum: (nent, ny / fy, nx / fx); entry y takes weight level (lev0 + y) % nlev
static int launch_coarsen(const gcmf_plan *pl, const double *fine, double *coarse, double *wsum, int64_t nent, int fy, int fx, int64_t lev0,
                          hipStream_t s) {
  if (nent <= 0) return GCMF_OK;
  CoarsenP P{};
  P.fine = fine;
  P.w = (const double *)pl->coarsen_w;
  P.coarse = coarse;
  P.wsum = wsum;
  P.ny = (int)pl->d.ny;
  P.nx = (int)pl->d.nx;
  P.fy = fy;
  P.fx = fx;
  P.cy = P.ny / fy;
  P.cx = P.nx / fx;
  P.nlev = (int)std::max<int64_t>(1, pl->coarsen_nlev);
  P.lev0 = (int)(lev0 % P.nlev);
  // 16-byte pairs: every row, entry and level then starts on a 16-byte boundary (nx even) if the planes do
  const bool vec_ok = P.nx % 2 == 0 && aligned16(P.fine) && aligned16(P.w);
  const int V = vec_ok ? 2 : 1, TW = COARSEN_THREADS * V;
  // (a workgroup's first pair may begin one column west of its first cell: V - 1 columns of the chunk are kept for that)
  P.cpt = fx <= TW - (V - 1) ? (TW - (V - 1)) / fx : 0;
  P.ntx = P.cpt ? (P.cx + P.cpt - 1) / P.cpt : P.cx;
  dim3 block(COARSEN_THREADS), grid((unsigned)((long long)P.cy * P.ntx), (unsigned)nent);
  if (vec_ok)
    hipLaunchKernelGGL((k_prepare<2>), grid, block, 0, s, P);
  else
    hipLaunchKernelGGL((k_prepare<1>), grid, block, 0, s, P);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

}  // namespace gcmf

using namespace gcmf;

extern "C" {

int gcmf_coarsen_weights(gcmf_plan *pl, const void *w, int64_t nlev, uint32_t flags) {
  if (!pl) {
    set_error("gcmf_coarsen_weights: `plan` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  if (w && nlev < 1) {
    set_error("gcmf_coarsen_weights: `nlev` must be at least 1, not %lld", (long long)nlev);
    return GCMF_ERR_INVALID_ARG;
  }
  if (flags & ~(uint32_t)GCMF_DEVICE_PTRS) {
    set_error("gcmf_coarsen_weights: `flags` takes GCMF_DEVICE_PTRS only, not 0x%x", flags);
    return GCMF_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> outer(pl->coarsen_mu);
  std::lock_guard<std::mutex> lk(pl->mu);
  GCMF_HIP(hipSetDevice(pl->d.device));
  GCMF_HIP(hipDeviceSynchronize());   // a pass of an earlier call may still be reading the planes that go
  if (pl->coarsen_w) GCMF_HIP(hipFree(pl->coarsen_w));
  pl->coarsen_w = nullptr;
  pl->coarsen_nlev = 0;
  if (!w) return GCMF_OK;
  const size_t bytes = (size_t)nlev * (size_t)pl->d.ny * (size_t)pl->d.nx * sizeof(double);
  void *dev = nullptr;
  GCMF_HIP(hipMalloc(&dev, bytes));
  const hipError_t e = hipMemcpy(dev, w, bytes, (flags & GCMF_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(dev);
    set_error("gcmf_coarsen_weights: copying %zu bytes of weights failed: %s", bytes, hipGetErrorString(e));
    return GCMF_ERR_HIP;
  }
  pl->coarsen_w = dev;
  pl->coarsen_nlev = nlev;
  return GCMF_OK;
}

int gcmf_apply_coarsen(gcmf_plan *pl, const double *p, int n_steps, double c, const void *const *in, void *const *out, void *const *wsum,
                       int64_t nbatch, int fy, int fx, uint32_t flags, void *stream) {
  if (!pl) {
    set_error("gcmf_apply_coarsen: `plan` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  const char *limit = pl->ncomp == 2 ? "vector plans (ncomp == 2) are not coarsened: scalar grid types only" :
                      (pl->d.flags & GCMF_PLAN_SELF_RING) ? "not available on a GCMF_PLAN_SELF_RING plan" :
                      !pl->full ? "not available on a row slab: it needs a plan covering the whole grid" :
                      (flags & GCMF_OUT_F32) ? "GCMF_OUT_F32 is not taken: the coarse planes are always f64" : nullptr;
  if (limit) {
    set_error("gcmf_apply_coarsen: %s (grid type %d)", limit, pl->d.grid_type);
    return GCMF_ERR_UNSUPPORTED;
  }
  const int64_t ny = pl->d.ny, nx = pl->d.nx;
  if (fy < 1 || ny % fy) {
    set_error("gcmf_apply_coarsen: `fy` = %d must be positive and divide ny = %lld", fy, (long long)ny);
    return GCMF_ERR_INVALID_ARG;
  }
  if (fx < 1 || nx % fx) {
    set_error("gcmf_apply_coarsen: `fx` = %d must be positive and divide nx = %lld", fx, (long long)nx);
    return GCMF_ERR_INVALID_ARG;
  }
  if (!in || !in[0]) {
    set_error("gcmf_apply_coarsen: `in` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  if (!out || !out[0]) {
    set_error("gcmf_apply_coarsen: `out` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  if (wsum && !wsum[0]) {
    set_error("gcmf_apply_coarsen: `wsum` is given but wsum[0] is null (pass wsum = NULL for no sums)");
    return GCMF_ERR_INVALID_ARG;
  }
  if (nbatch < 0) {
    set_error("gcmf_apply_coarsen: `nbatch` = %lld is negative", (long long)nbatch);
    return GCMF_ERR_INVALID_ARG;
  }
  if (!p || n_steps < 1) {
    set_error("gcmf_apply_coarsen: `p` is null or `n_steps` = %d is below 1", n_steps);
    return GCMF_ERR_INVALID_ARG;
  }
  const size_t ts = dtype_size(pl->d.dtype);
  const size_t cell = (size_t)ny * (size_t)nx, ccell = (size_t)(ny / fy) * (size_t)(nx / fx);
  const size_t in_bytes = (size_t)nbatch * cell * ts, out_bytes = (size_t)nbatch * ccell * sizeof(double);
  const char *a = nullptr, *b = nullptr;
  if (ranges_overlap(out[0], out_bytes, in[0], in_bytes)) a = "out", b = "in";
  else if (wsum && ranges_overlap(wsum[0], out_bytes, in[0], in_bytes)) a = "wsum", b = "in";
  else if (wsum && ranges_overlap(wsum[0], out_bytes, out[0], out_bytes)) a = "wsum", b = "out";
  if (a) {
    set_error("gcmf_apply_coarsen: `%s` must not overlap `%s` as byte ranges (%zu bytes of coarse planes, %zu bytes of input)", a, b, out_bytes,
              in_bytes);
    return GCMF_ERR_INVALID_ARG;
  }
  if (pl->stacked && nbatch % pl->nlev) {
    set_error("gcmf_apply_coarsen: a stacked plan of %lld levels takes an `nbatch` that is a multiple of it (entry b runs on level b %% nlev), "
              "not %lld", (long long)pl->nlev, (long long)nbatch);
    return GCMF_ERR_INVALID_ARG;
  }
  if (nbatch == 0) return GCMF_OK;

  std::lock_guard<std::mutex> outer(pl->coarsen_mu);   // (gcmf_apply takes the plan's mutex itself, run by run)
  GCMF_HIP(hipSetDevice(pl->d.device));
  const bool on_dev = flags & GCMF_DEVICE_PTRS;
  hipStream_t s = (on_dev || stream) ? (hipStream_t)stream : pl->stream;
  // a run: as many entries as keep the fine planes at or under "coarsen_scratch_mb" -- at least one, a stacked plan's in whole sets of
  // levels (gcmf_apply runs entry b of ITS batch on level b % nlev), and no more than one launch's gridDim.y takes
  const long long bound = (long long)std::max(0, pl->coarsen_scratch_mb) << 20;
  int64_t run_nb = std::max<int64_t>(1, std::min<int64_t>(32768, bound / (long long)(cell * sizeof(double))));
  if (pl->stacked) run_nb = std::max<int64_t>(pl->nlev, run_nb / pl->nlev * pl->nlev);
  run_nb = std::min(run_nb, nbatch);
  const size_t szF = up256((size_t)run_nb * cell * sizeof(double)), szI = on_dev ? 0 : up256((size_t)run_nb * cell * ts);
  const size_t szC = on_dev ? 0 : up256((size_t)run_nb * ccell * sizeof(double));
  const size_t need = szF + szI + 2 * szC;
  int rc;
  if ((rc = order_behind_last_call(pl, s))) return rc;
  if (need > pl->coarsen_bytes) {
    if (pl->coarsen_buf) GCMF_HIP(hipFree(pl->coarsen_buf));   // (synchronises the device: nothing reads the old block any more)
    pl->coarsen_buf = nullptr;
    pl->coarsen_bytes = 0;
    GCMF_HIP(hipMalloc(&pl->coarsen_buf, need));
    pl->coarsen_bytes = need;
  }
  char *base = (char *)pl->coarsen_buf;
  double *fine = (double *)base;
  char *din = base + szF;
  double *dco = (double *)(base + szF + szI), *dws = (double *)(base + szF + szI + szC);
  float ms = 0.f;
  int launches = 0;
  for (int64_t e0 = 0; e0 < nbatch; e0 += run_nb) {
    const int64_t nb = std::min(run_nb, nbatch - e0);
    const void *in1[2] = {(const char *)in[0] + (size_t)e0 * cell * ts, nullptr};
    void *fine1[2] = {fine, nullptr};
    double *co = (double *)out[0] + (size_t)e0 * ccell, *ws = wsum ? (double *)wsum[0] + (size_t)e0 * ccell : nullptr;
    if (!on_dev) {
      GCMF_HIP(hipMemcpyAsync(din, in1[0], (size_t)nb * cell * ts, hipMemcpyHostToDevice, s));
      in1[0] = din;
    }
    if ((rc = gcmf_apply(pl, p, n_steps, c, in1, fine1, nb, flags | GCMF_DEVICE_PTRS, (void *)s))) return rc;
    if ((rc = launch_coarsen(pl, fine, on_dev ? co : dco, wsum ? (on_dev ? ws : dws) : nullptr, nb, fy, fx, e0, s))) return rc;
    {
      std::lock_guard<std::mutex> lk(pl->mu);
      ms += pl->last_ms;
      launches += pl->last_launches + 1;
      // (gcmf_apply has put its event behind ITS launches where the stream is a caller's that may go away: behind the pass as well)
      if (pl->busy_recorded) GCMF_HIP(hipEventRecord(pl->ev_busy, s));
    }
    if (!on_dev) {
      GCMF_HIP(hipMemcpyAsync(co, dco, (size_t)nb * ccell * sizeof(double), hipMemcpyDeviceToHost, s));
      if (ws) GCMF_HIP(hipMemcpyAsync(ws, dws, (size_t)nb * ccell * sizeof(double), hipMemcpyDeviceToHost, s));
      GCMF_HIP(hipStreamSynchronize(s));
      std::lock_guard<std::mutex> lk(pl->mu);
      const unsigned rlo = pl->res_lo, rhi = pl->res_hi;
      pl->res_lo = pl->res_hi = 0;   // (the stream is drained: the synchronising host route can tell for THIS call, as gcmf_apply's does)
      if (rlo && resident_take_failure(pl->d.device, rlo, rhi)) {
        set_error("gcmf_apply_coarsen: the on-chip launch (k_resident) timed out waiting for a neighbour tile: the result is NaN; the "
                  "strip-marching launches are used from now on");
        return GCMF_ERR_HIP;
      }
    }
  }
  std::lock_guard<std::mutex> lk(pl->mu);
  pl->last_ms = ms;
  pl->last_launches = launches;
  return GCMF_OK;
}

}  // extern "C"
