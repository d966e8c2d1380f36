// gcmf_apply_cov (include/gcmf.h): the subfilter covariance tau(f, g) = F(f g) - F(f) F(g) of pairs of fields, on the device.
//
// A run of N pairs is ONE gcmf_apply on the batch [f'_0 .. f'_{N-1} | g'_0 .. | fg_0 ..] between two streaming launches -- further forms
// of k_prepare, the name of the plane passes that run before and after a schedule (gcmf_scalar.hip has the copy / area form and the
// adjoint's two scalings, gcmf_coarsen.hip the block means), each on its own parameter struct.  The cell rules are those of gcmf_cov.hpp,
// which the host restatements cov_pre_plane / cov_post_plane share.
//
// Mapping to the hardware (both passes are bandwidth-bound maps, cell by cell):
//   * 256 threads per workgroup; blockIdx.y is the pair; gridDim.x is capped and a workgroup strides over its pair's cells;
//   * a thread owns VEC neighbouring cells of every plane (VEC = 2: one 16-byte load or store per plane, 4 KiB fully coalesced per wave
//     instruction; VEC = 1 where ny * nx is odd or a plane of the call is not on a 16-byte boundary) -- the same arithmetic per cell
//     either way, so the same bits;
//   * plain loads and stores: the pre pass's planes are re-read at once by the schedule's first launch, and nothing measured backs
//     another flavour for the post pass.
// No atomics, no LDS: every cell has one owner.
#include "gcmf_internal.hpp"
#include "gcmf_cov.hpp"

namespace gcmf {

// pair y reads f + y * cell (and g + y * cell) and writes fo / go / fg + y * cell
struct CovPreP {
  const double *f, *g;   // g == nullptr: the variance form (g = f, no go plane)
  double *fo, *go, *fg;  // fo / go may BE f / g (host route: the fields were uploaded into their slots)
  long long cell;        // ny * nx
  int common;            // the common gaps of the rule
  int wr;                // write fo (and go): 0 where they are f (and g) in place and the gaps are off
};
// pair y reads a, b (and c) + y * cell and writes out + y * cell
struct CovPostP {
  const double *a, *b, *c;   // F(fg), F(f'), F(g'); c == nullptr: the variance form (c = b)
  double *out;
  long long cell;
};

constexpr int COV_THREADS = 256;

template <int VEC> struct CovIO;
template <> struct CovIO<1> {
  static __device__ __forceinline__ void get(double (&d)[1], const double *p) { d[0] = *p; }
  static __device__ __forceinline__ void put(double *p, const double (&d)[1]) { *p = d[0]; }
};
template <> struct CovIO<2> {
  static __device__ __forceinline__ void get(double (&d)[2], const double *p) {
    const double2 v = *reinterpret_cast<const double2 *>(p);
    d[0] = v.x;
    d[1] = v.y;
  }
  static __device__ __forceinline__ void put(double *p, const double (&d)[2]) { *reinterpret_cast<double2 *>(p) = make_double2(d[0], d[1]); }
};

// the pre pass: f, g -> f', g', f' g'   (VEC divides cell: a thread's cells end inside the pair's plane)
template <int VEC>
__global__ __launch_bounds__(COV_THREADS) void k_prepare(const CovPreP P) {
  const long long off = (long long)blockIdx.y * P.cell;
  const long long n = P.cell / VEC, stride = (long long)gridDim.x * COV_THREADS;
  for (long long i = (long long)blockIdx.x * COV_THREADS + threadIdx.x; i < n; i += stride) {
    const long long q = off + i * VEC;
    double fv[VEC], gv[VEC], fo[VEC], go[VEC], fg[VEC];
    CovIO<VEC>::get(fv, P.f + q);
    if (P.g) {
      CovIO<VEC>::get(gv, P.g + q);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) gv[k] = fv[k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) cov_pre(fv[k], gv[k], P.common != 0, fo[k], go[k], fg[k]);
    if (P.wr) {
      CovIO<VEC>::put(P.fo + q, fo);
      if (P.g) CovIO<VEC>::put(P.go + q, go);
    }
    CovIO<VEC>::put(P.fg + q, fg);
  }
}

// the post pass: F(fg), F(f'), F(g') -> tau
template <int VEC>
__global__ __launch_bounds__(COV_THREADS) void k_prepare(const CovPostP P) {
  const long long off = (long long)blockIdx.y * P.cell;
  const long long n = P.cell / VEC, stride = (long long)gridDim.x * COV_THREADS;
  for (long long i = (long long)blockIdx.x * COV_THREADS + threadIdx.x; i < n; i += stride) {
    const long long q = off + i * VEC;
    double a[VEC], b[VEC], c[VEC], o[VEC];
    CovIO<VEC>::get(a, P.a + q);
    CovIO<VEC>::get(b, P.b + q);
    if (P.c) {
      CovIO<VEC>::get(c, P.c + q);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) c[k] = b[k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = cov_post(a[k], b[k], c[k]);
    CovIO<VEC>::put(P.out + q, o);
  }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// workgroups along x for `npair` pairs of `units` threads' worth of work each: enough to cover a pair, capped so that a whole launch
// stays at a few workgroups per compute unit's slot and the rest is the grid-stride loop
static unsigned cov_grid_x(long long units, int64_t npair) {
  const long long need = (units + COV_THREADS - 1) / COV_THREADS;
  const long long cap = std::max<long long>(64, 8192 / std::max<int64_t>(1, npair));
  return (unsigned)std::max<long long>(1, std::min(need, cap));
}

static int launch_cov_pre(const CovPreP &P, bool vec, int64_t npair, hipStream_t s) {
  const int V = vec ? 2 : 1;
  dim3 block(COV_THREADS), grid(cov_grid_x(P.cell / V, npair), (unsigned)npair);
  if (vec)
    hipLaunchKernelGGL((k_prepare<2>), grid, block, 0, s, P);
  else
    hipLaunchKernelGGL((k_prepare<1>), grid, block, 0, s, P);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

static int launch_cov_post(const CovPostP &P, bool vec, int64_t npair, hipStream_t s) {
  const int V = vec ? 2 : 1;
  dim3 block(COV_THREADS), grid(cov_grid_x(P.cell / V, npair), (unsigned)npair);
  if (vec)
    hipLaunchKernelGGL((k_prepare<2>), grid, block, 0, s, P);
  else
    hipLaunchKernelGGL((k_prepare<1>), grid, block, 0, s, P);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

// gcmf_set_timing: an event pair of the call's own around each pass (gcmf_apply's pair brackets its schedule alone)
struct CovTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~CovTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

}  // namespace gcmf

using namespace gcmf;

extern "C" {

int gcmf_apply_cov(gcmf_plan *pl, const double *p, int n_steps, double c, const void *f, const void *g, void *out, int64_t npair,
                   uint32_t flags, void *stream) {
  if (!pl) {
    set_error("gcmf_apply_cov: `plan` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  const char *limit = pl->ncomp == 2 ? "vector plans (ncomp == 2) have no covariance call: scalar grid types only" :
                      pl->d.dtype != GCMF_F64 ? "f32 plans are not taken: tau is a small difference of large numbers, so the plan must be f64" :
                      (flags & GCMF_OUT_F32) ? "GCMF_OUT_F32 is not taken: tau is a small difference of large numbers, `out` is always f64" :
                      (pl->d.flags & GCMF_PLAN_SELF_RING) ? "not available on a GCMF_PLAN_SELF_RING plan" :
                      !pl->full ? "not available on a row slab: it needs a plan covering the whole grid" : nullptr;
  if (limit) {
    set_error("gcmf_apply_cov: %s (grid type %d)", limit, pl->d.grid_type);
    return GCMF_ERR_UNSUPPORTED;
  }
  if (!p || n_steps < 1) {
    set_error("gcmf_apply_cov: `p` is null or `n_steps` = %d is below 1", n_steps);
    return GCMF_ERR_INVALID_ARG;
  }
  if (!f) {
    set_error("gcmf_apply_cov: `f` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  if (!out) {
    set_error("gcmf_apply_cov: `out` is null");
    return GCMF_ERR_INVALID_ARG;
  }
  if (npair < 0) {
    set_error("gcmf_apply_cov: `npair` = %lld is negative", (long long)npair);
    return GCMF_ERR_INVALID_ARG;
  }
  const bool var = !g || g == f;
  const size_t cell = (size_t)pl->d.ny * (size_t)pl->d.nx, plane = cell * sizeof(double), bytes = (size_t)npair * plane;
  const char *b = ranges_overlap(out, bytes, f, bytes) ? "f" : (!var && ranges_overlap(out, bytes, g, bytes)) ? "g" : nullptr;
  if (b) {
    set_error("gcmf_apply_cov: `out` must not overlap `%s` as byte ranges (%zu bytes each)", b, bytes);
    return GCMF_ERR_INVALID_ARG;
  }
  if (pl->stacked && npair % pl->nlev) {
    set_error("gcmf_apply_cov: a stacked plan of %lld levels takes an `npair` that is a multiple of it (pair i runs on level i %% nlev), "
              "not %lld", (long long)pl->nlev, (long long)npair);
    return GCMF_ERR_INVALID_ARG;
  }
  if (npair == 0) return GCMF_OK;

  std::lock_guard<std::mutex> outer(pl->cov_mu);   // (gcmf_apply takes the plan's mutex itself, run by run)
  GCMF_HIP(hipSetDevice(pl->d.device));
  const bool on_dev = flags & GCMF_DEVICE_PTRS;
  const bool common = flags & (GCMF_MASK_FROM_NAN | GCMF_FACES_FROM_NAN);
  hipStream_t s = (on_dev || stream) ? (hipStream_t)stream : pl->stream;
  // a run: as many pairs as keep its 2 K planes each (K = 3 entries, 2 for a variance: the pre pass's and their filtered ones) at or
  // under "cov_scratch_mb" -- at least one, a stacked plan's in whole sets of levels (entry k N + i of the run's batch is then level
  // i % nlev: gcmf_apply runs entry e of ITS batch on level e % nlev), under GCMF_FACES_FROM_NAN no more than keep the folded planes of the
  // run's K N entries (25 bytes per cell and entry) at or under "gap_scratch_mb", and no more than one launch's gridDim.y takes
  const int K = var ? 2 : 3;
  const long long bound = (long long)std::max(0, pl->cov_scratch_mb) << 20;
  int64_t run_np = std::min<int64_t>(16384, bound / (long long)(2 * K * plane));
  if (flags & GCMF_FACES_FROM_NAN)
    run_np = std::min<int64_t>(run_np, ((long long)std::max(0, pl->gap_scratch_mb) << 20) / (long long)(K * 25 * cell));
  run_np = std::max<int64_t>(1, run_np);
  if (pl->stacked) run_np = std::max<int64_t>(pl->nlev, run_np / pl->nlev * pl->nlev);
  run_np = std::min(run_np, npair);
  const size_t half = up256((size_t)K * (size_t)run_np * plane), need = 2 * half;
  int rc;
  if ((rc = order_behind_last_call(pl, s))) return rc;
  if (need > pl->cov_bytes) {
    if (pl->cov_buf) GCMF_HIP(hipFree(pl->cov_buf));   // (synchronises the device: nothing reads the old block any more)
    pl->cov_buf = nullptr;
    pl->cov_bytes = 0;
    GCMF_HIP(hipMalloc(&pl->cov_buf, need));
    pl->cov_bytes = need;
  }
  double *pre = (double *)pl->cov_buf, *fil = (double *)((char *)pl->cov_buf + half);
  // 16-byte pairs: every plane of every pair then starts on a 16-byte boundary (the scratch does: hipMalloc's, and `half` is a multiple of 256)
  const bool vec = cell % 2 == 0 && aligned16(f) && (var || aligned16(g)) && aligned16(out);
  CovTimer tm;
  if (pl->timing) {
    GCMF_HIP(hipEventCreate(&tm.e0));
    GCMF_HIP(hipEventCreate(&tm.e1));
  }
  float ms = 0.f;
  int launches = 0;
  for (int64_t e0 = 0; e0 < npair; e0 += run_np) {
    const int64_t np = std::min(run_np, npair - e0);
    const size_t slot = (size_t)np * cell;   // doubles of one of the K groups of the run's batch
    const double *fr = (const double *)f + (size_t)e0 * cell, *gr = var ? nullptr : (const double *)g + (size_t)e0 * cell;
    double *outr = (double *)out + (size_t)e0 * cell;
    CovPreP A{};
    A.fo = pre;
    A.go = var ? nullptr : pre + slot;
    A.fg = pre + (size_t)(K - 1) * slot;
    A.cell = (long long)cell;
    A.common = common;
    if (on_dev) {
      A.f = fr;
      A.g = gr;
      A.wr = 1;
    } else {   // the fields go straight into their slots; the pass applies the common gaps there, where the call has them, and writes fg
      GCMF_HIP(hipMemcpyAsync(A.fo, fr, slot * sizeof(double), hipMemcpyHostToDevice, s));
      if (!var) GCMF_HIP(hipMemcpyAsync(A.go, gr, slot * sizeof(double), hipMemcpyHostToDevice, s));
      A.f = A.fo;
      A.g = A.go;
      A.wr = common;
    }
    if (tm.e0) GCMF_HIP(hipEventRecord(tm.e0, s));
    if ((rc = launch_cov_pre(A, on_dev ? vec : cell % 2 == 0, np, s))) return rc;
    if (tm.e0) GCMF_HIP(hipEventRecord(tm.e1, s));
    const void *in1[2] = {pre, nullptr};
    void *fil1[2] = {fil, nullptr};
    if ((rc = gcmf_apply(pl, p, n_steps, c, in1, fil1, (int64_t)K * np, flags | GCMF_DEVICE_PTRS, (void *)s))) return rc;
    {
      std::lock_guard<std::mutex> lk(pl->mu);
      if (pl->timing) ms += pl->last_ms;
      launches += pl->last_launches + 2;
    }
    if (tm.e0) {
      float t = 0.f;
      GCMF_HIP(hipEventSynchronize(tm.e1));
      GCMF_HIP(hipEventElapsedTime(&t, tm.e0, tm.e1));
      ms += t;
      GCMF_HIP(hipEventRecord(tm.e0, s));
    }
    CovPostP B{};
    B.a = fil + (size_t)(K - 1) * slot;
    B.b = fil;
    B.c = var ? nullptr : fil + slot;
    B.out = on_dev ? outr : pre;   // (host route: the run's f' slot is free once the schedule has run)
    B.cell = (long long)cell;
    if ((rc = launch_cov_post(B, on_dev ? vec : cell % 2 == 0, np, s))) return rc;
    if (tm.e0) {
      float t = 0.f;
      GCMF_HIP(hipEventRecord(tm.e1, s));
      GCMF_HIP(hipEventSynchronize(tm.e1));
      GCMF_HIP(hipEventElapsedTime(&t, tm.e0, tm.e1));
      ms += t;
    }
    {
      std::lock_guard<std::mutex> lk(pl->mu);
      // (gcmf_apply has put its event behind ITS launches where the stream is a caller's that may go away: behind the pass as well)
      if (pl->busy_recorded) GCMF_HIP(hipEventRecord(pl->ev_busy, s));
    }
    if (!on_dev) {
      GCMF_HIP(hipMemcpyAsync(outr, pre, slot * sizeof(double), hipMemcpyDeviceToHost, s));
      GCMF_HIP(hipStreamSynchronize(s));
      std::lock_guard<std::mutex> lk(pl->mu);
      const unsigned rlo = pl->res_lo, rhi = pl->res_hi;
      pl->res_lo = pl->res_hi = 0;   // (the stream is drained: the synchronising host route can tell for THIS call, as gcmf_apply's does)
      if (rlo && resident_take_failure(pl->d.device, rlo, rhi)) {
        set_error("gcmf_apply_cov: the on-chip launch timed out waiting for a neighbour tile: the result is NaN; the "
                  "strip-marching launches are used from now on");
        return GCMF_ERR_HIP;
      }
    }
  }
  std::lock_guard<std::mutex> lk(pl->mu);
  if (pl->timing) pl->last_ms = ms;
  pl->last_launches = launches;
  return GCMF_OK;
}

}  // extern "C"
