// Land kept out of the state (see gcmf_plan::lbits): the result of a cell that exchanges nothing with its neighbours.
//
// Such a cell has L = 0 at every step (reference: the land mask / the closed faces zero every flux, kernels.py:163-187,
// 286-315), so its recurrence T_k = 2(-T_{k-1} - c 0) - T_{k-2}, fbar += p_k T_k (filter.py:162-212) involves nothing but
// its own input value.  gcmf_apply runs the blocked kernels with these cells zeroed and calls this kernel at the end: it
// replays the recurrence with the same operations, in the same precision and order as the stencil kernels (the helpers of
// gcmf_recurrence.hpp), prepare / finalize included, and writes the result over `out` on those cells only.
#include "gcmf_multi_common.hpp"

namespace gcmf {

// LV: a stacked plan (gcmf_plan_create_levels) -- lbits holds nlev planes, one per level, and entry b reads plane (lev0 + b) % nlev;
// per_field = nlev | lev0 << 16 (nlev <= 32768).  An instantiation of its own: as a runtime branch in the one kernel (with its second
// 64-bit division) BASELINE config 3 measured 0.7 % slower, 0.747 against 0.741 ms per application, three alternating runs each
// PB: a filter bank (gcmf_apply_bank) -- blockIdx.y is the launch's entry, entry e = ent0 + blockIdx.y is row e / nfield of the table p
// (n_steps + 1 doubles per row) on field e % nfield of `in`, its result the launch's plane blockIdx.y of `out`; per_field = nfield,
// ntotal = ncell (a workgroup stays inside one entry: one polynomial in its LDS), lbits the plan's one plane.  An instantiation of its own.
// LV and PB: a filter bank over per-field planes (gcmf_apply_bank_gaps) -- PB's form with the land bytes of the entry's own FIELD, plane
// e % nfield of lbits (a gap is land in its own field's plane: it comes out NaN, the input's own value).
template <typename T, typename FB, bool FUSED, bool LV = false, bool PB = false>
__global__ __launch_bounds__(256) void k_land_fix(const T *in, FB *out, const uint8_t *lbits, const T *area,
                                                  const double *p, int n_steps, double c_, long long ncell,
                                                  long long ntotal, int per_field, int ent0) {
  extern __shared__ double sp[];  // p[0..n_steps], read by every step of every cell
  if constexpr (PB) {
    const int e = ent0 + (int)blockIdx.y, pol = e / per_field;
    p += (long long)pol * (n_steps + 1);
    in += (long long)(e - pol * per_field) * ncell;
    out += (long long)blockIdx.y * ncell;
    if constexpr (LV) lbits += (long long)(e - pol * per_field) * ncell;
  }
  for (int k = threadIdx.x; k <= n_steps; k += blockDim.x) sp[k] = p[k];
  __syncthreads();
  const T c = (T)c_;
  // four consecutive cells per thread (ncell is a multiple of 4: one field, one word of the byte plane): four independent
  // dependency chains per lane; cells that do exchange with neighbours are computed along and not stored
  for (long long q4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; q4 < ntotal; q4 += (long long)gridDim.x * blockDim.x * 4) {
    const long long cell = q4 % ncell;
    unsigned m;
    if constexpr (PB) m = *reinterpret_cast<const unsigned *>(lbits + q4);
    else if constexpr (LV) m = *reinterpret_cast<const unsigned *>(lbits + (((per_field >> 16) + q4 / ncell) % (per_field & 0xFFFF)) * ncell + cell);
    else m = *reinterpret_cast<const unsigned *>(lbits + (per_field ? q4 : cell));   // (per_field: every entry its own plane of bytes)
    if ((m & 0x01010101u) == 0x01010101u) continue;
    T xm2[4], xm1[4];
    FB fb[4];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      T x = in[q4 + j];
      if (area) x = x * area[cell + j];                 // prepare()
      const T a = cheb_a<FUSED>(x, c, T(0));
      fb[j] = cheb_acc_first<FUSED, T, FB>(sp[0], sp[1], x, a);
      xm2[j] = x;
      xm1[j] = a;
      // |x| <= max / 2 of the STATE type: the unfused forward kinds form 2 * a, which overflows beyond that and the general loop's bits
      // would differ (advisor, round 3)
      finite = finite && (mabs(x) <= MLim<T>::big() * T(0.5));
    }
    if (finite) {
      // With L = 0 and a finite x every step is exact up to the running sum: A(T) = -T, T_k = 2 A(T_{k-1}) - T_{k-2} = (-1)^k x, so only
      // fbar's chain is left (one dependent operation per step instead of three) -- the SAME bits: p_k * (-x) = -(p_k * x), fused or not.
      // (an infinite x makes T_2 = inf - inf = NaN in the recurrence: those cells take the general loop below)
      for (int k = 2; k <= n_steps; ++k) {
        const double pk = sp[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = cheb_acc<FUSED, T, FB>(fb[j], pk, (k & 1) ? xm1[j] : xm2[j]);   // xm1 = -x, xm2 = x
      }
    } else {
      for (int k = 2; k <= n_steps; ++k) {
        const double pk = sp[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const T a = cheb_a<FUSED>(xm1[j], c, T(0));
          const T tk = cheb_t<FUSED>(a, xm2[j]);
          fb[j] = cheb_acc<FUSED, T, FB>(fb[j], pk, tk);
          xm2[j] = xm1[j];
          xm1[j] = tk;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((m >> (8 * j)) & 1u) continue;
      FB r = fb[j];
      if (area) r = r / (FB)area[cell + j];             // finalize()
      out[q4 + j] = r;
    }
  }
}

// zero the isolated cells of two state planes in place (the outputs of the first blocked launch): from then on NaN on land
// cannot reach the NaN / inf bookkeeping of the blocked kernels.  Reads the byte plane, writes land cells only.
// Cells [cell0, cell0 + nsub) of every field (both multiples of 4: the caller checks nx % 4 == 0).
template <typename T>
__global__ __launch_bounds__(256) void k_zero_land(T *a, T *b, const uint8_t *lbits, long long ncell, long long cell0, long long nsub,
                                                   long long ntotal, int per_field) {
  for (long long q4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; q4 < ntotal; q4 += (long long)gridDim.x * blockDim.x * 4) {
    const long long field = q4 / nsub, cell = cell0 + (q4 - field * nsub);  // 4 cells of one field
    const long long o = field * ncell + cell;
    const unsigned m = *reinterpret_cast<const unsigned *>(lbits + (per_field ? o : cell));
    if ((m & 0x01010101u) == 0x01010101u) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!((m >> (8 * k)) & 1u)) { a[o + k] = T(0); b[o + k] = T(0); }
  }
}

// rows [row_lo, row_hi) of both planes (row_hi <= 0: all rows)
int launch_zero_land(gcmf_plan *pl, const CallView &cv, void *a, void *b, int64_t nbatch, hipStream_t s, int row_lo, int row_hi) {
  if (cv.stacked) {   // (only the forward schedule and gcmf_zero_land zero land in place: neither runs on a stacked plan)
    set_error("k_zero_land: not available on a stacked plan (gcmf_plan_create_levels)");
    return GCMF_ERR_UNSUPPORTED;
  }
  if (row_hi <= 0) { row_lo = 0; row_hi = (int)pl->rows_alloc; }
  const long long ncell = (long long)pl->rows_alloc * pl->d.nx, cell0 = (long long)row_lo * pl->d.nx;
  const long long nsub = (long long)(row_hi - row_lo) * pl->d.nx, ntotal = nsub * nbatch;
  if (ntotal <= 0) return GCMF_OK;
  long long nb = (ntotal / 4 + 255) / 256;
  if (nb > 65536) nb = 65536;
  dim3 block(256), grid((unsigned)nb);
  if (pl->d.dtype == GCMF_F64)
    hipLaunchKernelGGL(k_zero_land<double>, grid, block, 0, s, (double *)a, (double *)b, cv.lbits, ncell, cell0, nsub, ntotal, cv.mask_per_field);
  else
    hipLaunchKernelGGL(k_zero_land<float>, grid, block, 0, s, (float *)a, (float *)b, cv.lbits, ncell, cell0, nsub, ntotal, cv.mask_per_field);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

template <typename T, typename FB>
static int launch_lf(gcmf_plan *pl, const CallView &cv, const void *in, void *out, const double *dp, int n_steps, double c, int64_t nbatch,
                     hipStream_t s) {
  const long long ncell = (long long)pl->rows_alloc * pl->d.nx, ntotal = ncell * nbatch;
  const T *area = pl->area_weighted ? (const T *)pl->g.area : nullptr;
  long long nb = (ntotal / 4 + 255) / 256;
  if (nb > 32768) nb = 32768;
  dim3 block(256), grid((unsigned)nb);
  const size_t lds = ((size_t)n_steps + 1) * sizeof(double);
  if constexpr (sizeof(T) == 8 && sizeof(FB) == 8) {
    if (cv.stacked) {   // (f64 flux kinds; one level: the plan's one plane, the ordinary kernel)
      if (cv.nlev >= 2) {
        hipLaunchKernelGGL((k_land_fix<T, FB, true, true>), grid, block, lds, s, (const T *)in, (FB *)out, cv.lbits, area, dp, n_steps, c, ncell,
                           ntotal, (int)cv.nlev | ((int)(cv.entry0 % cv.nlev) << 16), 0);
        GCMF_HIP(hipGetLastError());
        return GCMF_OK;
      }
    }
  }
  if (pl->kind == K_FLUX)
    hipLaunchKernelGGL((k_land_fix<T, FB, true>), grid, block, lds, s, (const T *)in, (FB *)out, cv.lbits, area, dp, n_steps, c,
                       ncell, ntotal, cv.mask_per_field, 0);
  else
    hipLaunchKernelGGL((k_land_fix<T, FB, false>), grid, block, lds, s, (const T *)in, (FB *)out, cv.lbits, area, dp, n_steps,
                       c, ncell, ntotal, cv.mask_per_field, 0);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

int launch_land_fix_bank(gcmf_plan *pl, const CallView &cv, const void *in, void *out, int n_steps, double c, int64_t nbatch, hipStream_t s) {
  // (a stacked view: gcmf_apply_bank_gaps, one plane of land bytes per field)
  if (pl->kind != K_FLUX || pl->d.dtype != GCMF_F64 || (cv.stacked && cv.nlev != cv.bank_nfield) || pl->area_weighted || cv.bank_n < 1 || !cv.bank_fwd ||
      cv.bank_stride != (size_t)n_steps + 1 || nbatch < 1 || nbatch > 65535 || (pl->d.nx % 4) != 0) {
    set_error("k_land_fix (filter bank): not an ordinary f64 flux plan inside gcmf_apply_bank / gcmf_apply_bank_gaps");
    return GCMF_ERR_INVALID_ARG;
  }
  const long long ncell = (long long)pl->rows_alloc * pl->d.nx;
  long long nb = (ncell / 4 + 255) / 256;
  if (nb > 32768) nb = 32768;
  dim3 block(256), grid((unsigned)nb, (unsigned)nbatch);
  const size_t lds = ((size_t)n_steps + 1) * sizeof(double);
  if (cv.stacked)
    hipLaunchKernelGGL((k_land_fix<double, double, true, true, true>), grid, block, lds, s, (const double *)in, (double *)out, cv.lbits, (const double *)nullptr,
                       cv.bank_fwd, n_steps, c, ncell, ncell, (int)cv.bank_nfield, (int)cv.entry0);
  else
    hipLaunchKernelGGL((k_land_fix<double, double, true, false, true>), grid, block, lds, s, (const double *)in, (double *)out, cv.lbits, (const double *)nullptr,
                       cv.bank_fwd, n_steps, c, ncell, ncell, (int)cv.bank_nfield, (int)cv.entry0);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

int launch_land_fix(gcmf_plan *pl, const CallView &cv, const void *in, void *out, const double *dp, int n_steps, double c, int fb_is_f32,
                    int64_t nbatch, hipStream_t s) {
  if (pl->d.dtype == GCMF_F64) return launch_lf<double, double>(pl, cv, in, out, dp, n_steps, c, nbatch, s);
  if (fb_is_f32) return launch_lf<float, float>(pl, cv, in, out, dp, n_steps, c, nbatch, s);
  return launch_lf<float, double>(pl, cv, in, out, dp, n_steps, c, nbatch, s);
}

}  // namespace gcmf
