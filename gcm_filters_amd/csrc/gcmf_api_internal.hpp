// Private to the gcmf_api*.hip translation units (round 6: gcmf_api.hip was one file of 1 600 lines): what they share.
//   gcmf_api.hip          plan lifetime, gcmf_apply / gcmf_laplacian (the whole-polynomial drivers, host paths)
//   gcmf_api_blocks.hip   the row-slab building blocks and drivers (gcmf_cheb_*, gcmf_slab_apply_backward*, land helpers, resident levels)
//   gcmf_api_options.hip  tuning, named options, instrumentation and the per-launch timing events
#pragma once
#include "gcmf_internal.hpp"

namespace gcmf {
// gcmf_api.hip
int step_dispatch(gcmf_plan *pl, const CallView &cv, const StepArgs &a, hipStream_t s);
int land_fix_tail(gcmf_plan *pl, const CallView &cv, const double *p, int n_steps, double c, const void *in, void *out, bool fb32, int64_t nbatch,
                  hipStream_t s);
// gcmf_api_options.hip: an event pair around every launch of the dominant kernel (gcmf_set_timing(plan, 2))
int dom_begin(gcmf_plan *pl, hipStream_t s);
int dom_end(gcmf_plan *pl, hipStream_t s);
int dom_collect(gcmf_plan *pl);
// gcmf_api_blocks.hip
bool land_ok(const gcmf_plan *pl, const CallView &cv, int n_steps);
bool ringc9_ok(const gcmf_plan *pl);
int clenshaw_cut(const gcmf_plan *pl, const CallView &cv, int n_steps, int *depths, int max_depths, bool f32_asked = false, int64_t nbatch = 1);   // (nbatch: a lone field on a cache-resident grid may be cut into shallower launches)
bool bank_plan_ok(const gcmf_plan *pl, const CallView &cv);   // an ordinary whole-grid f64 plan of the four flux-form grid types: what gcmf_apply_bank runs on
int bank_cut(const gcmf_plan *pl, const CallView &cv, int n_steps, int64_t nentries, int *depths, int max_depths);   // gcmf_bank_cut
bool ptr_al16(const void *p);
int vec_backward_next_depth(const gcmf_plan *pl, int64_t nbatch, int left, int smax);

// The two entries of a pool of four state planes (ncomp = 2: plane pairs, pool[2 q + comp]) that hold neither u nor v, in pool
// order -- the order decides which buffer each launch writes.  fr[ncomp * k + comp]; a launch must not overwrite the planes its
// neighbours' halos are still reading.
inline void free_planes(void *const *pool, int ncomp, const void *u, const void *v, void **fr) {
  int nf = 0;
  for (int k = 0; k < 2 * ncomp; ++k) fr[k] = nullptr;
  for (int q = 0; q < 4 && nf < 2; ++q)
    if (pool[ncomp * q] != u && pool[ncomp * q] != v) {
      for (int k = 0; k < ncomp; ++k) fr[ncomp * nf + k] = pool[ncomp * q + k];
      ++nf;
    }
}

// Levels lvl .. lvl+S-1 of a backward (Clenshaw) application of p[0..n_steps] to f: state (u, v) = (b_{k+1}, b_{k+2}) -> fr, level l
// uses p[n_steps - l] (into pk: an on-chip launch takes more levels than MultiArgs holds), the first launch forms b_n = p[n_steps] f,
// the last one writes `out`.  Row range, batch and flags are the caller's.
inline MultiArgs backward_args(const double *p, int n_steps, double c, int lvl, int S, const void *u, const void *v, void *const *fr,
                               const void *f, void *out, double *pk = nullptr) {
  MultiArgs m{};
  m.u0 = u; m.v0 = v; m.uo = fr[0]; m.vo = fr[1];
  m.fb_in = f; m.fb_out = out;
  m.first = (lvl == 1); m.last = (lvl + S - 1 == n_steps); m.S = S; m.lvl = lvl;
  if (!pk) pk = m.pk;
  for (int t = 0; t < S; ++t) pk[t] = p[n_steps - (lvl + t)];
  m.p0 = p[n_steps]; m.c = c;
  return m;
}
// ... of a vector plan: u, v, f, out per component, fr as free_planes(pool, 2, ...) leaves it (the launch writes fr[0 / 1] to u1o
// and fr[2 / 3] to u2o)
inline VecMultiArgs backward_args_vec(const double *p, int n_steps, double c, int lvl, int S, const void *const *u, const void *const *v,
                                      void *const *fr, const void *const *f, void *const *out) {
  VecMultiArgs m{};
  for (int q = 0; q < 2; ++q) {
    m.u0[q] = u[q]; m.uprev[q] = v[q]; m.u1o[q] = fr[q]; m.u2o[q] = fr[2 + q];
    m.fb_in[q] = f[q]; m.fb_out[q] = out[q];
  }
  for (int t = 0; t < S; ++t) m.pk[t] = p[n_steps - (lvl + t)];
  m.p0 = p[n_steps]; m.c = c; m.S = S; m.clen = 1;
  m.first = (lvl == 1); m.last = (lvl + S - 1 == n_steps);
  return m;
}

// The largest depth in [2, ceiling] that ok() accepts and that does not strand a lone single step at the end of `left`; 1 if none.
template <class Ok>
inline int deepest_depth(int left, int ceiling, Ok ok) {
  for (int S = ceiling; S >= 2; --S)
    if (S <= left && left - S != 1 && ok(S)) return S;
  return 1;
}
}  // namespace gcmf
