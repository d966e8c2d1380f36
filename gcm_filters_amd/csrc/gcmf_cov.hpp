// gcmf_apply_cov: the two cell rules around the schedule that turn a pair of fields (f, g) into the subfilter covariance
//   tau(f, g) = F(f g) - F(f) F(g).
// No HIP header is needed: the device passes (forms of k_prepare, gcmf_cov.hip) and a plain C++ program (tests/cov/) compile the same
// functions.
//
// PRE, one cell of a pair; `common` = the call derives its gaps from NaNs (GCMF_MASK_FROM_NAN or GCMF_FACES_FROM_NAN):
//   n  = (f == f) && (g == g)            +-inf is data
//   f' = (common && !n) ? NaN : f        g' likewise: all three entries of the pair then carry the SAME gaps, isnan(f) | isnan(g)
//   fg = f' * g'                         one rounding
// Without `common`, f and g pass through bit for bit (a NaN keeps its payload).
// POST, one cell: out = a - b * c with a = F(fg), b = F(f'), c = F(g') -- a product rounded once, then a difference rounded once, never a
// fused multiply-add (the library is built with -ffp-contract=off; a host program that includes this header must be, too).  A NaN in any
// operand gives NaN.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define GCMF_COV_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GCMF_COV_HD inline
#endif

namespace gcmf {

// f, g -> f', g', f' * g'
GCMF_COV_HD void cov_pre(double f, double g, bool common, double &fo, double &go, double &fg) {
  const bool n = (f == f) && (g == g);
  const double nan = __builtin_nan("");
  fo = (common && !n) ? nan : f;
  go = (common && !n) ? nan : g;
  fg = fo * go;
}
// F(fg), F(f'), F(g') -> tau
GCMF_COV_HD double cov_post(double a, double b, double c) {
  const double bc = b * c;
  return a - bc;
}

// Whole planes on the host: the restatement the device passes are tested against.  g == nullptr or g == f: the variance form, which
// writes no go plane (go may be nullptr).
inline void cov_pre_plane(const double *f, const double *g, long long n, bool common, double *fo, double *go, double *fg) {
  const bool var = !g || g == f;
  for (long long q = 0; q < n; ++q) {
    double a, b, ab;
    cov_pre(f[q], var ? f[q] : g[q], common, a, b, ab);
    fo[q] = a;
    if (!var) go[q] = b;
    fg[q] = ab;
  }
}
// c == nullptr: the variance form, out = a - b * b
inline void cov_post_plane(const double *a, const double *b, const double *c, long long n, double *out) {
  for (long long q = 0; q < n; ++q) out[q] = cov_post(a[q], b[q], c ? c[q] : b[q]);
}

}  // namespace gcmf
