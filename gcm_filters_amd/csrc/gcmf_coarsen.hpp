// gcmf_apply_coarsen: the rule that turns a fine plane F and a weight plane w into weighted block means.  No HIP header is needed: the
// device pass (a form of k_prepare, gcmf_coarsen.hip) and a plain C++ program (tests/coarsen/) compile the same functions.
//
// For factors (fy, fx) that divide (ny, nx), block (J, I) holds the cells j in [J fy, (J + 1) fy), i in [I fx, (I + 1) fx):
//   count(j,i)  = w(j,i) > 0  &&  F(j,i) == F(j,i)     +-inf in F is data; a NaN in F, w <= 0 (+-0 too) and a NaN weight are SKIPPED --
//                                                      never multiplied: 0 * inf would be NaN, and F on land is finite junk
//   wsum(J,I)   = sum of w over the counted cells
//   coarse(J,I) = sum of w * F over the counted cells / wsum(J,I);   NaN, and wsum = 0, where no cell counts
// Everything is f64.  THE ORDER OF THE SUMS is fixed, and the same here and on the device whatever the batch, the alignment of the
// planes or the vector width: first every fine COLUMN of the block is summed over its rows, southernmost first (col(i) = ((t_0 + t_1) +
// t_2) + ..., a skipped cell adds +0.0), then the columns are summed from west to east, again one after the other from 0.0.  Products
// are rounded once (no fused multiply-add: the library is built with -ffp-contract=off, and coarsen_term is a product, then an add).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define GCMF_COARSEN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GCMF_COARSEN_HD inline
#endif

namespace gcmf {

// the per-cell predicate (a NaN weight fails w > 0)
GCMF_COARSEN_HD bool coarsen_counts(double w, double f) { return w > 0.0 && f == f; }
// what a cell adds to its column's two sums: (w * f, w) where it counts, (+0, +0) where it does not
GCMF_COARSEN_HD void coarsen_term(double w, double f, double &sp, double &sw) {
  const bool c = coarsen_counts(w, f);
  const double prod = w * f;   // (computed for every cell, used for the counted ones: the device code has no branch here)
  sp = sp + (c ? prod : 0.0);
  sw = sw + (c ? w : 0.0);
}
// a block's mean from its two sums
GCMF_COARSEN_HD double coarsen_mean(double sp, double sw) {
  const double nan = __builtin_nan("");
  return sw > 0.0 ? sp / sw : nan;
}

// A whole plane on the host: the restatement the device pass is tested against.  w == nullptr: every weight is 1.
inline void coarsen_plane(const double *f, const double *w, int ny, int nx, int fy, int fx, double *coarse, double *wsum) {
  const int cy = ny / fy, cx = nx / fx;
  for (int J = 0; J < cy; ++J)
    for (int I = 0; I < cx; ++I) {
      double sp = 0.0, sw = 0.0;
      for (int i = I * fx; i < (I + 1) * fx; ++i) {
        double cp = 0.0, cw = 0.0;   // the column's sums
        for (int j = J * fy; j < (J + 1) * fy; ++j) {
          const long long q = (long long)j * nx + i;
          coarsen_term(w ? w[q] : 1.0, f[q], cp, cw);
        }
        sp = sp + cp;
        sw = sw + cw;
      }
      const long long Q = (long long)J * cx + I;
      coarse[Q] = coarsen_mean(sp, sw);
      if (wsum) wsum[Q] = sw;
    }
}

}  // namespace gcmf
