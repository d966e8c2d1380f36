// GCMF_FACES_FROM_NAN: the fold rule that turns an ordinary flux-form plan's coefficient planes into those of ONE batch entry whose own
// NaNs are gaps (land).  No HIP header is needed: the device kernel (k_pre_isolated<T, true, MOM5>, gcmf_precompute.hip) and a plain C++
// program (tests/gap_fold/) compile the same functions.
//
// An ordinary plan of IRREGULAR_WITH_LAND, MOM5U or MOM5T holds cE (east face), cN (north face) and ra = 1 / area, with wet_mask and the
// kappas folded in (k_pre_irregular, k_pre_mom5).  For entry b let n(j, i) = [field_b(j, i) is not NaN]; +-inf is data.  Wrap is periodic in
// x and y.  The entry's planes are what those kernels produce from wet_mask * n:
//   IRREGULAR_WITH_LAND   cE_b(j,i) = cE(j,i) * [n(j,i) && n(j,i+1)]      cN_b(j,i) = cN(j,i) * [n(j,i) && n(j+1,i)]
//   MOM5U / MOM5T         cN_b(j,i) = cN(j,i) * [n(j,i) && n(j,i+1)]      cE_b(j,i) = cE(j,i) * [n(j,i) && n(j+1,i)]
//                         (the reference pairs the masks the other way round there, kernels.py:345-372; k_pre_mom5 keeps that)
// A product, not a select: c * 1.0 is c, and c * 0.0 carries the sign (or the NaN of an infinite c) that the reference's
// ratio * (m * m * kappa) has when a mask factor is 0 -- the planes agree bit for bit.
// Land byte: 1 where any of cE_b(j,i), cE_b(j,i-1), cN_b(j,i), cN_b(j-1,i) is non-zero (k_pre_isolated's rule on the entry's planes).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define GCMF_GAP_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define GCMF_GAP_HD inline
#endif

namespace gcmf {

template <typename T> GCMF_GAP_HD bool gap_present(T v) { return v == v; }   // not a gap (+-inf is data)

// The faces of cell (j, i): nc = n(j, i), nxp = n(j, i + 1), nyp = n(j + 1, i)
template <typename T, bool MOM5> GCMF_GAP_HD T gap_fold_cE(T cE, bool nc, bool nxp, bool nyp) {
  return cE * ((nc && (MOM5 ? nyp : nxp)) ? T(1) : T(0));
}
template <typename T, bool MOM5> GCMF_GAP_HD T gap_fold_cN(T cN, bool nc, bool nxp, bool nyp) {
  return cN * ((nc && (MOM5 ? nxp : nyp)) ? T(1) : T(0));
}
// cE_b, cN_b of the cell, cE_b of its western and cN_b of its southern neighbour
template <typename T> GCMF_GAP_HD unsigned gap_land_byte(T cEb, T cEb_w, T cNb, T cNb_s) {
  return (cEb != T(0) || cEb_w != T(0) || cNb != T(0) || cNb_s != T(0)) ? 1u : 0u;
}

GCMF_GAP_HD int gap_wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// One cell from whole planes (the host restatement; the kernel works on four cells at a time from the same three functions)
template <typename T, bool MOM5>
GCMF_GAP_HD unsigned gap_fold_cell(const T *f, const T *cE, const T *cN, int ny, int nx, int j, int i, T *cEb, T *cNb) {
  const int ie = gap_wrap(i + 1, nx), iw = gap_wrap(i - 1, nx), jn = gap_wrap(j + 1, ny), js = gap_wrap(j - 1, ny);
  auto n = [&](int jj, int ii) { return gap_present(f[(long long)jj * nx + ii]); };
  auto at = [&](const T *p, int jj, int ii) { return p[(long long)jj * nx + ii]; };
  const T e = gap_fold_cE<T, MOM5>(at(cE, j, i), n(j, i), n(j, ie), n(jn, i));
  const T nn = gap_fold_cN<T, MOM5>(at(cN, j, i), n(j, i), n(j, ie), n(jn, i));
  const T ew = gap_fold_cE<T, MOM5>(at(cE, j, iw), n(j, iw), n(j, i), n(jn, iw));
  const T ns = gap_fold_cN<T, MOM5>(at(cN, js, i), n(js, i), n(js, ie), n(j, i));
  *cEb = e;
  *cNb = nn;
  return gap_land_byte(e, ew, nn, ns);
}

// A whole plane on the host
template <typename T>
inline void gap_fold_plane(const T *f, const T *cE, const T *cN, int ny, int nx, bool mom5, T *cEb, T *cNb, unsigned char *bytes) {
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const long long q = (long long)j * nx + i;
      bytes[q] = (unsigned char)(mom5 ? gap_fold_cell<T, true>(f, cE, cN, ny, nx, j, i, cEb + q, cNb + q)
                                      : gap_fold_cell<T, false>(f, cE, cN, ny, nx, j, i, cEb + q, cNb + q));
    }
}

}  // namespace gcmf
