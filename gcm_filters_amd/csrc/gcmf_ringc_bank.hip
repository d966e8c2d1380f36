// k_ringc<double, K_FLUX, S, FIRST, true, true>: the plain strips of a FILTER BANK (gcmf_apply_bank) -- every batch entry marches with
// the coefficients of its own polynomial, read from a table in device memory, on the input plane of its own field (ringc_march<PB>,
// gcmf_ringc_impl.hpp).  Nine levels here, eight and five in gcmf_ringc_bank_b.hip, seven and six in gcmf_ringc_bank_c.hip (the instantiations
// of a unit compile one after the other).
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_bank_b(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
int launch_ringc_bank(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  if (a.S == 9) return a.first ? launch_ringc_bank_sf<9, true>(pl, cv, a, cut, s) : launch_ringc_bank_sf<9, false>(pl, cv, a, cut, s);
  return launch_ringc_bank_b(pl, cv, a, cut, s);
}
}  // namespace gcmf
