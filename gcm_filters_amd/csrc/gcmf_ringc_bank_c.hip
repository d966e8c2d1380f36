// k_ringc<double, K_FLUX, S, FIRST, true, true> of filter banks, seven and six levels (see gcmf_ringc_bank.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_bank_c(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  switch (a.S) {
    case 7: return a.first ? launch_ringc_bank_sf<7, true>(pl, cv, a, cut, s) : launch_ringc_bank_sf<7, false>(pl, cv, a, cut, s);
    case 6: return a.first ? launch_ringc_bank_sf<6, true>(pl, cv, a, cut, s) : launch_ringc_bank_sf<6, false>(pl, cv, a, cut, s);
  }
  set_error("k_ringc (filter bank): depth %d is not offered", a.S);
  return GCMF_ERR_INVALID_ARG;
}
}  // namespace gcmf
