// k_ringc<double, K_FLUX, S, FIRST, true, false> of filter banks over per-field planes, eight and five levels (see gcmf_ringc_bank_gaps.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_bank_gaps_c(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
int launch_ringc_bank_gaps_b(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  switch (a.S) {
    case 8: return a.first ? launch_ringc_bank_gaps_sf<8, true>(pl, cv, a, cut, s) : launch_ringc_bank_gaps_sf<8, false>(pl, cv, a, cut, s);
    case 5: return a.first ? launch_ringc_bank_gaps_sf<5, true>(pl, cv, a, cut, s) : launch_ringc_bank_gaps_sf<5, false>(pl, cv, a, cut, s);
  }
  return launch_ringc_bank_gaps_c(pl, cv, a, cut, s);
}
}  // namespace gcmf
