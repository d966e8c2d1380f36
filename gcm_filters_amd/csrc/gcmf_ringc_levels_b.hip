// k_ringc<double, K_FLUX, S, FIRST, false, true> of stacked plans, seven, six and five levels (see gcmf_ringc_levels.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_levels_b(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  switch (a.S) {
    case 7: return a.first ? launch_ringc_levels_sf<7, true>(pl, cv, a, cut, s) : launch_ringc_levels_sf<7, false>(pl, cv, a, cut, s);
    case 6: return a.first ? launch_ringc_levels_sf<6, true>(pl, cv, a, cut, s) : launch_ringc_levels_sf<6, false>(pl, cv, a, cut, s);
    case 5: return a.first ? launch_ringc_levels_sf<5, true>(pl, cv, a, cut, s) : launch_ringc_levels_sf<5, false>(pl, cv, a, cut, s);
  }
  set_error("k_ringc (stacked plan): depth %d is not offered", a.S);
  return GCMF_ERR_INVALID_ARG;
}
}  // namespace gcmf
