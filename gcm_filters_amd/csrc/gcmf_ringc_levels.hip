// k_ringc<double, K_FLUX, S, FIRST, false, true>: the plain strips of a STACKED plan (gcmf_plan_create_levels) -- every batch entry marches
// with the coefficient planes and land bytes of its own level (ringc_march<LV>, gcmf_ringc_impl.hpp).  Nine and eight levels here, seven,
// six and five in gcmf_ringc_levels_b.hip (the instantiations of a unit compile one after the other).
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_levels_b(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
int launch_ringc_levels(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  switch (a.S) {
    case 9: return a.first ? launch_ringc_levels_sf<9, true>(pl, cv, a, cut, s) : launch_ringc_levels_sf<9, false>(pl, cv, a, cut, s);
    case 8: return a.first ? launch_ringc_levels_sf<8, true>(pl, cv, a, cut, s) : launch_ringc_levels_sf<8, false>(pl, cv, a, cut, s);
  }
  return launch_ringc_levels_b(pl, cv, a, cut, s);
}
}  // namespace gcmf
