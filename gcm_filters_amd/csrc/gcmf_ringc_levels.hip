// k_ringc<double, K_FLUX, S, FIRST, false, true>: the plain strips of a STACKED plan (gcmf_plan_create_levels) -- every batch entry marches
// with the coefficient planes and land bytes of its own level (ringc_march<LV>, gcmf_ringc_impl.hpp).  Nine and eight levels here, seven,
// six and five in gcmf_ringc_levels_b.hip (the instantiations of a unit compile one after the other).
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_levels(GCMF_RINGC_DEFINE)
}  // namespace gcmf
