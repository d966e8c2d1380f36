// k_ringc<double, K_FLUX, S, FIRST, false, true> of stacked plans, seven, six and five levels (see gcmf_ringc_levels.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_levels_b(GCMF_RINGC_DEFINE)
}  // namespace gcmf
