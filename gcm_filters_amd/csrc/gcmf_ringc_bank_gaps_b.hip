// k_ringc<double, K_FLUX, S, FIRST, true, false> of filter banks over per-field planes, eight and five levels (see gcmf_ringc_bank_gaps.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_bank_gaps_b(GCMF_RINGC_DEFINE)
}  // namespace gcmf
