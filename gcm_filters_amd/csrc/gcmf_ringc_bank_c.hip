// k_ringc<double, K_FLUX, S, FIRST, true, true> of filter banks, seven and six levels (see gcmf_ringc_bank.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_bank_c(GCMF_RINGC_DEFINE)
}  // namespace gcmf
