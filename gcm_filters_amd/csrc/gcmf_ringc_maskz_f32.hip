// k_ringc<float, K_MASKZ, ...>: the f32-state instantiations of gcmf_ringc_maskz.hip, in their own translation unit
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_maskz_f32(GCMF_RINGC_DEFINE)
}  // namespace gcmf
