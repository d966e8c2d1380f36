// k_ringc<float, K_REG, ...>: the f32-state instantiations of gcmf_ringc_reg.hip, in their own translation unit
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_reg_f32(GCMF_RINGC_DEFINE)
}  // namespace gcmf
