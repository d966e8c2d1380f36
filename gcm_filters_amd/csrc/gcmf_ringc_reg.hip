// k_ringc (backward / Clenshaw evaluation, gcmf_ringc_impl.hpp) instantiations for K_REG, f64 state; the f32 ones: gcmf_ringc_reg_f32.hip
// (one translation unit per stencil kind and state type: they compile side by side)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_reg(GCMF_RINGC_DEFINE)
}  // namespace gcmf
