// k_ringc (backward / Clenshaw evaluation, gcmf_ringc_impl.hpp) instantiations for K_MASKZ, f64 state; the f32 ones: gcmf_ringc_maskz_f32.hip
// (one translation unit per stencil kind and state type: they compile side by side)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_maskz(GCMF_RINGC_DEFINE)
}  // namespace gcmf
