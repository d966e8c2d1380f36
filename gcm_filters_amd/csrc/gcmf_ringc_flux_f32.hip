// k_ringc<float, K_FLUX, ...>: the f32-state instantiations of gcmf_ringc_flux.hip, in their own translation unit
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_flux_f32(GCMF_RINGC_DEFINE)
}  // namespace gcmf
