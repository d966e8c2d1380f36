// k_ringcs<float> at seven and eight levels (see gcmf_ringc_flux_slab_f32.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_flux_slab_f32b(GCMF_RINGC_DEFINE)
}  // namespace gcmf
