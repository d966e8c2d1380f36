// k_ringcs<float>: the f32-state flux-kind backward kernel with early exits (gcmf_ringc_impl.hpp, gcmf_ringc_flux_slab.hip), five and six
// levels; seven and eight: gcmf_ringc_flux_slab_f32b.hip (translation units that compile side by side)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_flux_slab_f32(GCMF_RINGC_DEFINE)
}  // namespace gcmf
