// k_ringcs: the flux-kind backward kernel with early exits, for row slabs without a tripole seam (gcmf_ringc_impl.hpp): f64 state, five and
// six levels; seven and eight: gcmf_ringc_flux_slab_b.hip; f32 state: gcmf_ringc_flux_slab_f32[b].hip (translation units that compile side by side)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_flux_slab(GCMF_RINGC_DEFINE)
}  // namespace gcmf
