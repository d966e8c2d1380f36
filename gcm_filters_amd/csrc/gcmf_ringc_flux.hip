// k_ringc (backward / Clenshaw evaluation, gcmf_ringc_impl.hpp) instantiations for K_FLUX, f64 state; the f32 ones: gcmf_ringc_flux_f32.hip
// (one translation unit per stencil kind and state type: they compile side by side)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
int launch_ringc_flux_f32(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
int launch_ringc_flux(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  return pl->d.dtype != GCMF_F64 ? launch_ringc_flux_f32(pl, cv, a, cut, s) : launch_ringc_kind_f64<K_FLUX>(pl, cv, a, cut, s);
}
}  // namespace gcmf
