// The launchers of the backward strip kernels (k_ringc, k_ringcp, k_ringcs, k_ringcz) and THE list of their instantiations, one row per
// translation unit.  A unit gcmf_ringc_<name>.hip is that row as explicit instantiation definitions (it includes gcmf_ringc_impl.hpp, where
// the launchers and kernels are defined); the dispatcher (gcmf_ringc_dispatch.hip) sees the same rows as explicit instantiation declarations
// and never the kernels.  The partition is tuned for build time (the instantiations of a unit compile one after the other, the units side by
// side): moving an entry to another row moves its kernels' compile there.  What the rows hold together is ringc_offered()
// (gcmf_ringc_cut.hpp); tests/test_ringc_table.py holds the objects to both.
#pragma once
#include "gcmf_internal.hpp"

namespace gcmf {

constexpr int RINGC_MASKZ = 5;   // K_MASKZ, the land-mask stencil on states whose land cells are zero (gcmf_scalar_multi_impl.hpp)

// k_ringc / k_ringcs (XE) / k_ringcp as the cut says; PF, LV: k_ringc's per-entry forms (gcmf_ringc_impl.hpp)
template <typename T, int KIND, int S, bool FIRST, bool XE = false, bool PF = false, bool LV = false>
int launch_ringc_sf(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
// k_ringcz: the even cut, the fold strips, or a launch from a wet-row table
template <typename T, int S, bool FIRST>
int launch_ringc_zip_sf(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);

}  // namespace gcmf

#define GCMF_RINGC_DEFINE(...) template int __VA_ARGS__(gcmf_plan *, const CallView &, const MultiArgs &, const RingcCut &, hipStream_t);
#define GCMF_RINGC_DECLARE(...) extern GCMF_RINGC_DEFINE(__VA_ARGS__)

// XE, PF, LV of launch_ringc_sf
#define GCMF_RINGC_PLAIN false, false, false
#define GCMF_RINGC_SLAB true, false, false
#define GCMF_RINGC_LEVELS false, false, true
#define GCMF_RINGC_BANK false, true, true
#define GCMF_RINGC_GAPS false, true, false
// S levels as a first and as a later launch; LATER: never a first launch (f32 state at eight levels)
#define GCMF_RINGC_SF(X, T, KIND, S, ...) X(launch_ringc_sf<T, KIND, S, true, __VA_ARGS__>) X(launch_ringc_sf<T, KIND, S, false, __VA_ARGS__>)
#define GCMF_RINGC_SF_LATER(X, T, KIND, S, ...) X(launch_ringc_sf<T, KIND, S, false, __VA_ARGS__>)
#define GCMF_RINGC_ZIP(X, S) X(launch_ringc_zip_sf<double, S, true>) X(launch_ringc_zip_sf<double, S, false>)
#define GCMF_RINGC_F64_5TO8(X, KIND, ...) \
  GCMF_RINGC_SF(X, double, KIND, 5, __VA_ARGS__) GCMF_RINGC_SF(X, double, KIND, 6, __VA_ARGS__) GCMF_RINGC_SF(X, double, KIND, 7, __VA_ARGS__) GCMF_RINGC_SF(X, double, KIND, 8, __VA_ARGS__)
#define GCMF_RINGC_F32_5TO8(X, KIND, ...) \
  GCMF_RINGC_SF(X, float, KIND, 5, __VA_ARGS__) GCMF_RINGC_SF(X, float, KIND, 6, __VA_ARGS__) GCMF_RINGC_SF(X, float, KIND, 7, __VA_ARGS__) GCMF_RINGC_SF_LATER(X, float, KIND, 8, __VA_ARGS__)

// one stencil kind, one state type
#define GCMF_RINGC_UNIT_reg(X) GCMF_RINGC_F64_5TO8(X, K_REG, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_reg_f32(X) GCMF_RINGC_F32_5TO8(X, K_REG, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_maskz(X) GCMF_RINGC_F64_5TO8(X, RINGC_MASKZ, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_maskz_f32(X) GCMF_RINGC_F32_5TO8(X, RINGC_MASKZ, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_flux(X) GCMF_RINGC_F64_5TO8(X, K_FLUX, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_flux_f32(X) GCMF_RINGC_F32_5TO8(X, K_FLUX, GCMF_RINGC_PLAIN)
#define GCMF_RINGC_UNIT_flux9(X) GCMF_RINGC_SF(X, double, K_FLUX, 9, GCMF_RINGC_PLAIN)
// the flux kinds with early exits
#define GCMF_RINGC_UNIT_flux_slab(X) GCMF_RINGC_SF(X, double, K_FLUX, 5, GCMF_RINGC_SLAB) GCMF_RINGC_SF(X, double, K_FLUX, 6, GCMF_RINGC_SLAB)
#define GCMF_RINGC_UNIT_flux_slab_b(X) GCMF_RINGC_SF(X, double, K_FLUX, 7, GCMF_RINGC_SLAB) GCMF_RINGC_SF(X, double, K_FLUX, 8, GCMF_RINGC_SLAB)
#define GCMF_RINGC_UNIT_flux_slab_f32(X) GCMF_RINGC_SF(X, float, K_FLUX, 5, GCMF_RINGC_SLAB) GCMF_RINGC_SF(X, float, K_FLUX, 6, GCMF_RINGC_SLAB)
#define GCMF_RINGC_UNIT_flux_slab_f32b(X) GCMF_RINGC_SF(X, float, K_FLUX, 7, GCMF_RINGC_SLAB) GCMF_RINGC_SF_LATER(X, float, K_FLUX, 8, GCMF_RINGC_SLAB)
// stacked plans, filter banks, filter banks over per-field planes
#define GCMF_RINGC_UNIT_levels(X) GCMF_RINGC_SF(X, double, K_FLUX, 9, GCMF_RINGC_LEVELS) GCMF_RINGC_SF(X, double, K_FLUX, 8, GCMF_RINGC_LEVELS)
#define GCMF_RINGC_UNIT_levels_b(X) \
  GCMF_RINGC_SF(X, double, K_FLUX, 7, GCMF_RINGC_LEVELS) GCMF_RINGC_SF(X, double, K_FLUX, 6, GCMF_RINGC_LEVELS) GCMF_RINGC_SF(X, double, K_FLUX, 5, GCMF_RINGC_LEVELS)
#define GCMF_RINGC_UNIT_bank(X) GCMF_RINGC_SF(X, double, K_FLUX, 9, GCMF_RINGC_BANK)
#define GCMF_RINGC_UNIT_bank_b(X) GCMF_RINGC_SF(X, double, K_FLUX, 8, GCMF_RINGC_BANK) GCMF_RINGC_SF(X, double, K_FLUX, 5, GCMF_RINGC_BANK)
#define GCMF_RINGC_UNIT_bank_c(X) GCMF_RINGC_SF(X, double, K_FLUX, 7, GCMF_RINGC_BANK) GCMF_RINGC_SF(X, double, K_FLUX, 6, GCMF_RINGC_BANK)
#define GCMF_RINGC_UNIT_bank_gaps(X) GCMF_RINGC_SF(X, double, K_FLUX, 9, GCMF_RINGC_GAPS)
#define GCMF_RINGC_UNIT_bank_gaps_b(X) GCMF_RINGC_SF(X, double, K_FLUX, 8, GCMF_RINGC_GAPS) GCMF_RINGC_SF(X, double, K_FLUX, 5, GCMF_RINGC_GAPS)
#define GCMF_RINGC_UNIT_bank_gaps_c(X) GCMF_RINGC_SF(X, double, K_FLUX, 7, GCMF_RINGC_GAPS) GCMF_RINGC_SF(X, double, K_FLUX, 6, GCMF_RINGC_GAPS)
// zipped strips
#define GCMF_RINGC_UNIT_zip(X) GCMF_RINGC_ZIP(X, 9)
#define GCMF_RINGC_UNIT_zip_b(X) GCMF_RINGC_ZIP(X, 8)
#define GCMF_RINGC_UNIT_zip_c(X) GCMF_RINGC_ZIP(X, 7)
#define GCMF_RINGC_UNIT_zip_d(X) GCMF_RINGC_ZIP(X, 5) GCMF_RINGC_ZIP(X, 6)

#define GCMF_RINGC_ALL_UNITS(X) \
  GCMF_RINGC_UNIT_reg(X) GCMF_RINGC_UNIT_reg_f32(X) GCMF_RINGC_UNIT_maskz(X) GCMF_RINGC_UNIT_maskz_f32(X) GCMF_RINGC_UNIT_flux(X) GCMF_RINGC_UNIT_flux_f32(X) \
  GCMF_RINGC_UNIT_flux9(X) GCMF_RINGC_UNIT_flux_slab(X) GCMF_RINGC_UNIT_flux_slab_b(X) GCMF_RINGC_UNIT_flux_slab_f32(X) GCMF_RINGC_UNIT_flux_slab_f32b(X) \
  GCMF_RINGC_UNIT_levels(X) GCMF_RINGC_UNIT_levels_b(X) GCMF_RINGC_UNIT_bank(X) GCMF_RINGC_UNIT_bank_b(X) GCMF_RINGC_UNIT_bank_c(X) GCMF_RINGC_UNIT_bank_gaps(X) \
  GCMF_RINGC_UNIT_bank_gaps_b(X) GCMF_RINGC_UNIT_bank_gaps_c(X) GCMF_RINGC_UNIT_zip(X) GCMF_RINGC_UNIT_zip_b(X) GCMF_RINGC_UNIT_zip_c(X) GCMF_RINGC_UNIT_zip_d(X)
