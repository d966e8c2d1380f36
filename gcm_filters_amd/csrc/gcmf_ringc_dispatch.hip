// launch_ringc: the one place that maps a launch of the backward strip kernels to its instantiation.  Which instantiations exist is
// ringc_offered() (gcmf_ringc_cut.hpp); where each is compiled is gcmf_ringc_table.hpp, whose rows this unit sees as explicit
// instantiation declarations -- it holds no kernel, on either side.
#include "gcmf_ringc_table.hpp"

#include <type_traits>

namespace gcmf {

GCMF_RINGC_ALL_UNITS(GCMF_RINGC_DECLARE)

namespace {

using Launcher = int (*)(gcmf_plan *, const CallView &, const MultiArgs &, const RingcCut &, hipStream_t);

template <RingcEntry E, bool F64, int S, bool FIRST> constexpr Launcher instantiation() {
  if constexpr (!ringc_offered(E, F64, S, FIRST)) {
    return nullptr;
  } else if constexpr (E == RINGC_E_ZIP) {
    return &launch_ringc_zip_sf<double, S, FIRST>;
  } else {
    constexpr int KIND = E == RINGC_E_REG ? (int)K_REG : E == RINGC_E_MASKZ ? RINGC_MASKZ : (int)K_FLUX;
    constexpr bool PF = E == RINGC_E_BANK || E == RINGC_E_BANK_GAPS, LV = E == RINGC_E_LEVELS || E == RINGC_E_BANK;
    return &launch_ringc_sf<std::conditional_t<F64, double, float>, KIND, S, FIRST, E == RINGC_E_SLAB, PF, LV>;
  }
}
template <RingcEntry E, bool F64, bool FIRST> Launcher by_depth(int S) {
  switch (S) {
    case 5: return instantiation<E, F64, 5, FIRST>();
    case 6: return instantiation<E, F64, 6, FIRST>();
    case 7: return instantiation<E, F64, 7, FIRST>();
    case 8: return instantiation<E, F64, 8, FIRST>();
    case 9: return instantiation<E, F64, 9, FIRST>();
  }
  return nullptr;
}
template <RingcEntry E> Launcher row(bool f64, int S, bool first) {
  if (f64) return first ? by_depth<E, true, true>(S) : by_depth<E, true, false>(S);
  return first ? by_depth<E, false, true>(S) : by_depth<E, false, false>(S);
}

}  // namespace

int launch_ringc(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  if (cut.form == RINGC_NONE) return GCMF_OK;
  const bool f64 = pl->d.dtype == GCMF_F64, first = a.first != 0, zip = cut.form == RINGC_ZIP || cut.form == RINGC_ZIP_FOLD;
  RingcEntry e = RINGC_E_COUNT;
  switch (pl->kind) {
    case K_REG: e = RINGC_E_REG; break;
    case K_MASK: e = RINGC_E_MASKZ; break;
    case K_FLUX:
      // (gcmf_apply_bank, and gcmf_apply_bank_gaps whose view is stacked, one level per field; these and the stacked plans: always the
      // plain strips, ringc_cut)
      e = zip ? RINGC_E_ZIP : cv.bank_n > 0 ? (cv.stacked ? RINGC_E_BANK_GAPS : RINGC_E_BANK) : cv.stacked ? RINGC_E_LEVELS : cut.xe ? RINGC_E_SLAB : RINGC_E_FLUX;
      break;
    default: break;
  }
  if (e == RINGC_E_COUNT || (zip && e != RINGC_E_ZIP)) {
    set_error(zip ? "k_ringcz: plan is not a flux kind" : "k_ringc: plan is not a scalar kind");
    return GCMF_ERR_INVALID_ARG;
  }
  Launcher fn = nullptr;
  switch (e) {
    case RINGC_E_REG: fn = row<RINGC_E_REG>(f64, a.S, first); break;
    case RINGC_E_MASKZ: fn = row<RINGC_E_MASKZ>(f64, a.S, first); break;   // (with one plane of mask bytes per entry: the launcher picks the kernel)
    case RINGC_E_FLUX: fn = row<RINGC_E_FLUX>(f64, a.S, first); break;
    case RINGC_E_SLAB: fn = row<RINGC_E_SLAB>(f64, a.S, first); break;
    case RINGC_E_ZIP: fn = row<RINGC_E_ZIP>(f64, a.S, first); break;
    case RINGC_E_LEVELS: fn = row<RINGC_E_LEVELS>(f64, a.S, first); break;
    case RINGC_E_BANK: fn = row<RINGC_E_BANK>(f64, a.S, first); break;
    case RINGC_E_BANK_GAPS: fn = row<RINGC_E_BANK_GAPS>(f64, a.S, first); break;
    default: break;
  }
  if (!fn) {   // (exactly where ringc_offered says no: instantiation())
    set_error("backward strips (%s, %s state): %d levels as %s launch are not offered", ringc_entry_name(e), f64 ? "f64" : "f32", a.S, first ? "a first" : "a later");
    return GCMF_ERR_INVALID_ARG;
  }
  return fn(pl, cv, a, cut, s);
}

}  // namespace gcmf
