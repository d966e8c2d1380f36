// k_ringc<double, K_FLUX, S, FIRST, true, true>: the plain strips of a FILTER BANK (gcmf_apply_bank) -- every batch entry marches with
// the coefficients of its own polynomial, read from a table in device memory, on the input plane of its own field (ringc_march<PB>,
// gcmf_ringc_impl.hpp).  Nine levels here, eight and five in gcmf_ringc_bank_b.hip, seven and six in gcmf_ringc_bank_c.hip (the instantiations
// of a unit compile one after the other).
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_bank(GCMF_RINGC_DEFINE)
}  // namespace gcmf
