// k_ringc<double, K_FLUX, S, FIRST, true, false>: the plain strips of a FILTER BANK OVER PER-FIELD PLANES (gcmf_apply_bank_gaps) -- every batch
// entry marches with the coefficients of its own polynomial, read from a table in device memory, on the input plane, the folded face
// coefficients and the land bytes of its own field (ringc_march<PB, LV>, gcmf_ringc_impl.hpp).  Nine levels here, eight and five in
// gcmf_ringc_bank_gaps_b.hip, seven and six in gcmf_ringc_bank_gaps_c.hip (the instantiations of a unit compile one after the other).
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_bank_gaps(GCMF_RINGC_DEFINE)
}  // namespace gcmf
