// k_ringcz<double> at five and six levels (see gcmf_ringc_zip.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_zip_d(GCMF_RINGC_DEFINE)
}  // namespace gcmf
