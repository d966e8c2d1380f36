// k_ringcz<double> at seven levels (see gcmf_ringc_zip.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_zip_c(GCMF_RINGC_DEFINE)
}  // namespace gcmf
