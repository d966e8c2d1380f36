// k_ringcz<double> at eight levels (see gcmf_ringc_zip.hip)
#include "gcmf_ringc_impl.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_zip_b(GCMF_RINGC_DEFINE)
}  // namespace gcmf
