// Prints ringc_offered() over every entry form x state type x depth 4..10 x first / later launch, one line each.  Host only: compiled with
// g++ against csrc/gcmf_ringc_cut.hpp and nothing else (tests/test_ringc_table.py).
#include <cstdio>

#include "gcmf_ringc_cut.hpp"

static_assert(gcmf::ringc_offered(gcmf::RINGC_E_FLUX, true, 9, true) && !gcmf::ringc_offered(gcmf::RINGC_E_FLUX, false, 8, true), "usable in constant expressions");

int main() {
  static const char *const form[gcmf::RINGC_E_COUNT] = {"reg", "maskz", "flux", "slab", "zip", "levels", "bank", "bank_gaps"};
  for (int e = 0; e < gcmf::RINGC_E_COUNT; ++e)
    for (int f64 = 1; f64 >= 0; --f64)
      for (int S = 4; S <= 10; ++S)
        for (int first = 1; first >= 0; --first)
          printf("%s %s %d %s %d\n", form[e], f64 ? "f64" : "f32", S, first ? "first" : "later", gcmf::ringc_offered((gcmf::RingcEntry)e, f64 != 0, S, first != 0) ? 1 : 0);
  // (what clenshaw_depth_refused and clenshaw_cut ask)
  for (int S = 4; S <= 10; ++S)
    printf("any %d exists=%d f64=%d%d f32=%d%d\n", S, gcmf::ringc_depth_exists(S) ? 1 : 0, gcmf::ringc_offered_any(true, S, true) ? 1 : 0, gcmf::ringc_offered_any(true, S, false) ? 1 : 0,
           gcmf::ringc_offered_any(false, S, true) ? 1 : 0, gcmf::ringc_offered_any(false, S, false) ? 1 : 0);
  return 0;
}
