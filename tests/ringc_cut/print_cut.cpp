// Reads planner inputs (one launch per line, the columns of tests/golden/ringc_cuts.txt before the "->"), prints each with the cut
// ringc_cut() gives it.  Host only: compiled with g++ against csrc/gcmf_ringc_cut.hpp and nothing else (tests/test_ringc_cut.py).
#include <cstdio>

#include "gcmf_ringc_cut.hpp"

int main() {
  static const char *const form[] = {"none", "k_ringc", "k_ringcs", "k_ringcz", "k_ringcz+fold", "k_ringcp"};
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    int nx, rows, seam, S, f64, kind, beside, mpf, strip_rows, xe_rows, zip, zip_fold, pack;
    long long batch;
    if (line[0] == '#' || line[0] == '\n') continue;
    if (sscanf(line, "%d %d %d %lld %d %d %d %d %d %d %d %d %d %d", &nx, &rows, &seam, &batch, &S, &f64, &kind, &beside, &mpf, &strip_rows, &xe_rows, &zip,
               &zip_fold, &pack) != 14) {
      fprintf(stderr, "bad input line: %s", line);
      return 2;
    }
    const gcmf::RingcCutIn in{nx, rows, seam != 0, batch, S, f64 != 0, kind, beside != 0, mpf != 0, strip_rows, xe_rows, zip, zip_fold, pack};
    const gcmf::RingcCut c = gcmf::ringc_cut(in);
    if (c.form == gcmf::RINGC_NONE) {   // (no rows left below the seam's band)
      printf("%d %d %d %lld %d %d %d %d %d %d %d %d %d %d -> none rows=%d\n", nx, rows, seam, batch, S, f64, kind, beside, mpf, strip_rows, xe_rows, zip, zip_fold, pack, c.rows);
      continue;
    }
    printf("%d %d %d %lld %d %d %d %d %d %d %d %d %d %d -> %s xe=%d rows=%d nwx=%d H=%d nstrips=%d pairs=%d fold_rows=%d nfw=%d npack=%d grid=%ux%u zip_march=%lld\n", nx,
           rows, seam, batch, S, f64, kind, beside, mpf, strip_rows, xe_rows, zip, zip_fold, pack, form[c.form], c.xe ? 1 : 0, c.rows, c.nwx, c.H, c.nstrips,
           c.pairs, c.fold_rows, c.nfw, c.npack, c.grid_x, c.grid_y, c.zip_march);
  }
  return 0;
}
