// The launches of a filter bank on a plan that owns the tripole seam: planner inputs with `stacked` set (what ringc_cut_in passes inside
// gcmf_apply_bank), every batch from 1 to 64 and every depth k_fold_band runs, with the zipped forms switched on.  Prints each input with
// the cut ringc_cut() gives it -- twice, with `stacked` and without -- for tests/test_ringc_cut_plain.py to read.  Host only: compiled
// with g++ against csrc/gcmf_ringc_cut.hpp and nothing else.
#include <cstdio>

#include "gcmf_ringc_cut.hpp"

int main() {
  static const char *const form[] = {"none", "k_ringc", "k_ringcs", "k_ringcz", "k_ringcz+fold", "k_ringcp"};
  static const int shapes[][2] = {{96, 160}, {96, 168}, {200, 520}, {2400, 3600}};   // (rows, nx)
  for (const auto &sh : shapes)
    for (long long batch = 1; batch <= 64; ++batch)
      for (int S = 5; S <= 8; ++S)
        for (int beside = 0; beside <= 1; ++beside)
          for (int stacked = 1; stacked >= 0; --stacked) {
            // the plan's defaults: f64 K_FLUX, strip_rows 0, ringc_xe_rows 64, ringc_zip 1, zip_fold 1, pack_batch 1
            gcmf::RingcCutIn in{sh[1], sh[0], true, batch, S, true, gcmf::K_FLUX, beside != 0, false, 0, 64, 1, 1, 1};
            in.stacked = stacked != 0;
            const gcmf::RingcCut c = gcmf::ringc_cut(in);
            printf("%d %d %lld %d %d %d -> %s xe=%d rows=%d grid_y=%u npack=%d fold_rows=%d\n", sh[0], sh[1], batch, S, beside, stacked, form[c.form], c.xe ? 1 : 0,
                   c.rows, c.grid_y, c.npack, c.fold_rows);
          }
  return 0;
}
