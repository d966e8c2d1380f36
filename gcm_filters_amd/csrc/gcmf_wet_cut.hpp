// The TIGHT cut of k_ringcz's wet-row table (round 8): from a plane of land bytes, a depth and a row range, the x offset of the window grid and
// the pairs of strips (x0, lo, mid, hi) of the launch.  Host arithmetic on bytes -- no device, no plan, no HIP header (standard headers and the
// even cut's planner, gcmf_ringc_cut.hpp, for the window width and the rows a zipped march runs): wet_table (gcmf_ringc_zip.hip) calls it for
// option "wet_rows" 3 and 4, tests/wet_cut/print_wet_cut.cpp compiles it alone.
//
// The table of round 7 (options 1 and 2, wet_table's own code) marches rows the result does not need: every run of needed rows is widened by
// S + 1 rows at both ends although the march reads its S ghost rows beyond a strip's end anyway; a row counts as needed for the wet cells of a
// window's GHOST columns, which the neighbouring window computes; and the window grid is pinned at column 0, so a coast inside a window costs
// the whole window on its land side.  Here:
//   * the window grid starts at column xoff, one of 0, 2, .., WI - 2 (even: a lane's two cells stay 16-byte aligned and on one side of the x
//     seam): window wx owns the columns [xoff + wx WI, min(xoff + (wx + 1) WI, xoff + nx)) mod nx;
//   * row r of window wx is needed iff one of the window's OWNED columns holds a cell that exchanges with a neighbour (bit 0 of its land byte);
//   * runs = the maximal runs of needed rows inside [row_lo, row_hi), not widened; two runs of a window less than S + 1 rows apart are bridged
//     (marching the gap is cheaper than two more strip ends); then a run shorter than 4 rows (a pair is two strips of two) is extended upwards
//     to 4 and shifted down where it would pass row_hi; runs that touch are merged; none is joined across the y wrap;
//   * pairs as in round 7: pairs_of(len, H) = max(1, min(len / 4, ceil(len / 2H))), the smallest H at which all pairs fit the 512 slots, runs
//     cut evenly, pairs ordered by (mid, window);
//   * of all offsets (one with more than 512 runs is out) the one with the smallest march, then the fewest owned window-rows, then the smallest
//     offset.  Once per plan and launch geometry: WI / 2 offsets x windows per row on one running count of the row -- milliseconds.
// Cells no pair owns are isolated; they are never written and are read as ghost cells by the pairs next to them (gcmf_plan::pool_clean).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gcmf_ringc_cut.hpp"

namespace gcmf {

struct WetUnit { int x0, lo, mid, hi; };   // x0: the window's first FOOTPRINT column, xoff + wx WI - M (may be negative: the x wrap)
struct WetCut {
  bool ok = false;          // false: no offset fits (or the shape is not one the table takes) -- the launch keeps the even cut
  int xoff = 0;             // the window grid's first column; a lane owns its cells iff they lie in the window's inner WI columns below nx + xoff
  int H = 0, nstrips = 0;   // the tallest strip; twice the most pairs of one window
  int march = 0;            // rows the launch marches
  long long owned = 0;      // window-rows the pairs own
  std::vector<WetUnit> units;
};

// Round 9: a table march (ringc_march<XO>, gcmf_ringc_impl.hpp) addresses a plane with a uniform base and ONE 32-bit byte offset per lane and
// row, so every byte of a plane -- rows x nx cells of `cell` bytes; batch and level offsets are part of the base -- must lie below 2^32, and
// "one row beyond the last" (the march's wrap test) must still be a 32-bit number of its own: rows nx cell < 2^32.  A launch that does not
// meet this keeps the even cut, as one whose table is refused does.
inline bool table_rows_fit32(long long rows, long long nx, long long cell) {
  if (rows < 1 || nx < 1 || cell < 1) return false;
  const unsigned long long lim = 1ull << 32;
  if ((unsigned long long)nx > lim / (unsigned long long)cell) return false;
  const unsigned long long row = (unsigned long long)nx * (unsigned long long)cell;
  return (unsigned long long)rows <= (lim - 1) / row;   // rows * row <= 2^32 - 1
}
// ... and the march wraps its cursor from one end of the grid to the other, nothing else: beyond a closed end (a row slab, a tripolar grid's
// south) the coefficient rows would have to come from the row of zeros.  No plan that gcmf_apply offers a table to has closed ends today
// (whole grids without a fold wrap); the launcher asks all the same.
inline bool table_rows_ok(long long rows, long long nx, long long cell, bool wraps_in_y) { return wraps_in_y && table_rows_fit32(rows, nx, cell); }

// Round 10: whether a nine-level table launch streams its state planes (ringc_march<NT>).  Per owned cell a later launch reads four constant
// planes and a land byte (33 bytes, the same ones in every launch of every application) and reads and writes two state planes (32 bytes, each
// used once).  The memory-side cache keeps a line while everything moved between two uses of it fits: a launch that moves less than the cache
// holds finds its STATE there too, written by the launch before, and must leave it there -- the default policy; one that moves more finds
// nothing, unless the state passes by without staying and the constants alone (with the ghost rows) fit.  The budget is the cache's size.
constexpr long long STREAM_CACHE_BYTES = 256ll << 20;   // the memory-side cache of an MI355X
constexpr long long STREAM_CELL_BYTES = 65;             // 4 x 8 + 1 constant, 2 x 8 read and 2 x 8 written state
inline bool stream_state_ok(long long owned_cells) {
  return owned_cells > STREAM_CACHE_BYTES / STREAM_CELL_BYTES;   // cells x 65 > budget, for whole cells, without the product
}
// the cells the pairs of a table own: window columns [x0 + M, min(x0 + M + WI, xlim)), rows [lo, hi)
inline long long table_owned_cells(const WetUnit *units, size_t n, int S, int xlim) {
  const int WI = ringc_window(true, S), M = (128 - WI) / 2;
  long long cells = 0;
  for (size_t i = 0; i < n; ++i) {
    const int c0 = units[i].x0 + M, cols = std::min(c0 + WI, xlim) - c0;
    if (cols > 0 && units[i].hi > units[i].lo) cells += (long long)cols * (units[i].hi - units[i].lo);
  }
  return cells;
}

namespace wet_detail {

struct Run { int wx, lo, hi; };

inline int pairs_of(int len, int H) { return std::max(1, std::min(len / 4, (len + 2 * H - 1) / (2 * H))); }

// the runs of one window from its needed rows (need[r - row_lo]), appended to `out`
inline void runs_of(const uint8_t *need, int wx, int row_lo, int row_hi, int S, std::vector<Run> &out) {
  const size_t first = out.size();
  const int n = row_hi - row_lo;
  for (int r = 0; r < n;) {
    if (!need[r]) { ++r; continue; }
    int e = r;
    while (e < n && need[e]) ++e;
    if (out.size() > first && row_lo + r - out.back().hi < S + 1) out.back().hi = row_lo + e;
    else out.push_back({wx, row_lo + r, row_lo + e});
    r = e;
  }
  for (size_t i = first; i < out.size(); ++i) {
    Run &q = out[i];
    if (q.hi - q.lo >= 4) continue;
    q.hi = q.lo + 4;
    if (q.hi > row_hi) { q.lo = std::max(row_lo, row_hi - 4); q.hi = row_hi; }
  }
  // (bridged runs lie S + 1 >= 6 rows apart and an extension moves an end by at most 3, so none touch at the depths offered; kept for any S)
  size_t w = first;
  for (size_t i = first; i < out.size(); ++i) {
    if (w > first && out[i].lo <= out[w - 1].hi) out[w - 1].hi = std::max(out[w - 1].hi, out[i].hi);
    else out[w++] = out[i];
  }
  out.resize(w);
}

}  // namespace wet_detail

// bits: rows x nx land bytes (row-major; bit 0 = the cell exchanges with a neighbour); [row_lo, row_hi): the rows of the launch
inline WetCut wet_cut_tight(const uint8_t *bits, int rows, int nx, int S, int row_lo, int row_hi) {
  using namespace wet_detail;
  WetCut best;
  const int nrows = row_hi - row_lo;
  if (!bits || S < 5 || S > 9 || nx < 2 || (nx % 2) != 0 || row_lo < 0 || row_hi > rows || nrows < 4) return best;
  const int WI = ringc_window(true, S), M = (128 - WI) / 2, nwx = (nx + WI - 1) / WI, noff = WI / 2;
  // need[(o * nwx + wx) * nrows + r]: one pass over the rows, a row's windows are ranges of its running count
  std::vector<uint8_t> need((size_t)noff * nwx * nrows, 0);
  std::vector<int> run((size_t)nx + 1);
  for (int r = 0; r < nrows; ++r) {
    const uint8_t *row = bits + (size_t)(row_lo + r) * nx;
    run[0] = 0;
    for (int i = 0; i < nx; ++i) run[i + 1] = run[i] + (row[i] & 1);
    if (!run[nx]) continue;
    for (int o = 0; o < noff; ++o) {
      for (int wx = 0; wx < nwx; ++wx) {
        const int c0 = 2 * o + wx * WI, len = std::min(c0 + WI, 2 * o + nx) - c0;
        const int a = c0 % nx, b = a + len;
        const int any = b <= nx ? run[b] - run[a] : (run[nx] - run[a]) + run[b - nx];
        need[((size_t)o * nwx + wx) * nrows + r] = any ? 1 : 0;
      }
    }
  }
  std::vector<Run> runs, best_runs;
  int best_h = 0;
  for (int o = 0; o < noff; ++o) {
    runs.clear();
    for (int wx = 0; wx < nwx; ++wx) runs_of(need.data() + ((size_t)o * nwx + wx) * nrows, wx, row_lo, row_hi, S, runs);
    if ((long long)runs.size() > CUT_PAIRS) continue;
    int H = 2;
    for (;; ++H) {   // the smallest strip height at which the pairs of all runs fit one round of the 512 pair slots
      long long tot = 0;
      for (const Run &q : runs) tot += pairs_of(q.hi - q.lo, H);
      if (tot <= CUT_PAIRS) break;
    }
    int tallest = 0;
    long long owned = 0;
    for (const Run &q : runs) {
      const int len = q.hi - q.lo, n = pairs_of(len, H);
      owned += len;
      for (int p = 0; p < n; ++p) {
        const int h = (int)((long long)(p + 1) * len / n) - (int)((long long)p * len / n);
        tallest = std::max(tallest, h - h / 2);
      }
    }
    const int march = (int)ringc_zip_rows(tallest + S + 1, S, nullptr);
    if (best.ok && (march > best.march || (march == best.march && owned >= best.owned))) continue;
    best.ok = true;
    best.xoff = 2 * o;
    best.H = tallest;
    best.march = march;
    best.owned = owned;
    best_h = H;
    best_runs = runs;
  }
  if (!best.ok) return best;
  std::vector<int> per_window(nwx, 0);
  std::vector<Run> cut;   // (wx, lo, hi) of every pair
  for (const Run &q : best_runs) {
    const int len = q.hi - q.lo, n = pairs_of(len, best_h);
    per_window[q.wx] += n;
    for (int p = 0; p < n; ++p) cut.push_back({q.wx, q.lo + (int)((long long)p * len / n), q.lo + (int)((long long)(p + 1) * len / n)});
  }
  auto mid = [](const Run &q) { return q.lo + (q.hi - q.lo) / 2; };
  // neighbours in x side by side, then up the grid: the order in which the even cut numbers its pairs (they share an XCD's L2)
  std::stable_sort(cut.begin(), cut.end(), [&](const Run &p, const Run &q) { return mid(p) != mid(q) ? mid(p) < mid(q) : p.wx < q.wx; });
  best.units.reserve(cut.size());
  for (const Run &q : cut) best.units.push_back({best.xoff + q.wx * WI - M, q.lo, mid(q), q.hi});
  best.nstrips = 2 * (nwx ? *std::max_element(per_window.begin(), per_window.end()) : 0);
  return best;
}

}  // namespace gcmf
