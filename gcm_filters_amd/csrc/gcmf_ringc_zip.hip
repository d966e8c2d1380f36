// k_ringcz<double>: pairs of strips zipped at a shared seam (gcmf_ringc_impl.hpp), nine levels (with early exits and in whole ring periods); eight, seven, six and five: gcmf_ringc_zip_{b,c,d}.hip
#include "gcmf_ringc_impl.hpp"
#include "gcmf_wet_cut.hpp"

namespace gcmf {
GCMF_RINGC_UNIT_zip(GCMF_RINGC_DEFINE)

// Strips cut from the wet rows of each window (round 7).  A quarter to a third of an ocean grid is land in continents many windows wide:
// a (window, strip) tile whose 128 columns hold nothing but isolated cells marches its rows for nothing -- the state there is +-0 at every
// level and k_land_fix writes the result.  Leaving such waves out alone would not shorten the launch (it lasts as long as its tallest
// strip): their wave slots go to the wet part instead.  Per window the rows that hold anything wet (WetProfile, once per plan and window
// width) are widened by S + 1 rows on both ends (across the y wrap where the grid wraps) and merged into runs; every run is cut into
// pairs (lo, mid, hi) of equal height, the height being the smallest at which all pairs of the launch fit ONE round of the 512 pair
// slots.  Same march, same operands for every cell a pair owns; cells no pair owns are isolated, hold +-0 in the state planes
// (gcmf_plan::pool_clean) and get their result from k_land_fix.
// Round 8: options 3 and 4 take the TIGHT cut instead (wet_cut_tight, gcmf_wet_cut.hpp: no widening, rows needed by a window's owned columns
// only, the window grid shifted to the coast); options 1 and 2 keep the rules above and the code below.  Either way a pair goes to the
// device as (x0, lo, mid, hi), x0 = its window's first footprint column.
static bool land_bytes(gcmf_plan *pl, const CallView &cv, std::vector<uint8_t> &bits, hipStream_t s, const char *who, int *rc) {
  bits.resize((size_t)pl->g.rows * pl->g.nx);
  if (hipMemcpyAsync(bits.data(), cv.lbits, bits.size(), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("%s: reading the plan's land bytes back failed: %s", who, hipGetErrorString(hipGetLastError()));
    *rc = GCMF_ERR_HIP;
    return false;
  }
  return true;
}
// the pairs of a table on the device (at least one entry: an all-land grid has none and launches nothing)
static bool upload_units(gcmf_plan *pl, WetTable &nt, const std::vector<int4> &units, int *rc) {
  nt.nunits = (int)units.size();
  const size_t bytes = std::max<size_t>(1, units.size()) * sizeof(int4);
  if (hipMalloc(&nt.dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    nt.dev = nullptr;
    set_error("wet_table: no memory for %zu pairs", units.size());
    *rc = GCMF_ERR_HIP;
    return false;
  }
  pl->owned.push_back(nt.dev);
  if (!units.empty() && hipMemcpy(nt.dev, units.data(), units.size() * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("wet_table: uploading %zu pairs failed: %s", units.size(), hipGetErrorString(hipGetLastError()));
    *rc = GCMF_ERR_HIP;
    return false;
  }
  return true;
}
static const WetProfile *wet_profile(gcmf_plan *pl, const CallView &cv, int WI, hipStream_t s, int *rc) {
  for (const WetProfile &p : pl->wet_prof)
    if (p.WI == WI) return &p;
  // once per plan and window width, on the host: the plan's land bytes come back once (rows x nx bytes), a row's windows are ranges of
  // its running count of cells that exchange with a neighbour (the window's 128 columns: WI owned ones and the ghost columns, across
  // the x wrap)
  const int rows = pl->g.rows, nx = pl->g.nx, nwx = (nx + WI - 1) / WI, M = (128 - WI) / 2;
  std::vector<uint8_t> bits;
  if (!land_bytes(pl, cv, bits, s, "wet_profile", rc)) return nullptr;
  WetProfile p;
  p.WI = WI;
  p.need.assign((size_t)nwx * rows, 0);
  std::vector<int> run((size_t)nx + 1);
  for (int r = 0; r < rows; ++r) {
    const uint8_t *row = bits.data() + (size_t)r * nx;
    run[0] = 0;
    for (int i = 0; i < nx; ++i) run[i + 1] = run[i] + (row[i] & 1);
    for (int wx = 0; wx < nwx; ++wx) {
      int any = 0;
      if (nx <= 128) {
        any = run[nx];
      } else {
        int c0 = (wx * WI - M) % nx;
        if (c0 < 0) c0 += nx;
        const int c1 = c0 + 128;
        any = c1 <= nx ? run[c1] - run[c0] : (run[nx] - run[c0]) + run[c1 - nx];
      }
      p.need[(size_t)wx * rows + r] = any ? 1 : 0;
    }
  }
  pl->wet_prof.push_back(std::move(p));
  return &pl->wet_prof.back();
}

const WetTable *wet_table(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, long long even_march, hipStream_t s, int *rc) {
  *rc = GCMF_OK;
  const Geom &g = pl->g;
  const int S = a.S, rows = g.rows, nrows = a.row_hi - a.row_lo;
  if (!pl->wet_rows || !cv.wet_now || cv.mask_per_field || cv.stacked || cv.n_land <= 0 || !cv.lbits || pl->d.dtype != GCMF_F64 || pl->kind != K_FLUX ||
      g.fold || a.nbatch != 1 || !pl->pool_base || !pl->pool_bytes || !ringc_offered(RINGC_E_ZIP, true, S, a.first != 0) || nrows < 4)
    return nullptr;
  const bool tight = pl->wet_rows >= 3;
  const WetTable *t = nullptr;
  for (const WetTable &c : pl->wet_tabs)
    if (c.S == S && c.row_lo == a.row_lo && c.row_hi == a.row_hi && c.nbatch == a.nbatch && c.tight == tight) t = &c;
  if (!t && tight) {
    // once per plan, launch geometry and cut: the land bytes come back and the host-only planner weighs every offset of the window grid
    // (no profile is kept: each depth of a filter asks once)
    std::vector<uint8_t> bits;
    if (!land_bytes(pl, cv, bits, s, "wet_table", rc)) return nullptr;
    const WetCut cut = wet_cut_tight(bits.data(), rows, g.nx, S, a.row_lo, a.row_hi);
    WetTable nt;
    nt.S = S; nt.row_lo = a.row_lo; nt.row_hi = a.row_hi; nt.nbatch = a.nbatch; nt.tight = true;
    if (cut.ok) {
      std::vector<int4> units;
      units.reserve(cut.units.size());
      for (const WetUnit &u : cut.units) units.push_back(make_int4(u.x0, u.lo, u.mid, u.hi));
      nt.H = cut.H; nt.nstrips = cut.nstrips; nt.march = cut.march; nt.xlim = g.nx + cut.xoff;
      nt.cells = table_owned_cells(cut.units.data(), cut.units.size(), S, nt.xlim);
      if (!upload_units(pl, nt, units, rc)) return nullptr;
    }
    pl->wet_tabs.push_back(nt);
    t = &pl->wet_tabs.back();
  }
  if (!t) {
    const int WI = ringc_window(true, S), nwx = (g.nx + WI - 1) / WI, reach = S + 1;
    const WetProfile *prof = wet_profile(pl, cv, WI, s, rc);
    if (!prof) return nullptr;
    const bool wrap = g.south_wrap && g.north_wrap;
    WetTable nt;
    nt.S = S; nt.row_lo = a.row_lo; nt.row_hi = a.row_hi; nt.nbatch = a.nbatch;
    struct Run { int wx, lo, len; };
    std::vector<Run> runs;
    std::vector<uint8_t> own(nrows);
    bool ok = true;
    for (int wx = 0; wx < nwx && ok; ++wx) {
      const uint8_t *need = prof->need.data() + (size_t)wx * rows;
      std::fill(own.begin(), own.end(), 0);
      for (int r = 0; r < rows; ++r) {
        if (!need[r]) continue;
        for (int d = -reach; d <= reach; ++d) {
          int q = r + d;
          if (wrap) q = ((q % rows) + rows) % rows;
          if (q >= a.row_lo && q < a.row_hi) own[q - a.row_lo] = 1;
        }
      }
      for (int r = 0; r < nrows;) {
        if (!own[r]) { ++r; continue; }
        int e = r;
        while (e < nrows && own[e]) ++e;
        if (e - r < 4) ok = false;   // (a grid shorter than a run)
        runs.push_back({wx, a.row_lo + r, e - r});
        r = e;
      }
    }
    if (ok && runs.size() <= 512) {
      // the smallest strip height at which the pairs of all runs fit one round of the 512 pair slots
      auto pairs_of = [](int len, int H) { return std::max(1, std::min(len / 4, (len + 2 * H - 1) / (2 * H))); };
      int H = 2;
      for (;; ++H) {
        long long tot = 0;
        for (const Run &r : runs) tot += pairs_of(r.len, H);
        if (tot <= 512) break;
      }
      std::vector<int4> units;
      std::vector<int> per_window(nwx, 0);
      for (const Run &r : runs) {
        const int n = pairs_of(r.len, H);
        per_window[r.wx] += n;
        for (int p = 0; p < n; ++p) {
          const int lo = r.lo + (int)((long long)p * r.len / n), hi = r.lo + (int)((long long)(p + 1) * r.len / n), mid = lo + (hi - lo) / 2;
          units.push_back(make_int4(r.wx, lo, mid, hi));
          nt.H = std::max(nt.H, std::max(mid - lo, hi - mid));
        }
      }
      // neighbours in x side by side, then up the grid: the order in which the even cut numbers its pairs (they share an XCD's L2)
      std::stable_sort(units.begin(), units.end(), [](const int4 &p, const int4 &q) { return p.z != q.z ? p.z < q.z : p.x < q.x; });
      nt.nstrips = 2 * (nwx ? *std::max_element(per_window.begin(), per_window.end()) : 0);
      nt.march = (int)ringc_zip_rows(nt.H + S + 1, S, nullptr);
      nt.xlim = g.nx;   // this cut's window grid starts at column 0: window wx's footprint at wx WI - M, ownership below nx
      const int M = (128 - WI) / 2;
      std::vector<WetUnit> owned;
      owned.reserve(units.size());
      for (int4 &u : units) {
        u.x = u.x * WI - M;
        owned.push_back({u.x, u.y, u.z, u.w});
      }
      nt.cells = table_owned_cells(owned.data(), owned.size(), S, nt.xlim);
      if (!upload_units(pl, nt, units, rc)) return nullptr;
    }
    pl->wet_tabs.push_back(nt);
    t = &pl->wet_tabs.back();
  }
  if (!t->dev) return nullptr;
  // the policy of the zipped strips themselves: only where it marches at least 10 % fewer rows than the even cut (RingcCut::march)
  if ((pl->wet_rows == 1 || pl->wet_rows == 3) && (even_march < 1 || (long long)t->march * 100 > even_march * 90)) return nullptr;
  return t;
}
}  // namespace gcmf
