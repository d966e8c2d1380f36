// How one launch of the backward scalar kernels (k_ringc, k_ringcs, k_ringcz, k_ringcp, k_ringc_one; gcmf_ringc_impl.hpp) is cut: which form
// runs, strip height, strips per window, pairs, fold strips, runs of a packed batch, the grid.  Integer arithmetic on the launch's shape and
// a few options -- no device, no plan, no HIP header: ringc_cut() is the one place that decides, advance_multi asks it once per launch and
// the launchers apply its answer; the policies that weigh depths against each other (clenshaw_cut, wet_table) ask it too.
#pragma once
#include <algorithm>

namespace gcmf {

// Stencil families.  Every reference Laplacian maps onto one of them after plan-time folding.
enum Kind : int {
  K_REG = 0,   // REGULAR, REGULAR_AREA_WEIGHTED: 5-point, no coefficients              (40 B/cell.step f64)
  K_MASK = 1,  // *_WITH_LAND regular grids + tripolar regular: 1 byte of neighbour bits (41 B)
  K_FLUX = 2,  // IRREGULAR / POP / MOM5U / MOM5T: east-face, north-face, 1/area planes  (64 B)
  K_CGRID = 3, // VECTOR_C_GRID: 14 folded planes
  K_BGRID = 4  // VECTOR_B_GRID: 8 folded planes
};

// one wave per SIMD: 1024 waves march at once, in 256 workgroups of four; k_ringcz's pairs of strips: 512
constexpr long long CUT_WAVES = 1024, CUT_PAIRS = 512, CUT_WGS = 256;
constexpr int CUT_PERIOD = 12;   // rows of a ring period (RingGeom::R): what a march without early exits is a multiple of

// useful columns of a wave's window: 64 lanes x 16 bytes, less S ghost columns (whole lanes' worth) on either side
inline int ringc_window(bool f64, int S) {
  const int vec = f64 ? 2 : 4, M = (S + vec - 1) / vec * vec;
  return 64 * vec - 2 * M;
}

// How many strips a (window, batch entry) column of the one-wave-per-SIMD strip-marching kernels is cut into: ideally as many as fill ONE
// resident round of 1024 waves (all strips march in lock-step) -- a single field at BASELINE size: 33 windows x 31 strips.  Batches do
// not divide that well (33 windows x 16 fields = 528 columns: one strip each left half the SIMDs without a wave -- a batch of 16 ran at
// 515 G against 811 G for a batch of 4 before round 5): the number of rounds k <= 8 is chosen that minimises k x (rows a wave marches:
// H + 2 S, rounded up to the exit period), one round being preferred by 4 % per extra round.  (Also the forward k_ring launcher's.)
inline long long strips_per_column(long long per_strip, long long nrows, int S, int period) {
  if (per_strip < 1) per_strip = 1;
  long long best = 1;
  double best_cost = -1.0;
  for (int k = 1; k <= 8; ++k) {
    long long w = (CUT_WAVES * k) / per_strip;
    if (w < 1) w = 1;
    if (w > nrows) w = nrows;
    const long long H = (nrows + w - 1) / w;
    long long march = H + 2 * S;
    if (period > 1) march = (march + period - 1) / period * period;
    const long long rounds = (w * per_strip + CUT_WAVES - 1) / CUT_WAVES;
    const double cost = (double)(rounds * march) * (1.0 + 0.04 * (rounds - 1));
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = w; }
    if (w >= nrows) break;
  }
  return best;
}

// k_ringcz: rows a zipped march of `need` rows runs -- with early exits: one every second row up to eight levels, every fourth at nine;
// without: whole ring periods (taken when it is no longer: 80 fewer registers, the same time per row -- 1080 x 1440 at eight levels, 24 rows
// either way: 215.2 against 214.7 us)
inline long long ringc_zip_rows(long long need, int S, bool *xe) {
  const long long ex = S <= 8 ? 2 : 4;
  const long long mx = std::max<long long>(CUT_PERIOD, (need + ex - 1) / ex * ex), mp = (need + CUT_PERIOD - 1) / CUT_PERIOD * CUT_PERIOD;
  if (xe) *xe = mx < mp;
  return std::min(mx, mp);
}
// ... and whether its early-exit form runs strips whose tallest is H rows (option ringc_zip: 2 = always, 3 = never); the launcher asks again
// for the height of a wet-row table
inline bool ringc_zip_exits(long long H, int S, int ringc_zip) {
  bool xe = true;
  ringc_zip_rows(H + S + 1, S, &xe);
  return ringc_zip == 2 ? true : ringc_zip == 3 ? false : xe;
}

enum RingcForm : int {
  RINGC_NONE = 0,     // no rows or no fields: nothing to launch
  RINGC_PLAIN,        // k_ringc: whole strips per field (the flux kinds: whole ring periods)
  RINGC_EARLY_EXIT,   // k_ringcs: the flux kinds leaving after every fourth row
  RINGC_ZIP,          // k_ringcz: pairs of strips zipped at a shared seam
  RINGC_ZIP_FOLD,     // ... and strips that start at the tripole seam, zipped with their mirror windows (no k_fold_band)
  RINGC_PACKED        // k_ringcp: the fields of a batch as one column per window, cut into runs
};

// What a launch enters the kernels as: the rows of the dispatch table (launch_ringc, gcmf_ringc_dispatch.hip) ...
enum RingcEntry : int {
  RINGC_E_REG = 0,     // k_ringc / k_ringcp of the REGULAR kinds
  RINGC_E_MASKZ,       // ... of the land-mask kinds (also with one plane of mask bytes per entry, GCMF_MASK_FROM_NAN)
  RINGC_E_FLUX,        // ... of the flux kinds, whole ring periods
  RINGC_E_SLAB,        // the flux kinds with early exits: k_ringcs, k_ringcp's early-exit form
  RINGC_E_ZIP,         // k_ringcz (RINGC_ZIP, RINGC_ZIP_FOLD)
  RINGC_E_LEVELS,      // k_ringc on a stacked plan (gcmf_plan_create_levels)
  RINGC_E_BANK,        // ... of a filter bank (gcmf_apply_bank)
  RINGC_E_BANK_GAPS,   // ... of a filter bank over per-field planes (gcmf_apply_bank_gaps)
  RINGC_E_COUNT
};
constexpr const char *ringc_entry_name(RingcEntry e) {
  constexpr const char *names[RINGC_E_COUNT] = {"regular strips", "land-mask strips", "flux strips", "early-exit flux strips", "zipped strips", "stacked plan",
                                                "filter bank", "filter bank over per-field planes"};
  return e >= 0 && e < RINGC_E_COUNT ? names[e] : "?";
}
// ... and THE statement of which launches exist: an entry form on f64 or f32 state, S levels, as the first launch of an application or a
// later one.  The translation units gcmf_ringc_*.hip instantiate exactly these (gcmf_ringc_table.hpp; tests/test_ringc_table.py), the
// dispatcher refuses everything else, and the policies that cut a polynomial into launches ask here.
//   f64: 5..8 levels everywhere; nine on whole ring periods of the flux kinds and in k_ringcz (the early-exit form of nine was measured and
//   not built, gcmf_ringc_flux9.hip); f32: the four forms that come per stencil kind, and never a first launch of eight levels -- it also
//   carries the land bits of the rows that become b_n and spills there.
constexpr bool ringc_offered(RingcEntry e, bool f64, int S, bool first) {
  if (e < 0 || e >= RINGC_E_COUNT || S < 5 || S > 9) return false;
  const bool per_kind = e <= RINGC_E_SLAB;
  if (!f64) return per_kind && S <= (first ? 7 : 8);
  return S <= 8 || !(e == RINGC_E_REG || e == RINGC_E_MASKZ || e == RINGC_E_SLAB);
}
// some entry form runs S levels on this state type / on any
constexpr bool ringc_offered_any(bool f64, int S, bool first) {
  for (int e = 0; e < RINGC_E_COUNT; ++e)
    if (ringc_offered((RingcEntry)e, f64, S, first)) return true;
  return false;
}
constexpr bool ringc_depth_exists(int S) { return ringc_offered_any(true, S, true) || ringc_offered_any(true, S, false) || ringc_offered_any(false, S, true) || ringc_offered_any(false, S, false); }

struct RingcCutIn {
  int nx, rows;          // columns; rows [row_lo, row_hi) handed to advance_multi ...
  bool seam;             // ... which end at the tripole seam of the plan: fold strips take them all, otherwise k_fold_band takes the top S
  long long batch;
  int S;
  bool f64;              // state type
  int kind;
  bool band_beside;      // k_fold_band runs BESIDE this launch (its waves must fit on the SIMDs next to these: no zip, no early exit)
  bool mask_per_field;   // GCMF_MASK_FROM_NAN: never packed
  int strip_rows, ringc_xe_rows, ringc_zip, zip_fold, pack_batch;   // the plan's options of these names
  bool stacked = false;  // a stacked plan (gcmf_plan_create_levels) or a filter bank (gcmf_apply_bank): whole strips per entry in whole ring periods --
                         // never zipped (nor at the tripole seam: k_fold_band keeps it), packed or with early exits
};

struct RingcCut {
  RingcForm form;
  bool xe;                // k_ringcz / k_ringcp: the early-exit instantiation
  int rows;               // rows the strips own: in.rows, less the S rows of k_fold_band where that advances the seam
  int WI, nwx;            // useful columns of a window, windows
  int H, nstrips;         // strip height (packed: rows of a run), strips per window (packed: runs)
  int pairs;              // k_ringcz: pairs per window below the fold strips
  int fold_rows, nfw;     // k_ringcz's fold strips: the rows they own, window pairs
  int npack;              // k_ringcp: the batch
  unsigned grid_x, grid_y;
  long long march;        // rows a wave slot marches, all rounds
  long long zip_march;    // ... what even zipped pairs without fold strips would march (0: not offered) -- what the policies compare
};

namespace cut_detail {

// pairs per window: whole rounds of the 1024 wave slots, strips of at least two rows; *march = rows the launch marches (all rounds)
inline long long zip_pairs(long long nwx, long long nbatch, long long nrows, int S, long long *march) {
  long long best = 0, best_cost = 0;
  for (int k = 1; k <= 8; ++k) {
    long long np = (CUT_PAIRS * k) / std::max(1LL, nwx * nbatch);
    np = std::min(np, nrows / 4);
    if (np < 1) continue;
    const long long H = (nrows + 2 * np - 1) / (2 * np);                 // the taller strips
    const long long m = ringc_zip_rows(H + S + 1, S, nullptr);
    const long long rounds = (2 * np * nwx * nbatch + CUT_WAVES - 1) / CUT_WAVES;
    const long long cost = rounds * m * (100 + 4 * (rounds - 1));
    if (!best || cost < best_cost) { best = np; best_cost = cost; *march = rounds * m; }
    if (np >= nrows / 4) break;
  }
  return best;
}

// Whole strips per field, or (pack) the packed column where that is cheaper: as many runs per window as fill whole rounds of the 1024 wave
// slots, never longer than a field.  Taken when its rounds x (run + warm-up rows, one field boundary in most runs) beat the whole strips --
// short grids (the 300-row slab of one of 8 ranks, 16 fields: 626-651 -> 708-710 G; tools/measure_batched_scaling.py).
// cost: rows marched x 1.04 per extra round of the wave slots.  exitp: rows between two exits of the march.
struct Strips { long long H, nstrips, npack, march; double cost; };
inline Strips strips(long long nwx, long long nbatch, long long nrows, int S, int exitp, long long strip_rows, bool pack) {
  auto padded = [&](long long m) { return (m + exitp - 1) / exitp * exitp; };
  Strips c{};
  c.H = strip_rows;
  if (c.H <= 0) {
    const long long want = strips_per_column(nwx * nbatch, nrows, S, exitp);
    c.H = std::max(4LL, (nrows + want - 1) / want);   // (short strips for small grids: see k_ring)
    if (exitp == CUT_PERIOD) c.H += (exitp - (c.H + 2 * S) % exitp) % exitp;   // whole periods (no early exit): let the padding carry real rows
  }
  c.H = std::min(c.H, nrows);
  c.nstrips = (nrows + c.H - 1) / c.H;
  const long long rounds_u = (nwx * nbatch * c.nstrips + CUT_WAVES - 1) / CUT_WAVES;
  c.march = rounds_u * padded(c.H + 2 * S);
  c.cost = (double)c.march * (1.0 + 0.04 * (rounds_u - 1));
  if (!pack) return c;
  const long long total = nbatch * nrows, slots = std::max(1LL, CUT_WAVES / nwx);
  for (long long k = 1; k <= 16; ++k) {
    const long long w = std::min(total, slots * k);                 // runs per window
    const long long q = (total + w - 1) / w;                       // rows per run
    if (q > nrows || q > 320) continue;   // (tall runs lose: 2400 x 3600 x 8 fields as 30 runs of 640 rows per window 768 G against 805 G as whole strips)
    const long long rounds = (w * nwx + CUT_WAVES - 1) / CUT_WAVES;
    const bool crosses = (nrows % q) != 0;                          // (runs aligned with the fields cross nothing)
    const long long m = rounds * (padded(q + 2 * S) + (crosses ? padded(2 * S + exitp / 2) : 0));
    const double cost = (double)m * (1.0 + 0.04 * (rounds - 1));
    if (cost < 0.97 * c.cost) { c.cost = cost; c.H = q; c.nstrips = (total + q - 1) / q; c.npack = nbatch; c.march = m; }
    if (w >= total) break;
  }
  return c;
}

// k_ringcz's fold strips: as many pairs below them as fill whole rounds of the 256 CUs together with the fold strips (two units per
// workgroup, pairs and fold strips mixed: 257 workgroups would be two rounds -- config 4 measured 1.32 ms that way against 0.90)
struct Fold { long long rounds, npmax, np, fold_rows, nfw; };
inline Fold fold(long long nx, long long nwx, long long WI, long long nbatch, long long nrows, int S) {
  Fold f{};
  f.nfw = (nx / 2 + WI - 1) / WI;
  long long k = 1;
  for (; k <= 8 && f.npmax < 1; ++k) {
    const long long cap = CUT_WGS * k / std::max(1LL, std::min(nbatch, CUT_WGS * k));   // workgroups per field
    f.npmax = 2 * cap > f.nfw ? (2 * cap - f.nfw) / nwx : 0;                              // (two units per workgroup)
  }
  f.rounds = k - 1;
  f.np = std::max(1LL, std::min(f.npmax, (nrows - S) / 4));
  // (at least S rows: the ghost rows the pairs below march beyond their last row must stay on this side of the seam)
  f.fold_rows = std::max<long long>(S, (nrows + 2 * f.np) / (2 * f.np + 1));
  f.np = std::max(1LL, std::min(f.np, (nrows - f.fold_rows) / 4));
  return f;
}

}  // namespace cut_detail

inline RingcCut ringc_cut(const RingcCutIn &in) {
  using namespace cut_detail;
  const int S = in.S;
  const bool flux = in.kind == K_FLUX;
  RingcCut c{};
  c.WI = ringc_window(in.f64, S);
  c.nwx = (in.nx + c.WI - 1) / c.WI;
  c.rows = in.rows;
  if (in.rows <= 0 || in.batch <= 0) return c;
  long long nrows = in.rows;
  auto zipped = [&](RingcForm form, long long np, long long fold_rows, long long nfw, long long rounds) {
    c.form = form;
    c.pairs = (int)np;
    c.fold_rows = (int)fold_rows;
    c.nfw = (int)nfw;
    c.nstrips = (int)(2 * np);
    c.H = np > 0 ? (int)((nrows - fold_rows + 2 * np - 1) / (2 * np)) : 0;
    c.xe = ringc_zip_exits(std::max(c.H, c.fold_rows), S, in.ringc_zip);
    c.grid_x = (unsigned)((c.nwx * np + nfw + 1) / 2);
    c.grid_y = (unsigned)in.batch;
    c.march = rounds * ringc_zip_rows(std::max(c.H, c.fold_rows) + S + 1, S, nullptr);
    return c;
  };
  if (in.seam) {
    // The tripole seam inside the launch (round 6): the f64 flux kind, a lane's two cells on one side of the row's centre, no packed batch
    // (stacked: never zipped -- a filter bank on a tripolar plan keeps k_fold_band, whose per-entry form advances the seam's rows)
    if (!in.stacked && in.ringc_zip && in.zip_fold && in.f64 && flux && in.strip_rows <= 0 && S >= 5 && S <= 9 && (in.nx % 4) == 0 && in.nx >= 256 &&
        nrows >= 24 && in.batch <= 64) {
      const Fold f = fold(in.nx, c.nwx, c.WI, in.batch, nrows, S);
      bool take = in.batch <= 1 || !in.pack_batch;
      if (!take && f.npmax >= 1) {
        // a batch that may be packed: the fold strips (gridDim.y = the batch) against the packed column + k_fold_band, in rows marched
        // (1080 x 1440 POP, 8 fields: 1167 -> 995 us; 16 fields stay packed: 2126 against 2613 us)
        const long long H = std::max(f.fold_rows, (nrows - f.fold_rows + 2 * f.np - 1) / (2 * f.np));
        const double zip = (double)(f.rounds * ringc_zip_rows(H + S + 1, S, nullptr)) * (1.0 + 0.04 * (f.rounds - 1));
        take = zip <= strips(c.nwx, in.batch, nrows - S, std::min(S, 8), CUT_PERIOD, 0, true).cost;
      }
      if (take) return zipped(RINGC_ZIP_FOLD, f.np, f.fold_rows, f.nfw, f.rounds);
    }
    nrows -= S;   // k_fold_band owns the top S rows
    c.rows = (int)std::max(0LL, nrows);
    if (nrows <= 0) return c;
  }
  bool xe = false;
  if (flux && !in.band_beside && !in.stacked) {
    // Nothing has to fit beside the waves -> the early-exit form (k_ringcs) wherever it shortens the march: the plain form marches whole
    // 12-row ring periods, the early-exit form leaves after every fourth row (and costs ~60 registers: 1.4 % per launch in f64, ~8 % in
    // f32).  1024 lone waves on 1080 x 1440 f64 cells own 14-row strips: 32 rows marched instead of 36, and every SIMD has a wave (330 ->
    // 364 G cell-steps/s, tools/measure_midsize.py); an 8-way slab 28 instead of 36; BASELINE-size f64 grids 96 either way (-> k_ringc),
    // BASELINE-size f32 grids 52 instead of 60 (+4 %), 1080 x 1440 f32 24 either way (-> k_ringc, the early-exit form measured 9 % slower).
    // This first step ESTIMATES the strips -- with the plain form's period, and five and six f64 levels with the windows of seven -- the
    // cut of the form it settles on follows below.
    const int wi = ringc_window(in.f64, in.f64 ? std::max(S, 7) : S);
    const long long nwx_est = (in.nx + wi - 1) / wi, per = nwx_est * in.batch;
    const long long want = strips_per_column(per, nrows, S, CUT_PERIOD);
    const long long H0 = std::min(nrows, std::max(4LL, in.strip_rows > 0 ? (long long)in.strip_rows : (nrows + want - 1) / want));
    const long long need = H0 + 2 * S;
    const long long rows_xe = std::max<long long>(CUT_PERIOD, (need + 3) / 4 * 4), rows_pad = (need + CUT_PERIOD - 1) / CUT_PERIOD * CUT_PERIOD;
    xe = S <= 8 && H0 < in.ringc_xe_rows && rows_xe * 100 <= rows_pad * (in.f64 ? 95 : 90);
    // Round 6: strips zipped in pairs at a shared seam (k_ringcz) march H + S + 1 rows instead of H + 2 S: where strips are as short as
    // their ghost zones (1/4-degree grids: 15 rows behind 2 x 9; the 300-row slab of one of eight ranks: 11 behind 2 x 8) -- and, for
    // less, at BASELINE size (2400 x 3600: 30 strips of 80 rows marching 92 instead of 27 of 90 marching 108: 890.5 against 906 us,
    // same box, alternating; the launch is bound by HBM there)
    long long np = 0, mz = 0;
    if (in.ringc_zip && in.f64 && in.strip_rows <= 0 && S >= 5 && S <= 9) np = zip_pairs(c.nwx, in.batch, nrows, S, &mz);
    c.zip_march = np >= 1 ? mz : 0;
    if (c.zip_march > 0) {
      const long long rounds = (per * ((nrows + H0 - 1) / H0) + CUT_WAVES - 1) / CUT_WAVES;
      // batches: against the better of whole strips per field and the packed column (1/4-degree grids, 2 .. 8 fields: + 3 .. 20 %)
      const bool take = in.batch <= 1 ? mz * 100 <= rounds * (xe ? rows_xe : rows_pad) * 90
                                      : mz * 100.0 <= strips(nwx_est, in.batch, nrows, S, xe ? 4 : CUT_PERIOD, 0, in.pack_batch != 0).cost * 90.0;
      if (take) {
        zipped(RINGC_ZIP, np, 0, 0, 0);
        c.march = mz;
        return c;
      }
    }
  }
  // (GCMF_MASK_FROM_NAN, stacked plans: whole strips per field -- the packed walk has not been run with one plane of mask bytes per
  // entry, nor with coefficient planes per level)
  const bool pack = in.batch > 1 && in.strip_rows <= 0 && in.pack_batch && !in.mask_per_field && !in.stacked && in.batch * nrows < (1LL << 30);
  const Strips st = strips(c.nwx, in.batch, nrows, S, (flux && !xe) ? CUT_PERIOD : 4, in.strip_rows, pack);
  c.form = st.npack > 0 ? RINGC_PACKED : xe ? RINGC_EARLY_EXIT : RINGC_PLAIN;
  c.xe = xe;
  c.H = (int)st.H;
  c.nstrips = (int)st.nstrips;
  c.npack = (int)st.npack;
  c.grid_x = (unsigned)((c.nwx * st.nstrips + 3) / 4);
  c.grid_y = st.npack > 0 ? 1u : (unsigned)in.batch;
  c.march = st.march;
  return c;
}

}  // namespace gcmf
