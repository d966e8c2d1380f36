// Internal declarations shared by the libgcmf translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "gcmf.h"
#include "gcmf_ringc_cut.hpp"   // enum Kind, strips_per_column; ringc_cut(): how a backward scalar launch is cut

namespace gcmf {

// internal mode bit on top of GCMF_STEP_FIRST / GCMF_STEP_LAST
constexpr unsigned STEP_LAPL = 0x100u;  // t0 = L(t1) only (gcmf_laplacian)

constexpr int MAX_COEF = 14;

void set_error(const char *fmt, ...);
const char *hip_err_name(hipError_t e);

#define GCMF_HIP(call)                                                                    \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      ::gcmf::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? GCMF_ERR_NO_DEVICE : GCMF_ERR_HIP; \
    }                                                                                     \
  } while (0)

// Device-side view of the slab geometry + coefficient planes, passed by value to kernels.
struct Geom {
  int nx;          // columns (never sharded; x is periodic)
  int rows;        // rows in the slab allocation (owned + ghost)
  int south_wrap;  // row 0's southern neighbour is row rows-1 (single slab, periodic in y)
  int north_wrap;  // row rows-1's northern neighbour is row 0
  int fold;        // row rows-1's northern neighbour is itself mirrored in x (tripole seam)
  int area_weighted;
  const void *coef[MAX_COEF];  // K_FLUX: cE, cN, ra;  K_CGRID: 14;  K_BGRID: 8
  const uint8_t *mbits;        // K_MASK: bit0 wet, bit1 E wet, bit2 W wet, bit3 N wet, bit4 S wet, bits 5-7 their count
  const void *area;            // prepare / finalize plane (area-weighted types)
};

// Arguments of one recurrence step (device pointers, per component).
struct StepArgs {
  const void *t1[2];
  const void *t2[2];
  const void *fb_in[2];
  void *t0[2];
  void *fb_out[2];
  double coef0, coef1, c;
  unsigned mode;
  int fb_is_f32;  // f32 plans only: fbar arrays are f32 (GCMF_OUT_F32)
  int64_t nbatch;
  int row_lo, row_hi;
  int fb_lo;  // scalar kinds: rows < fb_lo leave fbar untouched
  int rpw;    // scalar kinds: rows marched per wave (0 = the plan's / default 2); the tripole band steps use 1
};

// Arguments of one temporally blocked launch: S recurrence steps in one pass (scalar kinds, one component).
struct MultiArgs {
  const void *u0, *v0;      // T_{k-1}, T_{k-2}
  void *uo, *vo;            // T_{k-1+S}, T_{k-2+S}  (must not alias u0 / v0)
  const void *fb_in;
  void *fb_out;
  double pk[9];             // coefficients of the S steps (p[k] .. p[k+S-1]); with `first`: p[1] .. p[S]
  double p0, c;
  int S, first, last, fb_is_f32;
  int64_t nbatch;
  int row_lo, row_hi;
  int land_zero;  // the caller guarantees that isolated (land) cells of u0 and v0 are zero: GCMF_STEP_LAND_ZERO
  int ring_first; // first launch: the caller will overwrite the result of the isolated (land) cells (k_land_fix) or there are
                  // none, so the launch may take them as zero while it loads the field (k_ring<..., FIRST>)
  int lvl;        // backward evaluation (backward_args): the launch's first level, 1-based (0: not told) -- what a filter bank's launch
                  // finds its coefficients by (ringc_march<..., PB>)
};

// Arguments of one S-step vector launch (gcmf_cgrid_stream2.hip / gcmf_bgrid_stream2.hip): T_{k-1}, T_{k-2} -> T_{k+S-2}, T_{k+S-1}.
struct VecMultiArgs {
  const void *u0[2];     // T_{k-1} (u, v)
  const void *uprev[2];  // T_{k-2}             (ignored with `first`)
  void *u1o[2];          // T_{k+S-2} out (must not alias u0 / uprev)
  void *u2o[2];          // T_{k+S-1} out (must not alias u0 / uprev / u1o)
  const void *fb_in[2];
  void *fb_out[2];
  double pk[8];          // p[k] .. p[k+S-1]; with `first`: p[1] .. p[S]
  double p0, c;
  int S, first, last, fb_is_f32;
  int64_t nbatch;
  int row_lo, row_hi;
  int clen;              // backward (Clenshaw) evaluation: u0 / uprev = (b_{k+1}, b_{k+2}) (first: u0 = the input f, uprev unused), fb_in =
                         // the input f, p0 = p_n, pk[t] = coefficient of level t + 1, fb_out = the result (last launch)
};

// Strips cut from the wet rows of each window (k_ringcz, round 7; gcmf_ringc_zip.hip).  need[wx * rows + r]: row r of window wx holds a
// cell that exchanges with a neighbour somewhere in the window's 128 columns (one profile per window width WI).
struct WetProfile {
  int WI = 0;
  std::vector<uint8_t> need;
};
// The pairs of one launch geometry and cut: units = (x0, lo, mid, hi) on the device, x0 = the window's first footprint column; dev == nullptr:
// this geometry keeps the even cut.  tight: the cut of round 8 (gcmf_wet_cut.hpp; options 3 and 4) -- round 7's otherwise (options 1 and 2).
// xlim: a lane owns its cells below this column, nx + the offset of the window grid (round 7's grid starts at column 0).
struct WetTable {
  int S = 0, row_lo = 0, row_hi = 0;
  int64_t nbatch = 0;
  bool tight = false;
  void *dev = nullptr;
  int nunits = 0, H = 0, nstrips = 0, march = 0, xlim = 0;
  long long cells = 0;   // cells the pairs own (table_owned_cells, gcmf_wet_cut.hpp): what stream_state_ok weighs
};

}  // namespace gcmf

struct gcmf_plan {
  gcmf_plan_desc d{};
  int kind = 0;
  int ncomp = 1;
  bool tripolar = false;
  bool area_weighted = false;
  bool dimensional = false;
  bool full = true;  // single slab covering the whole grid
  int64_t rows_alloc = 0, first_owned = 0, rows_owned = 0;
  gcmf::Geom g{};
  std::vector<void *> owned;  // device allocations freed at destroy
  // work buffers of gcmf_apply (grow-only)
  void *work = nullptr;
  size_t work_bytes = 0;
  hipStream_t side = nullptr;           // k_fold_band (the tripole seam rows) runs here, concurrently with the blocked launch
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t stream = nullptr;
  // pipelined host path (batched host arrays): staging slots, upload / download streams, per-slot events
  void *stage = nullptr;
  size_t stage_bytes = 0;
  size_t host_chunk_bytes = 32u << 20;  // per component and chunk; 0 = no pipelining (env GCMF_HOST_CHUNK_MB)
  int host_register = 1;                // page-lock the caller's input during a pipelined call (env GCMF_HOST_REGISTER)
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_cmp[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_busy = nullptr;  // end of the last gcmf_apply that used the plan's work buffers
  bool busy_valid = false;
  bool busy_recorded = false;   // ev_busy already stands behind the last call's work (recorded eagerly: see run_whole_locked)
  hipStream_t busy_stream = nullptr;  // the stream that call ran on
  bool timing = false;
  // gcmf_set_timing(plan, 2): an event pair around every temporally blocked launch of gcmf_apply (the dominant kernel)
  bool timing_detail = false;
  std::vector<hipEvent_t> dom_ev;  // pairs
  std::vector<std::string> dom_name;  // kernel each pair bracketed
  std::string last_launched;          // name of the most recent recurrence kernel launch
  int dom_used = 0;
  float dom_ms = 0.f, dom_min = 0.f, dom_max = 0.f;
  int dom_n = 0;
  // the recurrence kernel with the most steps per launch since gcmf_last_kernel was last read (instrumentation:
  // bench.py ties its HBM-traffic figures to the kernel that actually ran)
  std::string last_kernel;
  int last_kernel_weight = 0;
  std::string last_geom;   // launch geometry of last_kernel (note_kernel)
  float last_ms = 0.f;
  int last_launches = 0;
  int rows_per_wave = 0;
  int xcd_remap = 1;
  int ringc_xe_rows = 64;   // flux plans without a seam: strips shorter than this MAY run the early-exit form k_ringcs (launch_ringc decides; GCMF_RINGC_XE_ROWS=0: never)
  int zigzag = 1;        // k_ringc (flux kinds): neighbouring strips march in opposite directions (GCMF_ZIGZAG=0: all downwards)
  int multi_s = 8;     // steps fused per pass by the temporally blocked kernel (1 = off); 8 measured best
  int strip_rows = 0;  // rows per wave strip of that kernel (0 = auto)
  int prefetch_rows = 0;  // rows of operands in flight per wave (0 = default per S)
  int cgrid_tile = 0;     // 1: force the LDS-tile C-grid kernel instead of the streaming one (A/B testing)
  int cgrid_ring = 1;     // k_cgrid_ring (gcmf_cgrid_ring.hip) for batched f32 levels (0: k_cgrid_stream2c everywhere); env GCMF_CGRID_RING, gcmf_set_option
  int cgrid_ring_smax = 6;  // levels per launch of that kernel (4 / 5 / 6; six since round 6); env GCMF_CGRID_RING_SMAX
  int ring_flux_f32 = 1;    // forward ring kernel for f32 flux-kind state (0: k_flux_multi2 as until round 4); gcmf_set_option
  int cgrid_ring_hmax = 0;  // tallest strip its launcher picks (0 = 96); gcmf_set_option
  int cgrid_ring_ncarry = 0;  // 0: the levels carry their previous row's scaled copies in registers (round 6; six levels: the top two), 1: only the last one (round 5); gcmf_set_option
  // Land kept out of the state (scalar plans; slab-row layout): bit 0 of lbits[cell] = the cell exchanges with a neighbour.
  // A cell that does not (land under a wet mask; a flux-form cell whose four faces are closed) has L = 0 and evolves
  // on its own: gcmf_apply zeroes such cells in the two states the first blocked launch wrote -- NaN on land then never
  // reaches the NaN / inf bookkeeping of the blocked kernels -- and writes their polynomial into the result with
  // k_land_fix at the end.
  const uint8_t *lbits = nullptr;
  int64_t n_land = 0;
  // A STACKED plan (gcmf_plan_create_levels): g.coef[0..2] and lbits hold nlev planes of the whole grid, one after the other, and batch
  // entry b of a gcmf_apply call is filtered with level b % nlev.  Only the plain strips of the backward evaluation know the level axis
  // (k_ringc<..., LV>, k_land_fix): every other schedule, the building blocks and gcmf_laplacian refuse such a plan.
  // g.coef, g.mbits, lbits, n_land, stacked and nlev are written while the plan is created and never again: what a flagged call or a
  // filter bank sees in their place it carries in its own CallView (below).
  bool stacked = false;
  int64_t nlev = 1;
  // GCMF_FACES_FROM_NAN: the most scratch one launch may take for its folded planes (25 bytes per cell and entry); longer batches are cut.
  int gap_scratch_mb = 4096;   // gcmf_set_option "gap_scratch_mb"
  // gcmf_apply_adjoint: F^T = D F D^-1 (gcmf.h).  D is made of planes the plan holds anyway -- ra of the flux kinds, the area of the
  // area-weighted ones -- except on the C-grid, whose folded coefficients hold no plane of area_u or area_v alone: such a plan keeps a copy
  // of both (slab-row layout, two planes more).  The pre-scaled input is one plane of the plan dtype per component and entry of a launch,
  // in the work buffer behind everything else; longer batches are cut so that it stays at or under "adjoint_scratch_mb".
  const void *adj_area[2] = {nullptr, nullptr};
  int adjoint_scratch_mb = 4096;   // gcmf_set_option "adjoint_scratch_mb"
  // gcmf_apply_coarsen (gcmf_coarsen.hip): the weight planes gcmf_coarsen_weights copied ((coarsen_nlev, ny, nx) f64; nullptr: every
  // weight is 1) and the call's own work buffer -- the fine planes of one run of entries, at or under "coarsen_scratch_mb", and with host
  // pointers the staged input and coarse planes (grow-only).  coarsen_mu is held for a whole call, OUTSIDE mu, which the gcmf_apply
  // inside takes run by run.
  void *coarsen_w = nullptr;
  int64_t coarsen_nlev = 0;
  void *coarsen_buf = nullptr;
  size_t coarsen_bytes = 0;
  int coarsen_scratch_mb = 4096;   // gcmf_set_option "coarsen_scratch_mb"
  std::mutex coarsen_mu;
  // gcmf_apply_cov (gcmf_cov.hip): the call's own work buffer -- per pair of a run the three planes the pre pass writes (f', g', f' g';
  // two for a variance) and their three filtered planes, at or under "cov_scratch_mb" (grow-only).  cov_mu is held for a whole call,
  // OUTSIDE mu, like coarsen_mu.
  void *cov_buf = nullptr;
  size_t cov_bytes = 0;
  int cov_scratch_mb = 4096;   // gcmf_set_option "cov_scratch_mb"
  std::mutex cov_mu;
  int zero_land = 1;    // env GCMF_ZERO_LAND=0 turns it off
  int ring = 1;           // env GCMF_RING=0: deep launches stay with k_flux_multi2 / k_scalar_multi
  unsigned *ring_nfb = nullptr;    // device counter behind gcmf_ring_fallbacks (lives behind zero_row)
  const void *zero_row = nullptr;  // nx zeros: what rows beyond a closed boundary read as coefficients / mask bits (k_ring)
  int single_launch = 0;  // whole f64 flux grids: the whole polynomial in ONE persistent launch (k_ringc_one; measured slower); gcmf_set_option / GCMF_SINGLE_LAUNCH
  int pack_batch = 1;     // k_ringc / k_ringcs: the fields of a batch as one column per window (ringc_walk, round 6); gcmf_set_option "pack_batch"
  int ringc_zip = 1;      // f64 flux plans without a tripole seam: k_ringcz where it marches fewer rows (env GCMF_RINGC_ZIP, gcmf_set_option "ringc_zip")
  long long band_seq_cells = 3000000;   // tripolar plans: blocked launches over at most this many cells run k_fold_band AFTER themselves (its 1024-thread form), not beside (env GCMF_BAND_SEQ_CELLS; 0 = never)
  int zip_fold = 1;       // tripolar f64 flux plans, backward evaluation: k_ringcz advances the seam's rows itself (no k_fold_band); gcmf_set_option "zip_fold", env GCMF_ZIP_FOLD
  // Whole f64 flux grids with land, a lone field (round 7): k_ringcz's strips are cut from the rows of each window that hold anything wet
  // (wet_table, gcmf_ringc_zip.hip).  0 off, 1 where that marches at least 10 % fewer rows than the even cut, 2 whenever eligible; 3 and 4
  // (round 8; 3 is the default): the same two policies with the TIGHT cut (gcmf_wet_cut.hpp), whose unowned cells may be direct neighbours
  // of wet ones.  gcmf_set_option "wet_rows".  Cells no strip owns are never written, but they are read as ghost cells (against zero coefficients:
  // harmless while finite), so the four state planes must be finite there: pool_clean says they are (zero-filled once, and the flux
  // kinds' backward launches only ever write +-0 into isolated cells).  What can put a NaN / inf there: a new or regrown work buffer
  // (anything), the one-launch-per-step schedule (k_scalar_step carries a NaN on land through every T_k), and calls whose work layout
  // puts other planes where the pool lies (without the blocked schedules: fbar and the staged host input, NaN on land and all).  The
  // blocked forward schedule zeroes land in its state too, but no schedule is trusted: every one other than sched_backward_scalar on
  // an eligible call clears the flag, and so does a work buffer or layout other than the last call's.
  int wet_rows = 3;
  // Nine-level table launches (round 10): the state planes streamed with the non-temporal policy (ringc_march<NT>), so that the constant
  // planes stay in the memory-side cache from launch to launch.  0 never, 1 where the launch moves more than that cache holds
  // (stream_state_ok, gcmf_wet_cut.hpp; the default), 2 whenever such a launch runs.  gcmf_set_option "stream_state".  Same bits either way.
  int stream_state = 1;
  bool pool_clean = false;
  void *pool_base = nullptr;    // the four state planes of the call that runs now (contiguous) ...
  size_t pool_bytes = 0;        // ... 0: the call has no such pool
  std::vector<gcmf::WetProfile> wet_prof;
  std::vector<gcmf::WetTable> wet_tabs;
  int slab_nines = 0;     // row slabs of f64 flux grids without a tripole seam: nine levels per launch where that saves one (gcmf_set_option "slab_nines"; every rank or none)
  int ringc_smax = 0;     // backward scalar launches: at most this many levels each (5..8; 0 = the default cut: nine where offered, else eight); gcmf_set_option "ringc_smax"
  int ringc9 = 1;         // whole f64 flux-form grids without a tripole seam: up to NINE levels per k_ringc launch (env GCMF_RINGC9, gcmf_set_option "ringc9")
  int clenshaw = 2;       // backward (Clenshaw) evaluation: 0 off, 1 the flux kinds + C-grid, 2 (default since round 4) every kind that has a
                          // backward kernel (f64 REGULAR / land-mask kinds, B-grid too); env GCMF_CLENSHAW.  Per call: GCMF_FORWARD_RECURRENCE
  int clenshaw_f32 = 0;   // backward evaluation also for f32 SCALAR state and the f32 B-grid (round 5: off by default -- an all-f32 Clenshaw
                          // sum is 15-45 x less accurate than the reference's own f32 path (f32 T_k, f64 running sum) on the scalar kinds,
                          // 2-3 x on the B-grid, and the forward kernels reproduce that path bit for bit on the REGULAR / land-mask /
                          // B-grid kinds; the f32 C-grid stays backward: in Reinsch's form it is MORE accurate than the reference's).
                          // GCMF_CLENSHAW_F32=1, gcmf_set_option("clenshaw_f32"), or per call GCMF_BACKWARD_F32.
  void *resident = nullptr;  // state of the on-chip (resident) kernel: exchange planes, tile flags (gcmf_resident.hip)
  unsigned res_lo = 0, res_hi = 0;   // serial numbers of the resident launches of the last gcmf_apply that took that path (0: none pending)
  int last_path = 0;                 // GCMF_PATH_* of the last gcmf_apply
  long long path_count[5] = {0, 0, 0, 0, 0};
  double *dev_p = nullptr;   // p[0..n_steps] of the last filter, for k_land_fix
  size_t dev_p_n = 0;
  std::vector<double> host_p;
  // The coefficient tables of the last FILTER BANK (gcmf_apply_bank, gcmf_apply_bank_gaps), a grow-only cache: bank_stride doubles per
  // polynomial, bank_rev reversed (MultiP::ptab, FoldBandP::ptab) and bank_fwd as given (k_land_fix); bank_host is what both hold
  // (bank_fwd's order).  A bank call points its CallView at the rows it runs (ensure_bank_tables).
  double *bank_rev = nullptr, *bank_fwd = nullptr;
  size_t bank_cap = 0, bank_stride = 0;   // doubles each table holds; doubles per row
  std::vector<double> bank_host;
  std::mutex mu;
};

namespace gcmf {
// The grid and the entry layout as ONE CALL sees them.  Every launcher, predicate and cut that a call reaches reads these from the view
// it is handed, never from the plan, so a call changes nothing on the plan and the C-ABI queries answer for the plan itself at any time.
//   own_view(pl)           the plan's own planes: the building blocks, the slab drivers, gcmf_laplacian, every query, an unflagged gcmf_apply
//   GCMF_MASK_FROM_NAN     mbits = lbits = the call's own mask bytes in the work buffer, one plane per batch entry (the field's own batch
//                          offset addresses them: mask_per_field), n_land says "has land"
//   GCMF_FACES_FROM_NAN    the view of a STACKED plan whose levels are the launch's entries: coef[0..2] and lbits are planes in the work
//                          buffer, folded from the plan's planes and each entry's NaNs (launch_gap_fold), nlev = the launch's batch -- so
//                          the launches are exactly a stacked plan's (launch_ringc_sf<.., LV>, the level form of k_land_fix)
//   a filter bank          bank_n polynomials of one degree on bank_nfield fields: entry e of the call is polynomial e / bank_nfield on field
//                          e % bank_nfield, by the plain strips of the backward evaluation alone (ringc_march<..., PB>, k_land_fix<..., PB>;
//                          on TRIPOLAR_POP_WITH_LAND with k_fold_band<..., PB> on the seam's rows), which read row j of bank_rev / bank_fwd
//                          (bank_stride doubles each) for polynomial j
//   ... on gappy fields    both: one folded level per FIELD (nlev = bank_nfield), launch_ringc_sf<.., PF, !LV> and k_land_fix<.., LV, PB>
// entry0: the index, within the caller's batch, of the first entry of the launch that runs now -- the host pipeline, very long batches and
// the banks cut a call into launches whose boundaries need not be multiples of nlev or bank_nfield.  The kernels take the level of entry y
// of a launch as (entry0 % nlev + y) % nlev and its polynomial and field from entry0 + y.
struct CallView {
  const void *coef[3];          // cE, cN, 1 / area (the flux kinds)
  const uint8_t *mbits, *lbits;
  int64_t n_land;
  int mask_per_field;
  bool stacked;
  int64_t nlev;
  int64_t entry0;
  int bank_n;
  int64_t bank_nfield;
  const double *bank_rev, *bank_fwd;
  size_t bank_stride;
  bool wet_now;                 // the launch belongs to a schedule that may take a wet-row table (sched_backward_scalar)
};
inline CallView own_view(const gcmf_plan *pl) {
  CallView cv{};
  for (int k = 0; k < 3; ++k) cv.coef[k] = pl->g.coef[k];
  cv.mbits = pl->g.mbits;
  cv.lbits = pl->lbits;
  cv.n_land = pl->n_land;
  cv.stacked = pl->stacked;
  cv.nlev = pl->nlev;
  cv.bank_nfield = 1;
  return cv;
}
// the geometry a kernel's parameters are filled from: the plan's, with the view's coefficient planes and mask bytes
inline Geom view_geom(const gcmf_plan *pl, const CallView &cv) {
  Geom g = pl->g;
  for (int k = 0; k < 3; ++k) g.coef[k] = cv.coef[k];
  g.mbits = cv.mbits;
  return g;
}
template <typename T> inline const char *tyname() { return sizeof(T) == 8 ? "double" : "float"; }
// "gcmf::k_ringc<double, 2, 8, true>": a kernel's name with its template arguments as rocprofv3 prints them (bench.py's traffic records and
// the dispatch tests key on these strings)
struct KernelArg {
  std::string text;
  KernelArg(const char *s) : text(s) {}
  KernelArg(int v) : text(std::to_string(v)) {}
  KernelArg(bool b) : text(b ? "true" : "false") {}
};
inline std::string kernel_name(const char *kernel, std::initializer_list<KernelArg> args) {
  std::string name = std::string("gcmf::") + kernel + "<";
  for (const KernelArg &a : args) name += (&a == args.begin() ? "" : ", ") + a.text;
  return name + ">";
}
// note_kernel: name as rocprofv3 prints it (without "void " and the argument list); weight = recurrence steps per launch
// geom: the launch geometry of blocked kernels ("H=.. nstrips=.. nwx=.. xcd=.. grid=..x.. rows=.."), what a PMC traffic
// record of the kernel is only valid for (gcmf_last_kernel_geometry; bench.py load_traffic)
inline void note_kernel(gcmf_plan *pl, const std::string &name, int weight, const std::string &geom = std::string()) {
  pl->last_launched = name;
  if (weight >= pl->last_kernel_weight) {
    pl->last_kernel = name;
    pl->last_kernel_weight = weight;
    pl->last_geom = geom;
  }
}
inline std::string launch_geom(int H, int nstrips, int nwx, int xcd, unsigned gx, unsigned gy, int nrows) {
  char b[160];
  snprintf(b, sizeof b, "H=%d nstrips=%d nwx=%d xcd=%d grid=%ux%u rows=%d", H, nstrips, nwx, xcd, gx, gy, nrows);
  return b;
}
size_t dtype_size(int dtype);
// kernel launchers (defined in gcmf_scalar.hip / gcmf_vector.hip)
int launch_scalar_step(gcmf_plan *pl, const CallView &cv, const StepArgs &a, hipStream_t s);
int launch_vector_step(gcmf_plan *pl, const StepArgs &a, hipStream_t s);
int launch_scalar_multi(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, hipStream_t s);
bool flux_multi2_supported(const gcmf_plan *pl, int S);
bool ring_supported(const gcmf_plan *pl, const CallView &cv, const MultiArgs &a);
int launch_ring_flux_f32(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, hipStream_t s);   // gcmf_ring_flux_f32.hip
// backward (Clenshaw) evaluation, gcmf_ringc_impl.hpp: one launch of S = 5..9 levels; a.fb_in = the constant input f, a.fb_out =
// the result (last launch), a.pk[t] = the coefficient of level t + 1 of this launch; cut = ringc_cut()'s answer for the launch
// (gcmf_ringc_cut.hpp), which the launchers apply: advance_multi asks once, and launch_ringc (gcmf_ringc_dispatch.hip) maps the launch to
// its instantiation -- the one place that does; what has none is GCMF_ERR_INVALID_ARG with the form, state type and depth in the error text
inline RingcCutIn ringc_cut_in(const gcmf_plan *pl, const CallView &cv, int rows, bool seam, int64_t nbatch, int S, bool band_beside) {
  return RingcCutIn{pl->g.nx, rows, seam, (long long)nbatch, S, pl->d.dtype == GCMF_F64, pl->kind, band_beside, cv.mask_per_field != 0,
                    pl->strip_rows, pl->ringc_xe_rows, pl->ringc_zip, pl->zip_fold, pl->pack_batch, cv.stacked || cv.bank_n > 0};
}
int launch_ringc(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s);
// k_ringcz's pairs cut from the wet rows of each window (round 7): the table of this launch geometry (built once, cached on the plan), or
// nullptr where the launch keeps the even cut (not eligible, the policy of option "wet_rows" against the even cut's march, or an error --
// then *rc says which)
const WetTable *wet_table(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, long long even_march, hipStream_t s, int *rc);
int launch_flux_multi2(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, hipStream_t s);
// the on-chip kernel (gcmf_resident.hip; the plan's own view only): L <= 64 levels of the backward evaluation in ONE launch on a field that fits the register
// files + LDS of the chip (short slabs, small grids); pk = the L coefficients (a.S / a.pk are ignored)
bool resident_supported(const gcmf_plan *pl, int row_lo, int row_hi, int L, int n_total, int *why = nullptr);   // fits AND the policy says so (n_total: levels of the whole filter; why: GCMF_RESIDENT_* when not)
bool resident_fits(const gcmf_plan *pl, int row_lo, int row_hi, int L);
int launch_resident(gcmf_plan *pl, const MultiArgs &a, const double *pk, int L, hipStream_t s);
void resident_free(gcmf_plan *pl);
bool resident_take_failure(int dev, unsigned lo, unsigned hi);   // did one of the resident launches with serials [lo, hi] time out?  (reported once)
void resident_status(int dev, int *state, unsigned long long *failures);
// another persistent kernel of this process (k_ringc_one): under the on-chip lock, chained behind the process's other persistent launches;
// launch(flags, fail word (device address of mapped host memory), serial, first value of the arrival counter flags[1001]); nbar = arrivals it adds
int resident_persistent_launch(int dev, hipStream_t s, unsigned nbar, const std::function<int(unsigned *, unsigned *, unsigned, unsigned)> &launch);
// the whole polynomial of a whole f64 flux grid in ONE launch (gcmf_ringc_one.hip; opt-in): levels per pass (0: not this application)
int ringc_one_depth(const gcmf_plan *pl, int n_steps, int64_t nbatch);
int launch_ringc_one(gcmf_plan *pl, int S, const double *p, int n_steps, double c, const void *f, void *out, void *const *pool, hipStream_t s);
int launch_cgrid_stream(gcmf_plan *pl, const StepArgs &a, hipStream_t s);
bool cgrid_stream_supported(const gcmf_plan *pl, const StepArgs &a);
int launch_bgrid_stream(gcmf_plan *pl, const StepArgs &a, hipStream_t s);
bool bgrid_stream_supported(const gcmf_plan *pl, const StepArgs &a);
bool multi_supported(const gcmf_plan *pl, int S);
bool cgrid_multi_supported(const gcmf_plan *pl, int64_t nbatch, int S, bool backward = false);   // (backward: k_cgrid_ring's deeper launches count)
int launch_cgrid_multi(gcmf_plan *pl, const VecMultiArgs &a, hipStream_t s);
// the static-ring form of the backward C-grid kernel (gcmf_cgrid_ring.hip): batched f32 levels, S = 4 .. 8
bool cgrid_ring_supported(const gcmf_plan *pl, int64_t nbatch, int S);
bool cgrid_ring_args_aligned(const VecMultiArgs &a);   // the caller's state / input / result planes on 16-byte boundaries
int cgrid_ring_smax(const gcmf_plan *pl, int64_t nbatch);   // deepest launch it offers this plan / batch (0: none)
int launch_cgrid_ring(gcmf_plan *pl, const VecMultiArgs &a, hipStream_t s);
// ... and of the forward recurrence with an f64 running sum (gcmf_cgrid_ringf.hip: Filter(evaluation="reference") on batched f32 levels)
bool cgrid_ringf_supported(const gcmf_plan *pl, const VecMultiArgs &a);
int launch_cgrid_ringf(gcmf_plan *pl, const VecMultiArgs &a, hipStream_t s);
bool bgrid_multi_supported(const gcmf_plan *pl, int64_t nbatch, int S);
int launch_bgrid_multi(gcmf_plan *pl, const VecMultiArgs &a, hipStream_t s);
inline bool vec_multi_supported(const gcmf_plan *pl, int64_t nbatch, int S, bool backward = false) {
  return pl->kind == K_CGRID ? cgrid_multi_supported(pl, nbatch, S, backward) : bgrid_multi_supported(pl, nbatch, S);
}
inline int launch_vec_multi(gcmf_plan *pl, const VecMultiArgs &a, hipStream_t s) {
  return pl->kind == K_CGRID ? launch_cgrid_multi(pl, a, s) : launch_bgrid_multi(pl, a, s);
}
// S fused steps on rows [row_lo,row_hi) incl. the tripole band when the range ends at the fold row (gcmf_api.hip)
// backward: m = the arguments of a k_ringc launch (the polynomial evaluated backwards)
int advance_multi(gcmf_plan *pl, const CallView &cv, const MultiArgs &m, hipStream_t s, int *launches, bool backward = false);
// the tripole seam rows of an S-step launch in one launch (gcmf_foldband.hip)
bool fold_band_supported(const gcmf_plan *pl, const MultiArgs &a);
int launch_fold_band(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, bool backward, hipStream_t s, bool wide = false);
int launch_prepare(gcmf_plan *pl, const void *const *in, void *const *out, int64_t nbatch, int row_lo,
                   int row_hi, hipStream_t s);
// gcmf_apply_adjoint's two passes (gcmf_scalar.hip, forms of k_prepare): pre (post = false) in -> out = in / D, both of the plan dtype;
// post: `out` times D in place, of the output type (f64, or f32 with out_f32 on an f32 plan).  D and the land bytes are the view's (the
// level of a stacked plan, the folded planes of a flagged call); like: null or the forward call's input planes (plan dtype) -- a NaN
// there gives 0, or NaN itself with nan_gaps (the pre-scale of a flagged call, whose gaps the schedule must see)
int launch_adjoint_scale(gcmf_plan *pl, const CallView &cv, bool post, const void *const *in, void *const *out, const void *const *like,
                         bool out_f32, bool nan_gaps, int64_t nbatch, hipStream_t s);
// the isolated cells' own polynomial, written over out (gcmf_landfix.hip); dp = p[0..n_steps] on the device
int launch_zero_land(gcmf_plan *pl, const CallView &cv, void *a, void *b, int64_t nbatch, hipStream_t s, int row_lo = 0, int row_hi = 0);
int launch_land_fix(gcmf_plan *pl, const CallView &cv, const void *in, void *out, const double *dp, int n_steps, double c, int fb_is_f32,
                    int64_t nbatch, hipStream_t s);
// ... of a filter bank (gcmf_apply_bank): entry e of the launch's nbatch, counted from cv.entry0, is row e / bank_nfield of cv.bank_fwd
// on field e % bank_nfield of `in`
int launch_land_fix_bank(gcmf_plan *pl, const CallView &cv, const void *in, void *out, int n_steps, double c, int64_t nbatch, hipStream_t s);
// plan-time precompute (gcmf_precompute.hip): fills pl->g from the raw global planes (device pointers)
int precompute(gcmf_plan *pl, const void *const *dplanes, const void *const *hplanes_or_null);
// ... of a stacked plan (f64 flux kinds without a seam, whole grid): plane k holds plane_levels[k] (1 or pl->nlev) planes
int precompute_levels(gcmf_plan *pl, const void *const *dplanes, const int64_t *plane_levels);
// GCMF_MASK_FROM_NAN: the mask bytes of every entry of a batch, from the plan's own bytes `wet` and the entries' NaNs (k_pre_mask)
int launch_field_masks(gcmf_plan *pl, const uint8_t *wet, const void *fields, uint8_t *bits, int64_t nbatch, hipStream_t s);
// GCMF_FACES_FROM_NAN: the coefficient planes and land bytes of every entry of a batch of f64 fields, from an ordinary flux plan's own
// planes (cE, cN, ra) and the entries' NaNs (k_pre_isolated<double, true, MOM5>, gcmf_gap_fold.hpp); nx must be a multiple of 4
int launch_gap_fold(gcmf_plan *pl, const double *cE, const double *cN, const double *ra, const void *fields, double *cEo, double *cNo,
                    double *rao, uint8_t *bits, int64_t nbatch, hipStream_t s);
// helpers of the calls that wrap gcmf_apply between passes of their own (gcmf_coarsen.hip, gcmf_cov.hip)
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// Such a call's scratch is the plan's, shared by all calls like the work buffers of gcmf_apply: a call on ANOTHER stream than the plan's
// last one orders itself behind it before it touches the scratch (gcmf_apply does the same for its own buffers, gcmf_api.hip).
inline int order_behind_last_call(gcmf_plan *pl, hipStream_t s) {
  std::lock_guard<std::mutex> lk(pl->mu);
  if (pl->busy_valid && pl->busy_stream != s) {
    if (pl->busy_recorded || hipEventRecord(pl->ev_busy, pl->busy_stream) == hipSuccess) {
      GCMF_HIP(hipStreamWaitEvent(s, pl->ev_busy, 0));
    } else {
      (void)hipGetLastError();
      GCMF_HIP(hipDeviceSynchronize());
    }
  }
  return GCMF_OK;
}

}  // namespace gcmf
