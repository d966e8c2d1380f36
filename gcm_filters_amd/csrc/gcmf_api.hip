// libgcmf C ABI: plan lifetime, the whole-polynomial apply loop and the per-step building blocks.
// See include/gcmf.h for the contract and the reference interfaces each entry point replaces.
#include "gcmf_api_internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace gcmf {

static thread_local std::string g_err = "";

void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

size_t dtype_size(int dtype) { return dtype == GCMF_F64 ? 8 : 4; }

struct GridInfo {
  int nplanes, ncomp, dimensional, tripolar, area_weighted, kind;
};
static bool grid_info(int gt, GridInfo &gi) {
  switch (gt) {
    case GCMF_REGULAR: gi = {0, 1, 0, 0, 0, K_REG}; return true;
    case GCMF_REGULAR_AREA_WEIGHTED: gi = {1, 1, 0, 0, 1, K_REG}; return true;
    case GCMF_REGULAR_WITH_LAND: gi = {1, 1, 0, 0, 0, K_MASK}; return true;
    case GCMF_REGULAR_WITH_LAND_AREA_WEIGHTED: gi = {2, 1, 0, 0, 1, K_MASK}; return true;
    case GCMF_IRREGULAR_WITH_LAND: gi = {8, 1, 1, 0, 0, K_FLUX}; return true;
    case GCMF_MOM5U: gi = {6, 1, 1, 0, 0, K_FLUX}; return true;
    case GCMF_MOM5T: gi = {6, 1, 1, 0, 0, K_FLUX}; return true;
    case GCMF_TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED: gi = {2, 1, 0, 1, 1, K_MASK}; return true;
    case GCMF_TRIPOLAR_POP_WITH_LAND: gi = {6, 1, 1, 1, 0, K_FLUX}; return true;
    case GCMF_VECTOR_C_GRID: gi = {14, 2, 1, 0, 0, K_CGRID}; return true;
    case GCMF_VECTOR_B_GRID: gi = {8, 2, 1, 0, 0, K_BGRID}; return true;
  }
  return false;
}


static int ensure_work(gcmf_plan *pl, size_t bytes) {
  if (bytes <= pl->work_bytes) return GCMF_OK;
  if (pl->work) {
    GCMF_HIP(hipFree(pl->work));
    pl->work = nullptr;
    pl->work_bytes = 0;
  }
  GCMF_HIP(hipMalloc(&pl->work, bytes));
  pl->work_bytes = bytes;
  pl->pool_clean = false;   // (new planes hold anything)
  return GCMF_OK;
}

static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Page-locked caller ranges, process wide and reference counted: two plans (two dask threads) may stream the same host
// array at once, and the first to finish must not unregister it under the other's transfers.
static std::mutex g_reg_mu;
static std::map<const void *, std::pair<size_t, int>> g_reg;
static bool host_register(const void *p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.find(p);
  if (it != g_reg.end()) {
    if (it->second.first < bytes) return false;  // a shorter range is locked: leave this call on the pageable path
    ++it->second.second;
    return true;
  }
  if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  g_reg[p] = {bytes, 1};
  return true;
}
static void host_unregister(const void *p) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  auto it = g_reg.find(p);
  if (it == g_reg.end()) return;
  if (--it->second.second == 0) {
    (void)hipHostUnregister(const_cast<void *>(p));
    g_reg.erase(it);
  }
}



// One temporally blocked advance of S steps on rows [row_lo, row_hi) of a scalar plan.
//
// Tripolar grids: the fold couples column i of the top row with column nx-1-i, i.e. with a DIFFERENT wave of the
// strip-marching kernel, which therefore stops S rows below the seam; the top S rows ("band") are advanced by k_fold_band.
// backward: launch_ringc (gcmf_ringc_dispatch.hip) runs the form ringc_cut chose for this launch (gcmf_ringc_cut.hpp has the policy and its measurements)
int advance_multi(gcmf_plan *pl, const CallView &cv, const MultiArgs &m, hipStream_t s, int *launches, bool backward) {
  const Geom &g = pl->g;
  const int rows = g.rows, S = m.S;
  const bool band = g.fold && m.row_hi == rows;
  int rc;
  RingcCut cut{};
  auto blocked = [&](const MultiArgs &a) -> int {   // (between the dominant kernel's timing events)
    int r;
    if ((r = dom_begin(pl, s)) || (r = backward ? launch_ringc(pl, cv, a, cut, s) : launch_scalar_multi(pl, cv, a, s)) || (r = dom_end(pl, s))) return r;
    if (launches) ++*launches;
    return GCMF_OK;
  };
  // Short launches on the seam's plan (round 6): the band AFTER the blocked launch, in its stream, 1024 threads per tile.  Beside a launch
  // that lasts no longer than itself the band is the slower of the two (its waves share the SIMDs with the marching waves) and the fork /
  // join costs ~5 us on top: a 1080 x 1440 tripolar grid took 294 us against 215 us for the same grid without a seam.
  const bool seq = band && pl->band_seq_cells > 0 && (long long)m.nbatch * (m.row_hi - m.row_lo) * g.nx <= pl->band_seq_cells;
  // how the strips of a backward launch are cut: decided once, here (on the seam's plan: of the rows k_fold_band leaves, or -- round 6 --
  // the seam's rows inside the launch: strips that start at the seam, zipped with their mirror windows)
  if (backward) cut = ringc_cut(ringc_cut_in(pl, cv, m.row_hi - m.row_lo, band, m.nbatch, S, band && !seq));
  if (!band || cut.form == RINGC_ZIP_FOLD) return blocked(m);
  const int blo = rows - S;  // first band row
  // k_fold_band reads rows [rows - 2S, rows) of the input planes (valid: the caller's ghost zone covers [row_lo - S, ...)) and owns
  // [rows - S, rows); the blocked launch gets [row_lo, rows - S), possibly nothing
  if (m.row_lo > blo || rows < 2 * S) {
    set_error("advance_multi: row range [%d, %d) too short for the tripole band of %d rows", m.row_lo, m.row_hi, S);
    return GCMF_ERR_INVALID_ARG;
  }
  MultiArgs mm = m;
  mm.row_hi = blo;
  if (!fold_band_supported(pl, m)) {
    set_error("advance_multi: k_fold_band does not cover this plan / depth %d / batch %lld", S, (long long)m.nbatch);
    return GCMF_ERR_UNSUPPORTED;
  }
  // The seam rows in ONE launch (k_fold_band, gcmf_foldband.hip) on a side stream beside the blocked launch: neither reads what
  // the other writes (the band reads rows >= rows - 2S of the input planes, the two write disjoint rows of the output planes).
  if (seq) {
    if (mm.row_hi > mm.row_lo && (rc = blocked(mm))) return rc;
    if ((rc = launch_fold_band(pl, cv, m, backward, s, true))) return rc;
    if (launches) ++*launches;
    return GCMF_OK;
  }
  if (!pl->side) {
    // both streams are on this device and nothing between fork and join is read by the host or a peer: no system-scope
    // fence on these events (agent scope orders the two queues; measured +2 % on config 4: the fork / join packets are
    // the only cost the seam has left, ~6 us per launch)
    const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    GCMF_HIP(hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking));
    GCMF_HIP(hipEventCreateWithFlags(&pl->ev_fork, evf));
    GCMF_HIP(hipEventCreateWithFlags(&pl->ev_join, evf));
  }
  GCMF_HIP(hipEventRecord(pl->ev_fork, s));
  GCMF_HIP(hipStreamWaitEvent(pl->side, pl->ev_fork, 0));
  if ((rc = launch_fold_band(pl, cv, m, backward, pl->side))) return rc;
  if (launches) ++*launches;
  GCMF_HIP(hipEventRecord(pl->ev_join, pl->side));
  if (mm.row_hi > mm.row_lo && (rc = blocked(mm))) return rc;
  GCMF_HIP(hipStreamWaitEvent(s, pl->ev_join, 0));
  return GCMF_OK;
}

int step_dispatch(gcmf_plan *pl, const CallView &cv, const StepArgs &a, hipStream_t s) {
  return pl->ncomp == 1 ? launch_scalar_step(pl, cv, a, s) : launch_vector_step(pl, a, s);   // (the vector kinds have no view but the plan's own)
}

// p[0..n_steps] on the device for k_land_fix; uploaded only when it changed (a pageable upload stalls the host behind
// the stream)
static int ensure_dev_p(gcmf_plan *pl, const double *p, int n_steps, hipStream_t s) {
  const size_t n = (size_t)n_steps + 1;
  if (pl->dev_p_n < n) {
    if (pl->dev_p) GCMF_HIP(hipFree(pl->dev_p));
    pl->dev_p = nullptr;
    pl->dev_p_n = 0;
    pl->host_p.clear();
    GCMF_HIP(hipMalloc((void **)&pl->dev_p, n * sizeof(double)));
    pl->dev_p_n = n;
  }
  if (pl->host_p.size() != n || memcmp(pl->host_p.data(), p, n * sizeof(double)) != 0) {
    pl->host_p.assign(p, p + n);
    GCMF_HIP(hipStreamSynchronize(s));  // nothing may still read the old coefficients
    GCMF_HIP(hipMemcpy(pl->dev_p, pl->host_p.data(), n * sizeof(double), hipMemcpyHostToDevice));
  }
  return GCMF_OK;
}

// The land-fix tail of a filter whose launches kept the isolated (land) cells out of their state: their own polynomial, from the
// untouched input `in` into `out` (k_land_fix)
int land_fix_tail(gcmf_plan *pl, const CallView &cv, const double *p, int n_steps, double c, const void *in, void *out, bool fb32,
                  int64_t nbatch, hipStream_t s) {
  int rc = ensure_dev_p(pl, p, n_steps, s);
  if (rc) return rc;
  return launch_land_fix(pl, cv, in, out, pl->dev_p, n_steps, c, fb32 ? 1 : 0, nbatch, s);
}
// Stages the raw grid planes on the device (temporaries, unless they are there already), folds them into the plan (precompute), frees
// the temporaries; scalar plans also get a row of zeros for k_ring.
// plane_levels (stacked plans, gcmf_plan_create_levels): plane k is plane_levels[k] planes long
static int stage_grid(gcmf_plan *pl, const void *const *planes, int nplanes, const int64_t *plane_levels = nullptr) {
  const gcmf_plan_desc &d = pl->d;
  const size_t one_plane = (size_t)d.ny * d.nx * dtype_size(d.dtype);
  std::vector<const void *> dplanes(nplanes, nullptr);
  std::vector<void *> staged;
  int rc = GCMF_OK;
  for (int k = 0; k < nplanes && rc == GCMF_OK; ++k) {
    if (d.planes_on_device) {
      dplanes[k] = planes[k];
      continue;
    }
    const size_t plane_bytes = one_plane * (size_t)(plane_levels ? plane_levels[k] : 1);
    int dup = -1;  // the same host array passed twice (e.g. wet_mask_t is wet_mask_q) is uploaded once
    for (int q = 0; q < k; ++q)
      if (planes[q] == planes[k] && (!plane_levels || plane_levels[q] == plane_levels[k])) dup = q;
    if (dup >= 0) {
      dplanes[k] = dplanes[dup];
      continue;
    }
    void *p = nullptr;
    hipError_t e3 = hipMalloc(&p, plane_bytes);
    if (e3 == hipSuccess) {
      staged.push_back(p);
      e3 = hipMemcpyAsync(p, planes[k], plane_bytes, hipMemcpyHostToDevice, pl->stream);
    }
    if (e3 != hipSuccess) {
      set_error("staging grid plane %d failed: %s", k, hipGetErrorString(e3));
      rc = GCMF_ERR_HIP;
    }
    dplanes[k] = p;
  }
  if (rc == GCMF_OK)
    rc = pl->stacked ? precompute_levels(pl, dplanes.data(), plane_levels) : precompute(pl, dplanes.data(), d.planes_on_device ? nullptr : planes);
  if (rc == GCMF_OK && pl->ncomp == 1) {  // a row of zeros for k_ring
    void *z = nullptr;
    const size_t zb = ((size_t)d.nx + 64) * 8 + 256;
    if (hipMalloc(&z, zb) == hipSuccess && hipMemsetAsync(z, 0, zb, pl->stream) == hipSuccess) {
      pl->owned.push_back(z);
      pl->zero_row = z;
      pl->ring_nfb = reinterpret_cast<unsigned *>((char *)z + zb - 8);  // beyond anything a (padded) row read touches
    } else if (z) {
      (void)hipFree(z);
    }
  }
  (void)hipStreamSynchronize(pl->stream);
  for (void *p : staged) (void)hipFree(p);
  return rc;
}

}  // namespace gcmf

using namespace gcmf;

extern "C" {

const char *gcmf_last_error(void) { return g_err.c_str(); }
int gcmf_version(void) { return GCMF_VERSION; }

int gcmf_grid_nplanes(int gt) {
  GridInfo gi;
  return grid_info(gt, gi) ? gi.nplanes : -1;
}
int gcmf_grid_ncomp(int gt) {
  GridInfo gi;
  return grid_info(gt, gi) ? gi.ncomp : -1;
}
int gcmf_grid_is_dimensional(int gt) {
  GridInfo gi;
  return grid_info(gt, gi) ? gi.dimensional : -1;
}
int gcmf_grid_is_tripolar(int gt) {
  GridInfo gi;
  return grid_info(gt, gi) ? gi.tripolar : -1;
}

void gcmf_plan_destroy(gcmf_plan *pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->d.device);
  if (pl->stream) (void)hipStreamSynchronize(pl->stream);
  for (void *p : pl->owned) (void)hipFree(p);
  for (hipEvent_t e : pl->dom_ev) (void)hipEventDestroy(e);
  if (pl->work) (void)hipFree(pl->work);
  if (pl->side) { (void)hipStreamSynchronize(pl->side); (void)hipStreamDestroy(pl->side); }
  if (pl->ev_fork) (void)hipEventDestroy(pl->ev_fork);
  if (pl->ev_join) (void)hipEventDestroy(pl->ev_join);
  if (pl->ev0) (void)hipEventDestroy(pl->ev0);
  if (pl->ev1) (void)hipEventDestroy(pl->ev1);
  if (pl->ev_busy) (void)hipEventDestroy(pl->ev_busy);
  if (pl->s_in) { (void)hipStreamSynchronize(pl->s_in); (void)hipStreamDestroy(pl->s_in); }
  if (pl->s_out) { (void)hipStreamSynchronize(pl->s_out); (void)hipStreamDestroy(pl->s_out); }
  for (int q = 0; q < 2; ++q) {
    if (pl->ev_in[q]) (void)hipEventDestroy(pl->ev_in[q]);
    if (pl->ev_cmp[q]) (void)hipEventDestroy(pl->ev_cmp[q]);
    if (pl->ev_out[q]) (void)hipEventDestroy(pl->ev_out[q]);
  }
  if (pl->stage) (void)hipFree(pl->stage);
  if (pl->dev_p) (void)hipFree(pl->dev_p);
  if (pl->bank_rev) (void)hipFree(pl->bank_rev);
  if (pl->bank_fwd) (void)hipFree(pl->bank_fwd);
  if (pl->coarsen_w) (void)hipFree(pl->coarsen_w);
  if (pl->coarsen_buf) (void)hipFree(pl->coarsen_buf);
  if (pl->cov_buf) (void)hipFree(pl->cov_buf);
  resident_free(pl);
  if (pl->stream) (void)hipStreamDestroy(pl->stream);
  delete pl;
}

// gcmf_plan_create (plane_levels == nullptr) and gcmf_plan_create_levels
static int plan_create(const gcmf_plan_desc *desc, const void *const *planes, const int64_t *plane_levels, int nplanes, int64_t nlev,
                       gcmf_plan **out) {
  if (!desc || !out) {
    set_error("gcmf_plan_create: null argument");
    return GCMF_ERR_INVALID_ARG;
  }
  *out = nullptr;
  GridInfo gi;
  if (!grid_info(desc->grid_type, gi)) {
    set_error("gcmf_plan_create: unknown grid_type %d", desc->grid_type);
    return GCMF_ERR_INVALID_ARG;
  }
  if (nplanes != gi.nplanes || (nplanes > 0 && !planes)) {
    set_error("gcmf_plan_create: grid type %d needs %d grid planes, got %d", desc->grid_type, gi.nplanes, nplanes);
    return GCMF_ERR_INVALID_ARG;
  }
  if (desc->dtype != GCMF_F32 && desc->dtype != GCMF_F64) {
    set_error("gcmf_plan_create: bad dtype %d", desc->dtype);
    return GCMF_ERR_INVALID_ARG;
  }
  if (desc->ny < 1 || desc->nx < 1 || desc->ny > (1 << 30) || desc->nx > (1 << 30) ||
      desc->ny * desc->nx > (int64_t)2000000000) {
    set_error("gcmf_plan_create: bad grid shape (%lld, %lld)", (long long)desc->ny, (long long)desc->nx);
    return GCMF_ERR_INVALID_ARG;
  }
  if (desc->row_begin < 0 || desc->row_end > desc->ny || desc->row_begin >= desc->row_end || desc->halo < 0) {
    set_error("gcmf_plan_create: bad row slab [%lld, %lld) of %lld rows", (long long)desc->row_begin,
              (long long)desc->row_end, (long long)desc->ny);
    return GCMF_ERR_INVALID_ARG;
  }
  for (int k = 0; k < nplanes; ++k)
    if (!planes[k]) {
      set_error("gcmf_plan_create: grid plane %d is NULL", k);
      return GCMF_ERR_INVALID_ARG;
    }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    set_error("no HIP device available (%s)", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return GCMF_ERR_NO_DEVICE;
  }
  GCMF_HIP(hipSetDevice(desc->device));

  gcmf_plan *pl = new gcmf_plan();
  pl->d = *desc;
  pl->stacked = plane_levels != nullptr;
  pl->nlev = nlev;
  pl->kind = gi.kind;
  pl->ncomp = gi.ncomp;
  pl->tripolar = gi.tripolar;
  pl->area_weighted = gi.area_weighted;
  pl->dimensional = gi.dimensional;
  const bool ring_of_one = (desc->flags & GCMF_PLAN_SELF_RING) != 0;
  if (ring_of_one && (gi.tripolar || desc->row_begin != 0 || desc->row_end != desc->ny)) {
    delete pl;
    set_error("gcmf_plan_create: GCMF_PLAN_SELF_RING needs a non-tripolar plan covering the whole grid");
    return GCMF_ERR_INVALID_ARG;
  }
  pl->full = (desc->row_begin == 0 && desc->row_end == desc->ny) && !ring_of_one;
  int64_t gs = 0, gn = 0;
  if (!pl->full) {
    if (desc->halo < 1) {
      delete pl;
      set_error("gcmf_plan_create: a partial row slab needs halo >= 1");
      return GCMF_ERR_INVALID_ARG;
    }
    gs = (pl->tripolar && desc->row_begin == 0) ? 0 : desc->halo;
    gn = (pl->tripolar && desc->row_end == desc->ny) ? 0 : desc->halo;
  }
  pl->rows_owned = desc->row_end - desc->row_begin;
  pl->rows_alloc = gs + pl->rows_owned + gn;
  pl->first_owned = gs;
  Geom &g = pl->g;
  g.nx = (int)desc->nx;
  g.rows = (int)pl->rows_alloc;
  g.south_wrap = pl->full && !pl->tripolar;
  g.north_wrap = pl->full && !pl->tripolar;
  g.fold = pl->tripolar && desc->row_end == desc->ny;
  g.area_weighted = pl->area_weighted;

  auto fail = [&](int rc) {
    gcmf_plan_destroy(pl);
    return rc;
  };
#define PLAN_HIP(call)                                                                 \
  do {                                                                                 \
    hipError_t e2_ = (call);                                                           \
    if (e2_ != hipSuccess) {                                                           \
      set_error("%s failed: %s", #call, hipGetErrorString(e2_));                       \
      return fail(GCMF_ERR_HIP);                                                       \
    }                                                                                  \
  } while (0)
  if (const char *e = getenv("GCMF_CGRID_TILE")) pl->cgrid_tile = atoi(e);
  if (const char *e = getenv("GCMF_CGRID_RING")) pl->cgrid_ring = atoi(e);
  if (const char *e = getenv("GCMF_CGRID_RING_SMAX")) pl->cgrid_ring_smax = atoi(e);
  if (const char *e = getenv("GCMF_HOST_CHUNK_MB")) pl->host_chunk_bytes = (size_t)(atof(e) * 1048576.0);
  if (const char *e = getenv("GCMF_HOST_REGISTER")) pl->host_register = atoi(e);
  if (const char *e = getenv("GCMF_ZERO_LAND")) pl->zero_land = atoi(e);
  if (const char *e = getenv("GCMF_RING")) pl->ring = atoi(e);
  if (const char *e = getenv("GCMF_ZIGZAG")) pl->zigzag = atoi(e);
  if (const char *e = getenv("GCMF_RINGC_XE_ROWS")) pl->ringc_xe_rows = atoi(e);
  if (const char *e = getenv("GCMF_CLENSHAW")) pl->clenshaw = atoi(e);
  if (const char *e = getenv("GCMF_RINGC9")) pl->ringc9 = atoi(e);
  if (const char *e = getenv("GCMF_RINGC_ZIP")) pl->ringc_zip = atoi(e);
  if (const char *e = getenv("GCMF_BAND_SEQ_CELLS")) pl->band_seq_cells = atoll(e);
  if (const char *e = getenv("GCMF_ZIP_FOLD")) pl->zip_fold = atoi(e);
  if (const char *e = getenv("GCMF_PACK_BATCH")) pl->pack_batch = atoi(e);
  if (const char *e = getenv("GCMF_SINGLE_LAUNCH")) pl->single_launch = atoi(e);
  if (const char *e = getenv("GCMF_CLENSHAW_F32")) pl->clenshaw_f32 = atoi(e);
  PLAN_HIP(hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking));
  PLAN_HIP(hipEventCreate(&pl->ev0));
  PLAN_HIP(hipEventCreate(&pl->ev1));
  PLAN_HIP(hipEventCreateWithFlags(&pl->ev_busy, hipEventDisableTiming));

  if (int rc = stage_grid(pl, planes, nplanes, plane_levels)) return fail(rc);
  *out = pl;
  return GCMF_OK;
#undef PLAN_HIP
}

int gcmf_plan_create(const gcmf_plan_desc *desc, const void *const *planes, int nplanes, gcmf_plan **out) {
  return plan_create(desc, planes, nullptr, nplanes, 1, out);
}

int gcmf_plan_create_levels(const gcmf_plan_desc *desc, const void *const *planes, const int64_t *plane_levels, int nplanes, int64_t nlev,
                            gcmf_plan **out) {
  if (!desc || !out || !plane_levels || nplanes < 1) {
    set_error("gcmf_plan_create_levels: null argument");
    return GCMF_ERR_INVALID_ARG;
  }
  *out = nullptr;
  GridInfo gi;
  if (!grid_info(desc->grid_type, gi)) {
    set_error("gcmf_plan_create_levels: unknown grid_type %d", desc->grid_type);
    return GCMF_ERR_INVALID_ARG;
  }
  if (gi.kind != K_FLUX || gi.tripolar) {
    set_error("gcmf_plan_create_levels: stacked plans exist for IRREGULAR_WITH_LAND, MOM5U and MOM5T (flux form, no tripole seam), not "
              "for grid type %d: build one plan per level", desc->grid_type);
    return GCMF_ERR_UNSUPPORTED;
  }
  if (desc->dtype != GCMF_F64) {
    set_error("gcmf_plan_create_levels: stacked plans compute in f64 (dtype %d given): build one plan per level", desc->dtype);
    return GCMF_ERR_UNSUPPORTED;
  }
  if (desc->row_begin != 0 || desc->row_end != desc->ny || (desc->flags & GCMF_PLAN_SELF_RING)) {
    set_error("gcmf_plan_create_levels: stacked plans cover the whole grid (rows [%lld, %lld) of %lld%s given)", (long long)desc->row_begin,
              (long long)desc->row_end, (long long)desc->ny, (desc->flags & GCMF_PLAN_SELF_RING) ? ", GCMF_PLAN_SELF_RING" : "");
    return GCMF_ERR_UNSUPPORTED;
  }
  if (nlev < 1 || nlev > 32768) {
    set_error("gcmf_plan_create_levels: %lld levels (1 .. 32768)", (long long)nlev);
    return GCMF_ERR_INVALID_ARG;
  }
  for (int k = 0; k < nplanes; ++k)
    if (plane_levels[k] != 1 && plane_levels[k] != nlev) {
      set_error("gcmf_plan_create_levels: grid plane %d has %lld levels, neither 1 nor %lld", k, (long long)plane_levels[k], (long long)nlev);
      return GCMF_ERR_INVALID_ARG;
    }
  return plan_create(desc, planes, plane_levels, nplanes, nlev, out);
}

int64_t gcmf_plan_levels(const gcmf_plan *pl) { return pl ? pl->nlev : 0; }

int gcmf_plan_rows(const gcmf_plan *pl, int64_t *rows_alloc, int64_t *first_owned, int64_t *rows_owned) {
  if (!pl) return GCMF_ERR_INVALID_ARG;
  if (rows_alloc) *rows_alloc = pl->rows_alloc;
  if (first_owned) *first_owned = pl->first_owned;
  if (rows_owned) *rows_owned = pl->rows_owned;
  return GCMF_OK;
}

static const int64_t MAX_LAUNCH_BATCH = 32768;  // batch entries per launch (gridDim.y of the scalar kernels)

// What the evaluation schedules of one gcmf_apply / gcmf_laplacian call share: the stream, the caller's fields (on the device), the work
// planes of every component (F2: the second fbar plane of the scalar blocked schedule), the polynomial and the launch count; cv: the
// grid and the entry layout as this call sees them (gcmf_internal.hpp).
struct ApplyCtx {
  gcmf_plan *pl;
  CallView cv;
  hipStream_t s;
  const void *din[2];
  void *dout[2], *A[2], *B[2], *Cb[2], *Db[2], *F[2], *F2, *Pp[2];
  const double *p;
  int n_steps, rows, launches;
  double c;
  int64_t nbatch;
  bool fb32;
};

// gcmf_apply_bank_gaps folds once per FIELD: what its launches have folded already, and where in the work buffer
struct GapFold {
  const void *in = nullptr, *at = nullptr;
  int64_t n = 0;
};

// gcmf_apply_adjoint (gcmf.h): out = F^T in = D F(in / D), F = what gcmf_apply applies.  A launch that is handed one of these scales its
// input into a plane of the work buffer first (the forms of k_prepare in gcmf_scalar.hip), runs gcmf_apply's own schedule on that
// plane, and scales the result in place.  like: the forward call's input planes (has_like), whose NaNs are the cells without a
// derivative -- and, under the two NaN flags, the gaps the launch derives its masks / faces from, as the forward call did.
struct Adjoint {
  const void *like[2] = {nullptr, nullptr};
  bool has_like = false;
};

static const char *const FACES_WHERE = "GCMF_FACES_FROM_NAN is a gcmf_apply flag for whole-grid f64 ordinary plans of IRREGULAR_WITH_LAND, MOM5U and MOM5T";

static int lapl_step(ApplyCtx &x) {
  StepArgs a{};
  for (int k = 0; k < x.pl->ncomp; ++k) { a.t1[k] = x.din[k]; a.t0[k] = x.dout[k]; a.fb_out[k] = nullptr; }
  a.mode = STEP_LAPL; a.nbatch = x.nbatch; a.row_lo = 0; a.row_hi = x.rows;
  const int rc = step_dispatch(x.pl, x.cv, a, x.s);
  if (!rc) ++x.launches;
  return rc;
}

// Small fields: the whole polynomial on the chip in ONE launch (64 levels at a time; gcmf_resident.hip) -- the field, both states
// and the coefficients live in registers / LDS, nothing but the result goes back to memory.  Same bits as the strip-marching launches.
static int sched_resident(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  pl->res_lo = pl->res_hi = 0;   // (launch_resident notes the serial numbers of this application's launches)
  void *pool[4] = {x.A[0], x.B[0], x.Cb[0], x.Db[0]};
  const void *u = nullptr, *v = nullptr;
  double pk[64];
  int rc;
  for (int lvl = 1; lvl <= x.n_steps;) {
    const int L = std::min(64, x.n_steps - lvl + 1);
    void *fr[2];
    free_planes(pool, 1, u, v, fr);
    MultiArgs m = backward_args(x.p, x.n_steps, x.c, lvl, L, u, v, fr, x.din[0], x.dout[0], pk);
    m.fb_is_f32 = x.fb32; m.nbatch = 1; m.row_lo = 0; m.row_hi = x.rows;
    if ((rc = dom_begin(pl, x.s))) return rc;
    if ((rc = launch_resident(pl, m, pk, L, x.s))) return rc;
    if ((rc = dom_end(pl, x.s))) return rc;
    ++x.launches;
    u = fr[0]; v = fr[1];
    lvl += L;
  }
  return GCMF_OK;
}

// OPT-IN ("single_launch"): the whole polynomial in ONE persistent launch (gcmf_ringc_one.hip).  false: it did not run (the process
// may not run persistent kernels now), the caller runs the back-to-back launches of sched_backward_scalar instead (same bits).
static bool sched_single_launch(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  void *pool[4] = {x.A[0], x.B[0], x.Cb[0], x.Db[0]};
  if (dom_begin(pl, x.s)) return false;
  const int r1 = launch_ringc_one(pl, ringc_one_depth(pl, x.n_steps, x.nbatch), x.p, x.n_steps, x.c, x.din[0], x.dout[0], pool, x.s);
  if (dom_end(pl, x.s)) return false;
  if (r1 == GCMF_OK) ++x.launches;
  return r1 == GCMF_OK;
}

// Backward (Clenshaw) evaluation, gcmf_ringc_impl.hpp: state (b_{k+1}, b_{k+2}) in a pool of four planes, the constant input read by
// every launch, no fbar planes.  The first launch forms b_n = p[n] f as it loads f; level l = 1..n uses p[n - l]; the last launch
// writes the result.  depths: clenshaw_cut's launches.
// was_clean: the pool's planes are finite wherever k_ringcz's wet-row tables leave them unwritten (gcmf_plan::pool_clean); launches of
// a whole grid and a lone field may take such a table (wet_table, gcmf_ringc_zip.hip) and keep the planes that way -- the flux kinds'
// backward kernels take f as zero on isolated cells, whose state is then +-0 at every level -- every other caller owns its planes.
static int sched_backward_scalar(ApplyCtx &x, const int *depths, int n_clen, bool was_clean) {
  void *pool[4] = {x.A[0], x.B[0], x.Cb[0], x.Db[0]};
  const void *u = nullptr, *v = nullptr;
  int rc;
  gcmf_plan *pl = x.pl;
  CallView &cv = x.cv;
  cv.wet_now = pl->wet_rows > 0 && x.nbatch == 1 && !cv.mask_per_field && !cv.stacked && !cv.bank_n && pl->full && !pl->g.fold && pl->kind == K_FLUX &&
               pl->d.dtype == GCMF_F64 && cv.n_land > 0 && pl->pool_bytes > 0;
  pl->pool_clean = cv.wet_now && was_clean;
  for (int q = 0, lvl = 1; q < n_clen; lvl += depths[q++]) {
    void *fr[2];
    free_planes(pool, 1, u, v, fr);
    MultiArgs m = backward_args(x.p, x.n_steps, x.c, lvl, depths[q], u, v, fr, x.din[0], x.dout[0]);
    m.fb_is_f32 = x.fb32; m.nbatch = x.nbatch; m.row_lo = 0; m.row_hi = x.rows;
    if ((rc = advance_multi(pl, cv, m, x.s, &x.launches, true))) return rc;   // (+ the tripole band on tripolar plans)
    u = fr[0]; v = fr[1];
  }
  return GCMF_OK;
}

// Temporally blocked schedule (scalar kinds): each launch advances S steps and reads/writes every plane once.  prepare/finalize are
// fused into the first / last launch.  State buffers rotate through a pool of four because a launch may not overwrite the planes its
// neighbours' halos are still reading.
static int sched_forward_scalar(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  const double *p = x.p;
  const int n_steps = x.n_steps;
  // flux kinds only: the land-mask kernels have a NaN-only mode that already makes NaN on land free, there the two extra passes
  // would only cost
  const bool zero_land = land_ok(pl, x.cv, n_steps);  // n_steps < 4096: k_land_fix keeps p in LDS
  void *pool[4] = {x.A[0], x.B[0], x.Cb[0], x.Db[0]};
  void *Fcur = x.F[0], *Fnext = x.F2;   // fbar ping-pongs between two planes (see oF2)
  const void *u = x.din[0], *v = nullptr;
  bool land_zeroed = false;  // the first blocked launch kept the isolated cells out of the state
  int rc;
  for (int k = 1; k <= n_steps;) {
    const int S = deepest_depth(n_steps - k + 1, std::min(8, pl->multi_s), [&](int d) { return multi_supported(pl, d); });
    void *fr[2];
    free_planes(pool, 1, u, v, fr);
    const bool is_last = (k + S - 1 == n_steps);
    if (S >= 2) {
      MultiArgs m{};
      m.u0 = u; m.v0 = v; m.uo = fr[0]; m.vo = fr[1];
      m.fb_in = Fcur; m.fb_out = is_last ? x.dout[0] : Fnext;
      std::swap(Fcur, Fnext);
      m.first = (k == 1); m.last = is_last; m.S = S; m.fb_is_f32 = x.fb32;
      m.land_zero = land_zeroed ? 1 : 0;
      // the first launch may drop land on load if k_land_fix restores it at the end (not for a one-launch filter)
      m.ring_first = (k == 1 && !is_last && (zero_land || x.cv.n_land == 0)) ? 1 : 0;
      for (int t = 0; t < S; ++t) m.pk[t] = p[k + t];
      m.p0 = p[0]; m.c = x.c; m.nbatch = x.nbatch; m.row_lo = 0; m.row_hi = x.rows;
      if ((rc = advance_multi(pl, x.cv, m, x.s, &x.launches))) return rc;
      u = fr[0]; v = fr[1];
      if (k == 1 && zero_land && !is_last) {  // keep the isolated cells out of the state from here on
        if (!ring_supported(pl, x.cv, m)) {
          if ((rc = launch_zero_land(pl, x.cv, fr[0], fr[1], x.nbatch, x.s))) return rc;
        }   // (k_ring's first launch and k_fold_band took the land as zero while they loaded the field)
        land_zeroed = true;
      }
    } else {
      StepArgs a1{};
      a1.mode = (k == 1 ? GCMF_STEP_FIRST : 0u) | (is_last ? GCMF_STEP_LAST : 0u);
      a1.coef0 = (k == 1) ? p[0] : p[k]; a1.coef1 = p[1]; a1.c = x.c; a1.fb_is_f32 = x.fb32; a1.nbatch = x.nbatch;
      a1.row_lo = 0; a1.row_hi = x.rows;
      const void *src = u;
      if (k == 1 && pl->area_weighted) {  // the single-step kernel wants T_0 = field*area materialised
        if ((rc = launch_prepare(pl, x.din, x.Pp, x.nbatch, 0, x.rows, x.s))) return rc;
        ++x.launches;
        src = x.Pp[0];
      }
      a1.t1[0] = src; a1.t2[0] = v; a1.t0[0] = fr[0]; a1.fb_in[0] = Fcur; a1.fb_out[0] = is_last ? x.dout[0] : Fcur;
      if ((rc = step_dispatch(pl, x.cv, a1, x.s))) return rc;
      ++x.launches;
      v = src; u = fr[0];
    }
    k += S;
  }
  if (land_zeroed)  // the isolated cells' own polynomial, from the caller's untouched input
    return land_fix_tail(pl, x.cv, p, n_steps, x.c, x.din[0], x.dout[0], x.fb32, x.nbatch, x.s);
  return GCMF_OK;
}

// C-grid (B-grid with GCMF_CLENSHAW=2: it is bit-exact with numpy forward, so backward is an option there like for the land-mask kinds):
// the polynomial evaluated backwards (k_cgrid_stream2c / k_bgrid_stream2c): state (b_{k+1}, b_{k+2}) in a pool of four plane pairs, the
// constant input (u, v) read by every launch, no fbar planes.  Level l = 1..n uses p[n - l]; the first launch forms b_n = p[n] f as it
// loads f, the last one writes the result.  Four levels per launch keep two operand rows in flight, five spill (DESIGN_HISTORY.md,
// round 6); deeper launches exist only in k_cgrid_ring (gcmf_cgrid_ring.hip), whose 16-byte accesses need the caller's planes aligned.
static int sched_backward_vec(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  void *pool[8] = {x.A[0], x.A[1], x.B[0], x.B[1], x.Cb[0], x.Cb[1], x.Db[0], x.Db[1]};
  const void *u[2] = {x.din[0], x.din[1]}, *v[2] = {nullptr, nullptr};
  const bool al16 = ptr_al16(x.din[0]) && ptr_al16(x.din[1]) && ptr_al16(x.dout[0]) && ptr_al16(x.dout[1]);
  const int ring_smax = cgrid_ring_smax(pl, x.nbatch);
  const int smax = std::min(pl->multi_s, std::max(4, al16 ? ring_smax : std::min(5, ring_smax)));
  int rc;
  for (int lvl = 1; lvl <= x.n_steps;) {
    const int S = vec_backward_next_depth(pl, x.nbatch, x.n_steps - lvl + 1, smax);
    void *fr[4];
    free_planes(pool, 2, u[0], v[0], fr);
    VecMultiArgs m = backward_args_vec(x.p, x.n_steps, x.c, lvl, S, u, v, fr, x.din, x.dout);
    m.fb_is_f32 = x.fb32; m.nbatch = x.nbatch; m.row_lo = 0; m.row_hi = x.rows;
    if ((rc = dom_begin(pl, x.s))) return rc;
    if ((rc = launch_vec_multi(pl, m, x.s))) return rc;
    if ((rc = dom_end(pl, x.s))) return rc;
    for (int q = 0; q < 2; ++q) { u[q] = fr[2 + q]; v[q] = fr[q]; }
    lvl += S;
    ++x.launches;
  }
  return GCMF_OK;
}

// vector kinds: S = 2..6 steps per pass, (T_{k-1}, T_{k-2}) -> (T_{k+S-2}, T_{k+S-1}).  Neither output may overwrite T_{k-2}: the halo
// rows / columns a strip recomputes need its neighbours' T_{k-2}.  The state rotates through four buffers.  A lone last step runs the
// single-step kernel.
static int sched_forward_vec(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  const double *p = x.p;
  const int n_steps = x.n_steps;
  void *pool[8] = {x.A[0], x.A[1], x.B[0], x.B[1], x.Cb[0], x.Cb[1], x.Db[0], x.Db[1]};
  const void *u[2] = {x.din[0], x.din[1]}, *v[2] = {nullptr, nullptr};
  int rc;
  for (int k = 1; k <= n_steps;) {
    const int left = n_steps - k + 1;
    void *fr[4];
    free_planes(pool, 2, u[0], v[0], fr);
    int S = deepest_depth(left, std::min(6, pl->multi_s), [&](int d) { return vec_multi_supported(pl, x.nbatch, d); });
    if (S == 1 && left >= 2) S = 2;
    if (S >= 2) {
      const bool is_last = (k + S - 1 == n_steps);
      VecMultiArgs m{};
      for (int q = 0; q < 2; ++q) {
        m.u0[q] = u[q]; m.uprev[q] = v[q]; m.u1o[q] = fr[q]; m.u2o[q] = fr[2 + q];
        m.fb_in[q] = x.F[q]; m.fb_out[q] = is_last ? x.dout[q] : x.F[q];
      }
      for (int t = 0; t < S; ++t) m.pk[t] = p[k + t];
      m.p0 = p[0]; m.c = x.c; m.S = S;
      m.first = (k == 1); m.last = is_last; m.fb_is_f32 = x.fb32; m.nbatch = x.nbatch; m.row_lo = 0; m.row_hi = x.rows;
      if ((rc = dom_begin(pl, x.s))) return rc;
      if ((rc = launch_vec_multi(pl, m, x.s))) return rc;
      if ((rc = dom_end(pl, x.s))) return rc;
      for (int q = 0; q < 2; ++q) { u[q] = fr[2 + q]; v[q] = fr[q]; }
      k += S;
    } else {
      StepArgs a1{};
      a1.mode = (k == 1 ? GCMF_STEP_FIRST : 0u) | GCMF_STEP_LAST;
      a1.coef0 = (k == 1) ? p[0] : p[k]; a1.coef1 = p[1]; a1.c = x.c; a1.fb_is_f32 = x.fb32; a1.nbatch = x.nbatch;
      a1.row_lo = 0; a1.row_hi = x.rows;
      for (int q = 0; q < 2; ++q) {
        a1.t1[q] = u[q]; a1.t2[q] = v[q]; a1.t0[q] = fr[q]; a1.fb_in[q] = x.F[q]; a1.fb_out[q] = x.dout[q];
      }
      if ((rc = step_dispatch(pl, x.cv, a1, x.s))) return rc;
      k += 1;
    }
    ++x.launches;
  }
  return GCMF_OK;
}

// One launch per step.  Step k reads T_{k-1} (stencil) and T_{k-2} (centre) and overwrites T_{k-2}'s buffer with T_k:
//   k=1: X0 -> A      k=2: (A, X0) -> B      k=3: (B, A) -> A      k=4: (A, B) -> B ...
static int sched_single_steps(ApplyCtx &x) {
  gcmf_plan *pl = x.pl;
  const double *p = x.p;
  const int n_steps = x.n_steps, nc = pl->ncomp;
  const void *x0[2] = {x.din[0], x.din[1]};
  int rc;
  if (pl->area_weighted) {  // T_0 = field * area
    if ((rc = launch_prepare(pl, x.din, x.Pp, x.nbatch, 0, x.rows, x.s))) return rc;
    ++x.launches;
    for (int k = 0; k < nc; ++k) x0[k] = x.Pp[k];
  }
  for (int k = 1; k <= n_steps; ++k) {
    StepArgs a{};
    a.mode = (k == 1 ? GCMF_STEP_FIRST : 0u) | (k == n_steps ? GCMF_STEP_LAST : 0u);
    a.coef0 = (k == 1) ? p[0] : p[k]; a.coef1 = p[1]; a.c = x.c; a.fb_is_f32 = x.fb32; a.nbatch = x.nbatch;
    a.row_lo = 0; a.row_hi = x.rows;
    for (int q = 0; q < nc; ++q) {
      if (k == 1) { a.t1[q] = x0[q]; a.t2[q] = nullptr; a.t0[q] = x.A[q]; }
      else if (k == 2) { a.t1[q] = x.A[q]; a.t2[q] = x0[q]; a.t0[q] = x.B[q]; }
      else if (k % 2) { a.t1[q] = x.B[q]; a.t2[q] = x.A[q]; a.t0[q] = x.A[q]; }
      else { a.t1[q] = x.A[q]; a.t2[q] = x.B[q]; a.t0[q] = x.B[q]; }
      a.fb_in[q] = x.F[q];
      a.fb_out[q] = (k == n_steps) ? x.dout[q] : x.F[q];
    }
    if ((rc = step_dispatch(pl, x.cv, a, x.s))) return rc;
    ++x.launches;
  }
  return GCMF_OK;
}

// The filter's schedule: the first of these that applies runs.  use_multi / use_vmulti: the scalar / vector blocked launches are on
// offer (the work layout has their planes).
static int run_schedule(ApplyCtx &x, uint32_t flags, bool use_multi, bool use_vmulti) {
  gcmf_plan *pl = x.pl;
  const CallView &cv = x.cv;
  int depths[1024];
  const bool fwd_only = flags & GCMF_FORWARD_RECURRENCE;   // the caller wants the reference's forward recurrence / accumulation
  const bool back_f32 = pl->clenshaw_f32 || (flags & GCMF_BACKWARD_F32);   // f32 B-grid / scalar state backwards: only when asked for
  const int n_clen = (use_multi && !fwd_only) ? clenshaw_cut(pl, cv, x.n_steps, depths, 1024, back_f32, x.nbatch) : 0;
  if (pl->res_lo) {   // the LAST call of this plan ran on the chip: did one of ITS launches time out?  (told once, to the plan whose
    //                   output was poisoned -- never to an unrelated plan; the process runs the strip-marching launches from now on)
    const unsigned lo = pl->res_lo, hi = pl->res_hi;
    pl->res_lo = pl->res_hi = 0;
    if (resident_take_failure(pl->d.device, lo, hi)) {
      set_error("the previous on-chip / single-launch application of this plan (k_resident, k_ringc_one) timed out waiting for another "
                "workgroup and its result is NaN (another process running persistent kernels on this GPU outside the lock file's reach?); "
                "the back-to-back strip-marching launches are used from now on");
      return GCMF_ERR_HIP;
    }
  }
  const bool was_clean = pl->pool_clean;   // (only sched_backward_scalar keeps the work planes finite on land)
  pl->pool_clean = false;
  bool resident = false;
  int path = GCMF_PATH_STRIPS;
  if (cv.stacked && n_clen <= 0) {   // (run_whole has refused GCMF_FORWARD_RECURRENCE)
    set_error("gcmf_apply: a stacked plan (gcmf_plan_create_levels) runs the backward evaluation only, which is not on offer for this plan "
              "and a polynomial of %d steps (gcmf_clenshaw_cut_batch returns 0): build one plan per level", x.n_steps);
    return GCMF_ERR_UNSUPPORTED;
  }
  // (the on-chip kernel reads the plan's own mask, and one level's planes)
  const bool own = !cv.mask_per_field && !cv.stacked && !cv.bank_n;
  if (n_clen > 0 && x.nbatch == 1 && !(flags & GCMF_NO_RESIDENT) && own) {
    int why = GCMF_RESIDENT_OFF;
    resident = resident_supported(pl, 0, x.rows, std::min(x.n_steps, 64), x.n_steps, &why);   // (small whole grids; GCMF_RESIDENT=1: whatever fits)
    if (!resident && why == GCMF_RESIDENT_LOCK_BUSY) path = GCMF_PATH_STRIPS_LOCK_BUSY;
    if (!resident && why == GCMF_RESIDENT_DISABLED) path = GCMF_PATH_STRIPS_DISABLED;
  }
  if (resident) path = GCMF_PATH_RESIDENT;
  pl->last_path = path;
  ++pl->path_count[path];
  if (n_clen > 0) {
    int rc = GCMF_OK;
    if (resident)
      rc = sched_resident(x);
    else if ((flags & GCMF_NO_RESIDENT) || !own || ringc_one_depth(pl, x.n_steps, x.nbatch) <= 0 || !sched_single_launch(x))
      rc = sched_backward_scalar(x, depths, n_clen, was_clean);
    if (rc || cv.n_land == 0) return rc;
    // the isolated cells' own polynomial (forward recurrence, as the reference computes it)
    // (every entry its own; gcmf_apply_bank_gaps: on the land bytes of its own field too -- the launcher looks at cv.stacked)
    if (cv.bank_n > 0) return launch_land_fix_bank(pl, cv, x.din[0], x.dout[0], x.n_steps, x.c, x.nbatch, x.s);
    return land_fix_tail(pl, cv, x.p, x.n_steps, x.c, x.din[0], x.dout[0], x.fb32, x.nbatch, x.s);
  }
  if (use_multi) return sched_forward_scalar(x);
  const bool vec_backward = (pl->kind == K_CGRID && pl->clenshaw >= 1) ||
                            (pl->kind == K_BGRID && pl->clenshaw >= 2 && (pl->d.dtype == GCMF_F64 || back_f32));
  if (use_vmulti && vec_backward && !fwd_only) return sched_backward_vec(x);
  if (use_vmulti) return sched_forward_vec(x);
  return sched_single_steps(x);
}

// The plan's work buffers are shared by all calls: a call enqueued on another stream (dask worker threads with their own streams) must
// not start before the previous one has finished with them.  The wait is needed only when this call is on ANOTHER stream than the last
// one: a stream orders its own work.  The event is recorded lazily, here, on the previous call's stream -- behind everything that stream
// was given since, which is later than necessary but correct -- so back-to-back calls on one stream pay for no event at all (two queue
// packets less per application).
static int wait_for_work(gcmf_plan *pl, hipStream_t s) {
  if (pl->busy_valid && pl->busy_stream != s) {
    if (pl->busy_recorded || hipEventRecord(pl->ev_busy, pl->busy_stream) == hipSuccess) {
      GCMF_HIP(hipStreamWaitEvent(s, pl->ev_busy, 0));
    } else {   // the caller destroyed that stream meanwhile: whatever ran on it is waited for the blunt way
      (void)hipGetLastError();
      GCMF_HIP(hipDeviceSynchronize());
    }
  }
  return GCMF_OK;
}

// After the launches: the work buffers are marked busy, the result goes back to the host (host pointers: `out`, `out_bytes` per
// component), a timed-out on-chip launch of this call is reported, and the timing events are read.
static int finish_call(ApplyCtx &x, bool on_dev, void *const *out, size_t out_bytes, bool timing, bool timed) {
  gcmf_plan *pl = x.pl;
  const hipStream_t s = x.s;
  int rc;
  if (timing) GCMF_HIP(hipEventRecord(pl->ev1, s));
  // "work buffers busy": recorded lazily by the NEXT call when it arrives on another stream (back-to-back calls on one stream pay for no
  // event).  That needs this stream to be alive then: a stream handed in by the caller (not the plan's own, not the null stream) may be
  // destroyed before the next call, so for such a stream the event is recorded now, while the handle is known to be good, whenever
  // the stream differs from the previous call's (a caller cycling through streams) -- the common case, one long-lived stream, stays free.
  if (s != pl->stream && s != nullptr && pl->busy_valid && pl->busy_stream != s) {
    GCMF_HIP(hipEventRecord(pl->ev_busy, s));
    pl->busy_recorded = true;
  } else {
    pl->busy_recorded = false;
  }
  pl->busy_stream = s;
  pl->busy_valid = true;
  pl->last_launches = timed ? x.launches : pl->last_launches + x.launches;
  if (!on_dev) {
    for (int k = 0; k < pl->ncomp; ++k)
      GCMF_HIP(hipMemcpyAsync(out[k], x.dout[k], out_bytes, hipMemcpyDeviceToHost, s));
    GCMF_HIP(hipStreamSynchronize(s));
    const unsigned rlo = pl->res_lo, rhi = pl->res_hi;
    pl->res_lo = pl->res_hi = 0;   // (the stream is drained: nothing of this call is pending any more)
    if (rlo && resident_take_failure(pl->d.device, rlo, rhi)) {   // (the synchronising host path can tell for THIS call)
      set_error("k_resident: the on-chip launch timed out waiting for a neighbour tile: the result is NaN (another process running "
                "resident kernels on this GPU?); the strip-marching launches are used from now on");
      return GCMF_ERR_HIP;
    }
  }
  if (timing) {
    GCMF_HIP(hipEventSynchronize(pl->ev1));
    GCMF_HIP(hipEventElapsedTime(&pl->last_ms, pl->ev0, pl->ev1));
  }
  if (pl->timing_detail && timed && (rc = dom_collect(pl))) return rc;
  return GCMF_OK;
}

// Shared driver of gcmf_apply, the banks and gcmf_laplacian: ONE launch's worth of entries; the plan's mutex is held and the device is current.
// base: the view the caller runs on -- the plan's own, with entry0 = the first entry of this launch within the call and, inside a bank,
// the bank's fields and table rows; the flags put the call's own mask bytes or folded planes into it.  fold: gcmf_apply_bank_gaps' memo.
// `timed` = false: the caller (the pipelined host path) brackets the launches with the timing events itself.
static int run_whole_locked(gcmf_plan *pl, const CallView &base, GapFold *fold, const double *p, int n_steps, double c, const void *const *in,
                            void *const *out, int64_t nbatch, uint32_t flags, void *stream, bool lapl_only, bool timed,
                            const Adjoint *adj = nullptr) {
  const bool on_dev = flags & GCMF_DEVICE_PTRS;
  ApplyCtx x{};
  x.pl = pl;
  x.cv = base;
  // device pointers: run on exactly the caller's stream (NULL = the HIP default stream) so the work is
  // ordered with the caller's own kernels; host pointers: the plan's private stream unless one is given
  x.s = (on_dev || stream) ? (hipStream_t)stream : pl->stream;
  x.p = p; x.n_steps = n_steps; x.c = c; x.nbatch = nbatch; x.rows = (int)pl->rows_alloc;
  const bool f32 = pl->d.dtype == GCMF_F32;
  x.fb32 = f32 && (flags & GCMF_OUT_F32);
  const size_t ts = dtype_size(pl->d.dtype);
  const size_t fbs = lapl_only ? ts : ((f32 && !x.fb32) ? 8 : ts);  // element size of fbar == element size of `out`
  const size_t ncell = (size_t)nbatch * pl->d.ny * pl->d.nx;
  const bool prep = pl->area_weighted && !lapl_only;

  // work layout per component: [A][B][fbar] (+ [prepared T0]) (+ host staging: [in][out])
  const size_t szT = align_up(ncell * ts, 256), szF = align_up(ncell * fbs, 256);
  const bool use_multi = !lapl_only && pl->multi_s >= 2 && n_steps >= 2 && multi_supported(pl, 2);
  const bool use_vmulti = !lapl_only && pl->multi_s >= 2 && n_steps >= 2 && vec_multi_supported(pl, nbatch, 2);
  size_t per = 0;
  const size_t oA = per; per += szT;
  const size_t oB = per; per += szT;
  const size_t oC = per; if (use_multi || use_vmulti) per += szT;
  const size_t oD = per; if (use_multi || use_vmulti) per += szT;
  const size_t oF = per; per += szF;
  // second fbar plane (scalar blocked schedule): k_ring re-does a strip from its inputs when it meets a NaN / inf,
  // so a launch must not accumulate fbar in place
  const size_t oF2 = per; if (use_multi) per += szF;
  const size_t oP = per; if (prep) per += szT;
  const size_t oIn = per; if (!on_dev) per += szT;
  const size_t oOut = per; if (!on_dev) per += szF;
  const bool from_nan = flags & GCMF_MASK_FROM_NAN;   // (run_whole has checked the plan: one component, a land-mask kind)
  const size_t oM = per; if (from_nan) per += align_up(ncell, 256);   // the entries' own mask bytes
  // GCMF_FACES_FROM_NAN (run_whole has checked the plan and cut the batch to the scratch bound): the entries' own cE, cN, ra and land bytes
  const bool faces = flags & GCMF_FACES_FROM_NAN;
  // (inside gcmf_apply_bank_gaps: the FIELDS' own planes, bank_nfield of them whatever the launch's entries)
  const bool bank_faces = faces && base.bank_n > 0;
  const int64_t nfold = bank_faces ? base.bank_nfield : nbatch;
  const size_t nface = (size_t)nfold * pl->d.ny * pl->d.nx;
  const size_t szG = align_up(nface * 8 + 256, 256), szL = align_up(nface + 256, 256);   // (padded as precompute_levels pads a stacked plan's)
  const size_t oG = per; if (faces) per += 3 * szG + szL;
  // gcmf_apply_adjoint: the pre-scaled input, behind everything a forward call lays out (host pointers: and the staged `like`)
  const bool adj_like = adj && adj->has_like;
  const size_t oAdj = per; if (adj) per += szT;
  const size_t oLike = per; if (adj_like && !on_dev) per += szT;
  int rc = ensure_work(pl, per * pl->ncomp);
  if (rc || (rc = wait_for_work(pl, x.s))) return rc;
  char *w = (char *)pl->work;
  // the four state planes of a scalar blocked schedule, one after the other: what a wet-row table launch zero-fills once (pool_clean)
  void *pool_base = w + oA;
  const size_t pool_bytes = (pl->ncomp == 1 && use_multi) ? 4 * szT : 0;
  if (pool_base != pl->pool_base || pool_bytes != pl->pool_bytes) pl->pool_clean = false;
  pl->pool_base = pool_base;
  pl->pool_bytes = pool_bytes;
  x.F2 = w + oF2;
  for (int k = 0; k < pl->ncomp; ++k) {
    char *base = w + per * k;
    x.A[k] = base + oA; x.B[k] = base + oB; x.Cb[k] = base + oC; x.Db[k] = base + oD; x.F[k] = base + oF; x.Pp[k] = base + oP;
    if (on_dev) {
      x.din[k] = in[k];
      x.dout[k] = out[k];
    } else {
      x.din[k] = base + oIn;
      x.dout[k] = base + oOut;
      GCMF_HIP(hipMemcpyAsync(base + oIn, in[k], ncell * ts, hipMemcpyHostToDevice, x.s));
    }
  }
  const void *dlike[2] = {nullptr, nullptr};
  for (int k = 0; adj_like && k < pl->ncomp; ++k) {
    dlike[k] = adj->like[k];
    if (!on_dev) {
      dlike[k] = w + per * k + oLike;
      GCMF_HIP(hipMemcpyAsync(w + per * k + oLike, adj->like[k], ncell * ts, hipMemcpyHostToDevice, x.s));
    }
  }
  // (the adjoint of a flagged call: the gaps are those of the forward call's input)
  const void *gaps_of = adj ? dlike[0] : x.din[0];
  const bool timing = pl->timing && timed;
  if (timing) GCMF_HIP(hipEventRecord(pl->ev0, x.s));
  CallView &cv = x.cv;
  if (from_nan) {   // the call's own mask bytes where the launchers look for the plan's; the plan's land count does not apply to them
    uint8_t *bits = (uint8_t *)(w + oM);
    if ((rc = launch_field_masks(pl, pl->g.mbits, gaps_of, bits, nbatch, x.s))) return rc;
    ++x.launches;
    cv.mbits = cv.lbits = bits;
    cv.n_land = std::max<int64_t>(1, pl->n_land);
    cv.mask_per_field = 1;
  }
  if (faces) {   // the view of a stacked plan whose levels are this launch's entries (a bank: its fields, entry0 kept -- see apply_bank)
    double *cEb = (double *)(w + oG), *cNb = (double *)(w + oG + szG), *rab = (double *)(w + oG + 2 * szG);
    uint8_t *bits = (uint8_t *)(w + oG + 3 * szG);
    cv.coef[0] = cEb; cv.coef[1] = cNb; cv.coef[2] = rab;
    cv.lbits = bits;
    cv.n_land = std::max<int64_t>(1, pl->n_land);
    cv.stacked = true;
    cv.nlev = nfold;
    if (!bank_faces) cv.entry0 = 0;
    int depths[1024];   // (asked of the call's view: the answer run_schedule will get)
    if (!use_multi || clenshaw_cut(pl, cv, n_steps, depths, 1024, false, nbatch) <= 0) {
      set_error("%s; for this plan and a polynomial of %d steps the stacked strips offer no backward cut (gcmf_clenshaw_cut_batch: fewer than "
                "five steps, nx not a multiple of 4, GCMF_CLENSHAW=0 ...): filter with a plan built from wet_mask * [not NaN]",
                bank_faces ? "gcmf_apply_bank_gaps" : FACES_WHERE, n_steps);
      return GCMF_ERR_UNSUPPORTED;
    }
    // (a bank: one fold per FIELD -- a later launch of the same call that finds the same fields folded at the same place folds nothing)
    if (!(fold && fold->at == (const void *)cEb && fold->in == x.din[0] && fold->n == nfold)) {
      if ((rc = launch_gap_fold(pl, (const double *)pl->g.coef[0], (const double *)pl->g.coef[1], (const double *)pl->g.coef[2], gaps_of, cEb, cNb,
                                rab, bits, nfold, x.s)))
        return rc;
      ++x.launches;
      if (fold) *fold = GapFold{x.din[0], cEb, nfold};
    }
  }
  if (adj) {   // in / D into the scratch plane, with the view's planes
    // Where `like` is NaN the schedule must see NaN again: the forward call read that cell as the value 0 at EVERY step (nan_to_num inside
    // the stencil), so what it applied to the finite cells is the polynomial of the principal submatrix on them -- whose transpose is that
    // submatrix's polynomial again, not the filter with the cell set to 0 once and left to evolve.  (A flagged call derives its gaps from
    // those NaNs besides.)  The REGULAR kinds' stencil reads a NaN as a NaN, which spreads: there is no derivative to keep, the cell is 0.
    void *scr[2] = {w + oAdj, w + per + oAdj};
    if ((rc = launch_adjoint_scale(pl, cv, false, x.din, scr, adj_like ? dlike : nullptr, x.fb32, pl->kind != K_REG, nbatch, x.s))) return rc;
    for (int k = 0; k < pl->ncomp; ++k) x.din[k] = scr[k];
    x.launches += pl->ncomp;
  }
  if ((rc = lapl_only ? lapl_step(x) : run_schedule(x, flags, use_multi, use_vmulti))) return rc;
  if (adj) {   // ... and the result times D, in place; 0 where `like` is NaN
    if ((rc = launch_adjoint_scale(pl, cv, true, x.dout, x.dout, adj_like ? dlike : nullptr, x.fb32, false, nbatch, x.s))) return rc;
    x.launches += pl->ncomp;
  }
  return finish_call(x, on_dev, out, ncell * fbs, timing, timed);
}

// Host pointers and a batch of fields: the batch is cut into chunks of ~32 MB per component that stream through two
// staging slots in HBM -- upload of chunk k+1 and download of chunk k-1 run on their own streams while chunk k is
// filtered ("overlap H2D of chunk k+1 with compute of chunk k").  The host issues upload(k+1) and the
// launches of chunk k+1 BEFORE download(k), so that a blocking download into pageable memory still overlaps with compute.
static int run_host_pipelined(gcmf_plan *pl, CallView cv, const double *p, int n_steps, double c, const void *const *in,
                              void *const *out, int64_t nbatch, uint32_t flags, void *stream, bool lapl_only,
                              int64_t chunk_nb) {
  const int nc = pl->ncomp;
  const bool f32 = pl->d.dtype == GCMF_F32;
  const size_t ts = dtype_size(pl->d.dtype);
  const size_t fbs = lapl_only ? ts : ((f32 && !(flags & GCMF_OUT_F32)) ? 8 : ts);
  const size_t cell = (size_t)pl->d.ny * pl->d.nx;
  const size_t szI = align_up((size_t)chunk_nb * cell * ts, 256), szO = align_up((size_t)chunk_nb * cell * fbs, 256);
  const size_t need = (size_t)nc * 2 * (szI + szO);
  if (need > pl->stage_bytes) {
    if (pl->stage) GCMF_HIP(hipFree(pl->stage));
    pl->stage = nullptr;
    pl->stage_bytes = 0;
    GCMF_HIP(hipMalloc(&pl->stage, need));
    pl->stage_bytes = need;
  }
  if (!pl->s_in) {
    GCMF_HIP(hipStreamCreateWithFlags(&pl->s_in, hipStreamNonBlocking));
    GCMF_HIP(hipStreamCreateWithFlags(&pl->s_out, hipStreamNonBlocking));
    for (int q = 0; q < 2; ++q) {
      GCMF_HIP(hipEventCreateWithFlags(&pl->ev_in[q], hipEventDisableTiming));
      GCMF_HIP(hipEventCreateWithFlags(&pl->ev_cmp[q], hipEventDisableTiming));
      GCMF_HIP(hipEventCreateWithFlags(&pl->ev_out[q], hipEventDisableTiming));
    }
  }
  hipStream_t s_cmp = stream ? (hipStream_t)stream : pl->stream;
  char *base = (char *)pl->stage;
  auto In = [&](int slot, int k) { return base + ((size_t)(slot * nc + k)) * szI; };
  auto Out = [&](int slot, int k) { return base + (size_t)2 * nc * szI + ((size_t)(slot * nc + k)) * szO; };
  const int64_t nchunks = (nbatch + chunk_nb - 1) / chunk_nb;
  auto nb_of = [&](int64_t ch) { return ch == nchunks - 1 ? nbatch - ch * chunk_nb : chunk_nb; };
  const uint32_t dflags = flags | GCMF_DEVICE_PTRS;
  int rc = GCMF_OK;
  pl->last_launches = 0;

  auto upload_and_launch = [&](int64_t ch) -> int {
    const int slot = (int)(ch & 1);
    const int64_t nb = nb_of(ch);
    if (ch >= 2) GCMF_HIP(hipStreamWaitEvent(pl->s_in, pl->ev_cmp[slot], 0));  // In[slot] was read by chunk ch-2
    for (int k = 0; k < nc; ++k)
      GCMF_HIP(hipMemcpyAsync(In(slot, k), (const char *)in[k] + (size_t)ch * chunk_nb * cell * ts, (size_t)nb * cell * ts,
                              hipMemcpyHostToDevice, pl->s_in));
    GCMF_HIP(hipEventRecord(pl->ev_in[slot], pl->s_in));
    GCMF_HIP(hipStreamWaitEvent(s_cmp, pl->ev_in[slot], 0));
    if (ch >= 2) GCMF_HIP(hipStreamWaitEvent(s_cmp, pl->ev_out[slot], 0));  // Out[slot] was drained by chunk ch-2
    if (ch == 0 && pl->timing) GCMF_HIP(hipEventRecord(pl->ev0, s_cmp));
    const void *din[2] = {In(slot, 0), nc > 1 ? In(slot, 1) : nullptr};
    void *dout[2] = {Out(slot, 0), nc > 1 ? Out(slot, 1) : nullptr};
    cv.entry0 = ch * chunk_nb;   // (stacked plans: the chunk's entry b is entry ch * chunk_nb + b of the call)
    int r = run_whole_locked(pl, cv, nullptr, p, n_steps, c, din, dout, nb, dflags, (void *)s_cmp, lapl_only, false);
    if (r) return r;
    if (ch == nchunks - 1 && pl->timing) GCMF_HIP(hipEventRecord(pl->ev1, s_cmp));
    GCMF_HIP(hipEventRecord(pl->ev_cmp[slot], s_cmp));
    return GCMF_OK;
  };
  auto download = [&](int64_t ch) -> int {
    const int slot = (int)(ch & 1);
    const int64_t nb = nb_of(ch);
    GCMF_HIP(hipStreamWaitEvent(pl->s_out, pl->ev_cmp[slot], 0));
    for (int k = 0; k < nc; ++k)
      GCMF_HIP(hipMemcpyAsync((char *)out[k] + (size_t)ch * chunk_nb * cell * fbs, Out(slot, k), (size_t)nb * cell * fbs,
                              hipMemcpyDeviceToHost, pl->s_out));
    GCMF_HIP(hipEventRecord(pl->ev_out[slot], pl->s_out));
    return GCMF_OK;
  };

  // Page-lock the caller's input for the duration of the call: uploads from pageable memory block the host and do
  // not overlap with the downloads (2.5 ms per 69 MB field); from registered memory they are plain asynchronous DMA and
  // the pipeline runs at the filter's own rate (1.65 ms).  Registration is best effort (already page-locked or
  // read-only mappings simply stay as they are).
  bool registered[2] = {false, false};
  if (pl->host_register)
    for (int k = 0; k < nc; ++k) {
      registered[k] = host_register(in[k], (size_t)nbatch * cell * ts);
    }
  auto finish = [&](int r) {
    (void)hipStreamSynchronize(pl->s_in);
    (void)hipStreamSynchronize(pl->s_out);
    (void)hipStreamSynchronize(s_cmp);
    for (int k = 0; k < nc; ++k)
      if (registered[k]) host_unregister(in[k]);
    return r;
  };
  // Order of the enqueues (round 5): the download of chunk ch goes out BEFORE the upload of chunk ch + 2, so that an upload that blocks the
  // calling thread (memory that could not be page-locked) never holds a download back.  Measured (tools/measure_host_batch.py, 12 fields of
  // 2400 x 3600 f64): 2.7 ms per field either way with a freshly registered input, 1.6 ms with an input that is ALREADY page-locked (a torch
  // pinned tensor): what separates the two is the per-call hipHostRegister / unregister of the caller's array (~1 ms per 69 MB), not the
  // order of the copies -- and a registration cache would only help a caller that passes the same buffer again.
  if ((rc = upload_and_launch(0))) return finish(rc);
  if (nchunks > 1 && (rc = upload_and_launch(1))) return finish(rc);
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    if ((rc = download(ch))) return finish(rc);
    if (ch + 2 < nchunks && (rc = upload_and_launch(ch + 2))) return finish(rc);
  }
  if ((rc = finish(GCMF_OK))) return rc;
  if (pl->timing) GCMF_HIP(hipEventElapsedTime(&pl->last_ms, pl->ev0, pl->ev1));
  return GCMF_OK;
}

// GCMF_FACES_FROM_NAN: the entries (a bank: the fields) one launch may carry -- their own planes (25 bytes per cell and entry) at or under
// option "gap_scratch_mb", at least one
static int64_t gap_launch_entries(const gcmf_plan *pl) {
  const long long bound = (long long)std::max(0, pl->gap_scratch_mb) << 20, per_entry = 25LL * pl->d.ny * pl->d.nx;
  return std::max<int64_t>(1, std::min<int64_t>(MAX_LAUNCH_BATCH, bound / per_entry));
}

// What the launches of one call add up to: gcmf_last_ms and gcmf_last_launches report the call
struct Tally {
  float ms = 0.f;
  int launches = 0;
  int leave(gcmf_plan *pl) const {
    pl->last_ms = ms;
    pl->last_launches = launches;
    return GCMF_OK;
  }
};

// nent entries in consecutive launches of at most launch_nb: launch k starts in_stride / out_stride bytes x its first entry into every
// component of `in` / `out` (in_stride 0: a bank, whose every launch reads all the fields) and an entry keeps its place in the call through
// the view's entry0, which counts on from cv.entry0.
static int run_launches(gcmf_plan *pl, CallView cv, GapFold *fold, const double *p, int n_steps, double c, const void *const *in, size_t in_stride,
                        void *const *out, size_t out_stride, int64_t nent, int64_t launch_nb, uint32_t flags, void *stream, bool lapl_only, Tally &t,
                        const Adjoint *adj = nullptr) {
  const int64_t first = cv.entry0;
  for (int64_t e0 = 0; e0 < nent; e0 += launch_nb) {
    const void *in2[2] = {nullptr, nullptr};
    void *out2[2] = {nullptr, nullptr};
    for (int k = 0; k < pl->ncomp; ++k) {
      in2[k] = (const char *)in[k] + (size_t)e0 * in_stride;
      out2[k] = (char *)out[k] + (size_t)e0 * out_stride;
    }
    cv.entry0 = first + e0;
    Adjoint adj2;
    if (adj) {
      adj2 = *adj;
      for (int k = 0; k < pl->ncomp && adj->has_like; ++k) adj2.like[k] = (const char *)adj->like[k] + (size_t)e0 * in_stride;
    }
    const int rc = run_whole_locked(pl, cv, fold, p, n_steps, c, in2, out2, std::min(nent - e0, launch_nb), flags, stream, lapl_only, true,
                                    adj ? &adj2 : nullptr);
    if (rc) return rc;
    t.ms += pl->last_ms;
    t.launches += pl->last_launches;
  }
  return GCMF_OK;
}

// adj: gcmf_apply_adjoint (like: null or its `like` argument)
static int run_whole(gcmf_plan *pl, const double *p, int n_steps, double c, const void *const *in, void *const *out,
                     int64_t nbatch, uint32_t flags, void *stream, bool lapl_only, bool adj = false, const void *const *like = nullptr) {
  const char *who = adj ? "gcmf_apply_adjoint" : lapl_only ? "gcmf_laplacian" : "gcmf_apply";
  if (!pl || !in || !out || nbatch < 0 || (!lapl_only && (!p || n_steps < 1))) {
    set_error("%s: bad argument", adj ? who : "gcmf_apply");
    return GCMF_ERR_INVALID_ARG;
  }
  for (int k = 0; k < pl->ncomp; ++k)
    if (!in[k] || !out[k] || (like && !like[k])) {
      set_error("%s: null component pointer", adj ? who : "gcmf_apply");
      return GCMF_ERR_INVALID_ARG;
    }
  for (int k = 0; k < pl->ncomp; ++k)
    for (int q = 0; q < pl->ncomp; ++q)
      if (in[k] == out[q]) {  // (the ranges are compared below, once the plan is known to cover the whole grid: their size is ny * nx)
        set_error("%s: `out` must not alias `in` (filtering in place is not supported)", who);
        return GCMF_ERR_INVALID_ARG;
      }
  if (adj) {
    // F^T = D F D^-1 needs a diagonal D: the B-grid Laplacian has none (sign(L_ij) != sign(L_ji) on part of its couplings)
    const char *why = pl->d.grid_type == GCMF_VECTOR_B_GRID ? "VECTOR_B_GRID has no diagonal symmetrizer: its adjoint needs a transposed stencil kernel" :
                      (pl->d.flags & GCMF_PLAN_SELF_RING) ? "not available on a GCMF_PLAN_SELF_RING plan" :
                      !pl->full ? "not available on a row slab: it needs a plan covering the whole grid" : nullptr;
    if (why) {
      set_error("gcmf_apply_adjoint: %s (grid type %d)", why, pl->d.grid_type);
      return GCMF_ERR_UNSUPPORTED;
    }
    if ((flags & (GCMF_MASK_FROM_NAN | GCMF_FACES_FROM_NAN)) && !like) {
      set_error("gcmf_apply_adjoint: GCMF_MASK_FROM_NAN / GCMF_FACES_FROM_NAN need `like`, the forward call's input: the gaps are its NaNs");
      return GCMF_ERR_INVALID_ARG;
    }
  }
  if (flags & GCMF_FACES_FROM_NAN) {
    const int gt = pl->d.grid_type;
    const bool kind_ok = gt == GCMF_IRREGULAR_WITH_LAND || gt == GCMF_MOM5U || gt == GCMF_MOM5T;
    const char *why = lapl_only ? "this is gcmf_laplacian" : !kind_ok ? "another grid type" : pl->d.dtype != GCMF_F64 ? "an f32 plan" : !pl->full ? "a row slab" :
                      pl->stacked ? "a stacked plan (gcmf_plan_create_levels)" : (flags & GCMF_FORWARD_RECURRENCE) ? "combined with GCMF_FORWARD_RECURRENCE" :
                      (flags & GCMF_MASK_FROM_NAN) ? "combined with GCMF_MASK_FROM_NAN" : nullptr;
    if (why) {
      set_error("%s (%s; grid type %d)", FACES_WHERE, why, gt);
      return GCMF_ERR_UNSUPPORTED;
    }
  }
  if ((flags & GCMF_MASK_FROM_NAN) && (lapl_only || pl->kind != K_MASK || !pl->full)) {
    set_error("GCMF_MASK_FROM_NAN is a gcmf_apply flag for whole-grid plans of REGULAR_WITH_LAND, REGULAR_WITH_LAND_AREA_WEIGHTED and "
              "TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED (this %s grid type %d%s)", lapl_only ? "is gcmf_laplacian on" : "plan has",
              pl->d.grid_type, pl->full ? "" : ", a row slab");
    return GCMF_ERR_UNSUPPORTED;
  }
  if (!pl->full) {
    set_error("gcmf_apply / gcmf_laplacian need a plan covering the whole grid; use gcmf_cheb_step on row slabs");
    return GCMF_ERR_INVALID_ARG;
  }
  if (pl->stacked) {   // (GCMF_MASK_FROM_NAN: refused above, the flux kinds have no mask bytes)
    if (lapl_only) {
      set_error("gcmf_laplacian: not available on a stacked plan (gcmf_plan_create_levels): build one plan per level");
      return GCMF_ERR_UNSUPPORTED;
    }
    if (flags & GCMF_FORWARD_RECURRENCE) {
      set_error("gcmf_apply: GCMF_FORWARD_RECURRENCE is not available on a stacked plan (gcmf_plan_create_levels), whose levels only the "
                "backward evaluation's strips address: build one plan per level");
      return GCMF_ERR_UNSUPPORTED;
    }
    if (nbatch % pl->nlev) {
      set_error("gcmf_apply: a stacked plan of %lld levels takes batches that are multiples of it (entry b runs on level b %% nlev), not %lld",
                (long long)pl->nlev, (long long)nbatch);
      return GCMF_ERR_INVALID_ARG;
    }
  }
  {
    // `out` against `in` and against the other `out` plane as BYTE RANGES, as gcmf_apply_bank compares them, host and device pointers
    // alike (here, where the plan is known to cover the whole grid: a plane is nbatch * ny * nx elements): the input is read by the first launch, by
    // neighbouring strips, by later launches of the backward evaluation and by k_land_fix at the end, so an `out` that starts a row or a
    // batch entry into `in` is as wrong as out == in.  (in[0] == in[1] is fine: nothing writes the input.)
    const size_t cells = (size_t)nbatch * (size_t)pl->d.ny * (size_t)pl->d.nx, its = dtype_size(pl->d.dtype);
    const size_t ots = lapl_only ? its : ((pl->d.dtype == GCMF_F32 && !(flags & GCMF_OUT_F32)) ? 8 : its);
    for (int q = 0; q < pl->ncomp; ++q) {
      const uintptr_t o0 = (uintptr_t)out[q], o1 = o0 + cells * ots;
      for (int k = 0; like && k < pl->ncomp; ++k) {
        const uintptr_t l0 = (uintptr_t)like[k], l1 = l0 + cells * its;
        if (l0 < o1 && o0 < l1) {
          set_error("%s: `out` must not alias `like`: the %zu bytes of out[%d] overlap the %zu bytes of like[%d]", who, cells * ots, q,
                    cells * its, k);
          return GCMF_ERR_INVALID_ARG;
        }
      }
      for (int k = 0; k < pl->ncomp; ++k) {
        const uintptr_t i0 = (uintptr_t)in[k], i1 = i0 + cells * its;
        if (in[k] == out[q] || (i0 < o1 && o0 < i1)) {
          set_error("%s: `out` must not alias `in`: the %zu bytes of out[%d] overlap the %zu bytes of in[%d] (filtering in place is not "
                    "supported)", who, cells * ots, q, cells * its, k);
          return GCMF_ERR_INVALID_ARG;
        }
      }
      for (int k = 0; k < q; ++k) {
        const uintptr_t p0 = (uintptr_t)out[k], p1 = p0 + cells * ots;
        if (out[k] == out[q] || (p0 < o1 && o0 < p1)) {
          set_error("%s: the %zu bytes of out[%d] overlap those of out[%d]: the components' results need planes of their own", who,
                    cells * ots, q, k);
          return GCMF_ERR_INVALID_ARG;
        }
      }
    }
  }
  if (nbatch == 0) return GCMF_OK;
  std::lock_guard<std::mutex> lk(pl->mu);
  GCMF_HIP(hipSetDevice(pl->d.device));
  // the most entries one launch takes: the scalar kernels index the batch with gridDim.y (<= 65535)
  int64_t launch_nb = (flags & GCMF_FACES_FROM_NAN) ? gap_launch_entries(pl) : MAX_LAUNCH_BATCH;
  if (adj) {   // the scratch plane of every component and entry of a launch at or under option "adjoint_scratch_mb", at least one entry
    const long long bound = (long long)std::max(0, pl->adjoint_scratch_mb) << 20;
    const long long per_entry = (long long)pl->ncomp * pl->d.ny * pl->d.nx * (long long)dtype_size(pl->d.dtype);
    launch_nb = std::max<int64_t>(1, std::min<int64_t>(launch_nb, bound / per_entry));
  }
  // (the adjoint stages host planes through HBM one launch at a time: no chunk pipeline)
  if (!adj && !(flags & GCMF_DEVICE_PTRS) && nbatch > 1 && pl->host_chunk_bytes > 0) {
    const size_t entry = (size_t)pl->d.ny * pl->d.nx * dtype_size(pl->d.dtype);
    int64_t chunk_nb = (int64_t)(pl->host_chunk_bytes / entry);
    if (chunk_nb < 1) chunk_nb = 1;
    if (chunk_nb > launch_nb) chunk_nb = launch_nb;
    if (chunk_nb < nbatch) return run_host_pipelined(pl, own_view(pl), p, n_steps, c, in, out, nbatch, flags, stream, lapl_only, chunk_nb);
  }
  // (more than one launch: very long batches of small fields, and batches whose per-entry planes exceed the scratch bound)
  const size_t cell = (size_t)pl->d.ny * pl->d.nx, ts = dtype_size(pl->d.dtype);
  const size_t fbs = lapl_only ? ts : ((pl->d.dtype == GCMF_F32 && !(flags & GCMF_OUT_F32)) ? 8 : ts);
  Tally t;
  Adjoint a;
  for (int k = 0; like && k < pl->ncomp; ++k) a.like[k] = like[k];
  a.has_like = like != nullptr;
  const int rc = run_launches(pl, own_view(pl), nullptr, p, n_steps, c, in, cell * ts, out, cell * fbs, nbatch, launch_nb, flags, stream, lapl_only, t,
                              adj ? &a : nullptr);
  return rc ? rc : t.leave(pl);
}

int gcmf_apply(gcmf_plan *pl, const double *p, int n_steps, double c, const void *const *in, void *const *out,
               int64_t nbatch, uint32_t flags, void *stream) {
  return run_whole(pl, p, n_steps, c, in, out, nbatch, flags, stream, false);
}

int gcmf_apply_adjoint(gcmf_plan *pl, const double *p, int n_steps, double c, const void *const *in, const void *const *like,
                       void *const *out, int64_t nbatch, uint32_t flags, void *stream) {
  return run_whole(pl, p, n_steps, c, in, out, nbatch, flags, stream, false, true, like);
}

// The two coefficient tables of a filter bank on the device (gcmf_plan::bank_rev / bank_fwd), uploaded only when they changed -- as
// ensure_dev_p: the previous call's kernels may still be reading the old ones, so the stream is drained first (and the device, when
// that call ran on another stream)
static int ensure_bank_tables(gcmf_plan *pl, const double *p, int nbank, int n_steps, hipStream_t s) {
  const size_t stride = (size_t)n_steps + 1, n = (size_t)nbank * stride;
  if (pl->bank_cap < n) {
    if (pl->bank_rev) GCMF_HIP(hipFree(pl->bank_rev));
    pl->bank_rev = nullptr;
    if (pl->bank_fwd) GCMF_HIP(hipFree(pl->bank_fwd));
    pl->bank_fwd = nullptr;
    pl->bank_cap = 0;
    pl->bank_host.clear();
    GCMF_HIP(hipMalloc((void **)&pl->bank_rev, n * sizeof(double)));
    GCMF_HIP(hipMalloc((void **)&pl->bank_fwd, n * sizeof(double)));
    pl->bank_cap = n;
  }
  if (pl->bank_stride != stride || pl->bank_host.size() != n || memcmp(pl->bank_host.data(), p, n * sizeof(double)) != 0) {
    pl->bank_host.assign(p, p + n);
    pl->bank_stride = stride;
    std::vector<double> rev(n);
    for (int j = 0; j < nbank; ++j)
      for (size_t q = 0; q < stride; ++q) rev[j * stride + q] = p[j * stride + (stride - 1 - q)];
    GCMF_HIP(hipStreamSynchronize(s));  // nothing may still read the old coefficients
    if (pl->busy_valid && pl->busy_stream != s) GCMF_HIP(hipDeviceSynchronize());
    GCMF_HIP(hipMemcpy(pl->bank_fwd, pl->bank_host.data(), n * sizeof(double), hipMemcpyHostToDevice));
    GCMF_HIP(hipMemcpy(pl->bank_rev, rev.data(), n * sizeof(double), hipMemcpyHostToDevice));
  }
  return GCMF_OK;
}

// gcmf_apply_bank and (gaps) gcmf_apply_bank_gaps: the same call but for the grid types, one flag and the fold.
// On gappy fields the launches run on the planes GCMF_FACES_FROM_NAN folds, once per FIELD: the view carries the bank AND, from
// run_whole_locked, a level axis of one level per field, and launch_ringc / run_schedule pick the forms that know both.
static int apply_bank(const char *who, bool gaps, gcmf_plan *pl, const double *p, int nbank, int n_steps, double c, const void *in, void *out,
                      int64_t nfield, uint32_t flags, void *stream) {
  if (!pl || !p || !in || !out) {
    set_error("%s: null argument", who);
    return GCMF_ERR_INVALID_ARG;
  }
  if (nbank < 1 || n_steps < 1 || nfield < 0) {
    set_error("%s: %d polynomials of %d steps on %lld fields (at least one polynomial of at least one step)", who, nbank, n_steps, (long long)nfield);
    return GCMF_ERR_INVALID_ARG;
  }
  const int gt = pl->d.grid_type;
  const bool pop = gt == GCMF_TRIPOLAR_POP_WITH_LAND, kind_ok = gt == GCMF_IRREGULAR_WITH_LAND || gt == GCMF_MOM5U || gt == GCMF_MOM5T || pop;
  const char *why = (gaps && pop) ? "TRIPOLAR_POP_WITH_LAND, whose gap fold is not offered" : !kind_ok ? "another grid type" :
                    pl->d.dtype != GCMF_F64 ? "an f32 plan" : (pl->d.flags & GCMF_PLAN_SELF_RING) ? "GCMF_PLAN_SELF_RING" : !pl->full ? "a row slab" :
                    pl->stacked ? "a stacked plan (gcmf_plan_create_levels)" : !(flags & GCMF_DEVICE_PTRS) ? "host pointers (GCMF_DEVICE_PTRS is required)" :
                    (flags & GCMF_FORWARD_RECURRENCE) ? "GCMF_FORWARD_RECURRENCE" : (flags & GCMF_MASK_FROM_NAN) ? "GCMF_MASK_FROM_NAN" :
                    (!gaps && (flags & GCMF_FACES_FROM_NAN)) ? "GCMF_FACES_FROM_NAN" : (flags & GCMF_OUT_F32) ? "GCMF_OUT_F32" : nullptr;
  if (why) {
    set_error(gaps ? "%s: filter banks on gappy fields run on ordinary whole-grid f64 plans of IRREGULAR_WITH_LAND, MOM5U and MOM5T with device "
                     "pointers, backwards and into f64 (%s; grid type %d): call gcmf_apply with GCMF_FACES_FROM_NAN once per polynomial"
                   : "%s: filter banks run on ordinary whole-grid f64 plans of IRREGULAR_WITH_LAND, MOM5U, MOM5T and TRIPOLAR_POP_WITH_LAND with device pointers, "
                     "backwards, on the plan's own mask and into f64 (%s; grid type %d): call gcmf_apply once per polynomial",
              who, why, gt);
    return GCMF_ERR_UNSUPPORTED;
  }
  const size_t cell = (size_t)pl->d.ny * pl->d.nx;
  if ((int64_t)nbank * nfield > (int64_t)2000000000) {
    set_error("%s: %d polynomials x %lld fields: at most 2e9 entries per call", who, nbank, (long long)nfield);
    return GCMF_ERR_INVALID_ARG;
  }
  const int64_t nent = (int64_t)nbank * nfield;
  {
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (size_t)nfield * cell * 8, o0 = (uintptr_t)out, o1 = o0 + (size_t)nent * cell * 8;
    if ((nfield > 0 && i0 < o1 && o0 < i1) || in == out) {   // (the fold,) every launch and k_land_fix read the input
      set_error("%s: `out` must not overlap `in` (filtering in place is not supported)", who);
      return GCMF_ERR_INVALID_ARG;
    }
  }
  int depths[1024];
  // (gaps: the folded planes always have land -- the gaps -- so what a plan without land may skip is needed here: land_ok)
  if ((gaps && ((pl->d.nx % 4) != 0 || !pl->zero_land || n_steps >= 4096)) || bank_cut(pl, own_view(pl), n_steps, std::max<int64_t>(1, nent), depths, 1024) <= 0) {
    if (gaps)
      set_error("%s: for this plan and a polynomial of %d steps the plain strips offer no backward cut (gcmf_bank_cut returns 0: fewer "
                "than five steps, GCMF_CLENSHAW=0 ...; or nx = %lld is not a multiple of 4, 4096 steps or more, GCMF_ZERO_LAND=0): call gcmf_apply with "
                "GCMF_FACES_FROM_NAN once per polynomial", who, n_steps, (long long)pl->d.nx);
    else
      set_error("%s: for this plan and a polynomial of %d steps the plain strips offer no backward cut (gcmf_bank_cut returns 0: fewer "
                "than five steps, nx = %lld not a multiple of 4 on a grid with land, GCMF_CLENSHAW=0 ...): call gcmf_apply once per polynomial",
                who, n_steps, (long long)pl->d.nx);
    return GCMF_ERR_UNSUPPORTED;
  }
  if (nfield == 0) return GCMF_OK;
  std::lock_guard<std::mutex> lk(pl->mu);
  GCMF_HIP(hipSetDevice(pl->d.device));
  int rc = ensure_bank_tables(pl, p, nbank, n_steps, (hipStream_t)stream);
  if (rc) return rc;
  const uint32_t rflags = GCMF_DEVICE_PTRS | GCMF_NO_RESIDENT | (gaps ? GCMF_FACES_FROM_NAN : 0u);
  const void *in1[2] = {in, nullptr};
  void *out1[2] = {out, nullptr};
  CallView cv = own_view(pl);
  cv.bank_rev = pl->bank_rev; cv.bank_fwd = pl->bank_fwd; cv.bank_stride = pl->bank_stride;
  GapFold fold;   // (this call's: the fields folded by its earlier launches)
  Tally t;
  const int64_t run_nf = gaps ? gap_launch_entries(pl) : nfield;
  if (nfield <= run_nf) {
    // All fields at once, the entries in consecutive launches: an entry keeps its place through entry0.  On gappy fields the view's level
    // axis has nlev = nfield levels and keeps the launch's entry0 = e0, so lev0 = e0 % nfield (ringc_params) and the kernel's level
    // (lev0 + y) % nlev = (e0 + y) % nfield: the field of entry e0 + y, also when e0 = k * MAX_LAUNCH_BATCH is no multiple of nfield;
    // k_land_fix takes the field from ent0 = entry0 itself.  Every such launch finds its work layout at another place (its batch differs
    // from the previous one's or the fields are folded already), so the fold is repeated only where it must be.
    // (p: the schedule reads the polynomial's degree only -- the launches and k_land_fix take the coefficients from the tables)
    cv.bank_n = nbank;
    cv.bank_nfield = nfield;
    rc = run_launches(pl, cv, gaps ? &fold : nullptr, p, n_steps, c, in1, 0, out1, cell * 8, nent, MAX_LAUNCH_BATCH, rflags, stream, false, t);
    return rc ? rc : t.leave(pl);
  }
  // Gappy fields beyond the scratch bound: the fields in runs that fit it; per run and polynomial one bank of ONE polynomial -- the table's
  // row base, `in` and `out` moved here, on the host -- over the run's fields: the same kernels on the same operands, and the run is folded
  // once (the launches of a run have one work layout).
  for (int64_t f0 = 0; f0 < nfield; f0 += run_nf) {
    const int64_t nf = std::min<int64_t>(nfield - f0, run_nf);
    cv.bank_n = 1;
    cv.bank_nfield = nf;
    in1[0] = (const char *)in + (size_t)f0 * cell * 8;
    for (int j = 0; j < nbank; ++j) {
      cv.bank_rev = pl->bank_rev + (size_t)j * pl->bank_stride;
      cv.bank_fwd = pl->bank_fwd + (size_t)j * pl->bank_stride;
      out1[0] = (char *)out + ((size_t)j * nfield + f0) * cell * 8;
      if ((rc = run_launches(pl, cv, &fold, p + (size_t)j * pl->bank_stride, n_steps, c, in1, 0, out1, cell * 8, nf, nf, rflags, stream, false, t))) return rc;
    }
  }
  return t.leave(pl);
}

int gcmf_apply_bank(gcmf_plan *pl, const double *p, int nbank, int n_steps, double c, const void *in, void *out, int64_t nfield,
                    uint32_t flags, void *stream) {
  return apply_bank("gcmf_apply_bank", false, pl, p, nbank, n_steps, c, in, out, nfield, flags, stream);
}

int gcmf_apply_bank_gaps(gcmf_plan *pl, const double *p, int nbank, int n_steps, double c, const void *in, void *out, int64_t nfield,
                         uint32_t flags, void *stream) {
  return apply_bank("gcmf_apply_bank_gaps", true, pl, p, nbank, n_steps, c, in, out, nfield, flags, stream);
}

int gcmf_laplacian(gcmf_plan *pl, const void *const *in, void *const *out, int64_t nbatch, uint32_t flags,
                   void *stream) {
  return run_whole(pl, nullptr, 0, 0.0, in, out, nbatch, flags, stream, true);
}

}  // extern "C"
