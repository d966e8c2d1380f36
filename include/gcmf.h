/*
 * gcmf.h -- C ABI of libgcmf, the MI355X (gfx950) implementation of the gcm-filters hot path.
 *
 * Drop-in boundary.  The reference (pure Python) has no FFI; the operator interface this library
 * replaces is the pair of closures created per Filter and called by xarray.apply_ufunc with raw
 * arrays whose last two axes are (y, x):
 *
 *     filter_func(field, *grid_args)            -> ndarray      gcm_filters/filter.py:177-212
 *     filter_func_vec(u, v, *grid_args)         -> (nd, nd)     gcm_filters/filter.py:242-289
 *
 * and the kernel plug-in protocol they drive                      gcm_filters/kernels.py:43-104
 *
 *     Laplacian(**grid_vars)   validation + precompute            -> gcmf_plan_create
 *     .prepare / .__call__ / .finalize                            -> gcmf_laplacian (one application)
 *     the n_steps recurrence around them                          -> gcmf_apply (whole polynomial)
 *
 * Everything is plain pointers and sizes; no torch / numpy types.  All entry points are thread-safe
 * with respect to *different* plans; calls on one plan are serialised by a per-plan mutex.
 *
 * Array conventions: C order, (nbatch, ny, nx) with x fastest.  Grid planes are 2-D (ny, nx) and
 * shared by every batch entry -- except on a STACKED plan (gcmf_plan_create_levels), whose grid planes
 * have a level axis and whose batch entry b is filtered with level b % nlev.  "Rows" are indices along
 * y (the slow, sharded axis).
 */
#ifndef GCMF_H
#define GCMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCMF_VERSION 1

/* ---- status codes -------------------------------------------------------------------------- */
typedef enum gcmf_status {
  GCMF_OK = 0,
  GCMF_ERR_INVALID_ARG = 1, /* bad pointer / size / enum / plane count                        */
  GCMF_ERR_HIP = 2,         /* a HIP runtime call failed; text in gcmf_last_error()           */
  GCMF_ERR_NO_DEVICE = 3,   /* no gfx950 device visible                                       */
  GCMF_ERR_UNSUPPORTED = 4,
  GCMF_ERR_P2P_TIMEOUT = 5, /* a peer-to-peer halo exchange of this rank failed (a neighbour never posted, or aborted): results NaN */
  /* Validation failures of the reference's Laplacian constructors.  The Python layer turns
   * them into the reference's exception type and message.                                   */
  GCMF_ERR_KAPPA_W_GT1 = 16,    /* ValueError  kernels.py:262-266                             */
  GCMF_ERR_KAPPA_S_GT1 = 17,    /* ValueError  kernels.py:268-272                             */
  GCMF_ERR_KAPPA_NONE_ONE = 18, /* ValueError  kernels.py:274-281                             */
  GCMF_ERR_WET_SOUTH_ROW = 19,  /* AssertionError kernels.py:458-459, 521-522                 */
  GCMF_ERR_DXN_FOLD = 20,       /* AssertionError kernels.py:551-554                          */
  GCMF_ERR_DYN_FOLD = 21        /* AssertionError kernels.py:559-562                          */
} gcmf_status;

/* ---- enums --------------------------------------------------------------------------------- */
/* Values equal the reference's GridType enum values (gcm_filters/kernels.py:13-28). */
typedef enum gcmf_grid_type {
  GCMF_REGULAR = 1,
  GCMF_REGULAR_AREA_WEIGHTED = 2,
  GCMF_REGULAR_WITH_LAND = 3,
  GCMF_REGULAR_WITH_LAND_AREA_WEIGHTED = 4,
  GCMF_IRREGULAR_WITH_LAND = 5,
  GCMF_MOM5U = 6,
  GCMF_MOM5T = 7,
  GCMF_TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED = 8,
  GCMF_TRIPOLAR_POP_WITH_LAND = 9,
  GCMF_VECTOR_C_GRID = 10,
  GCMF_VECTOR_B_GRID = 11
} gcmf_grid_type;

typedef enum gcmf_dtype { GCMF_F32 = 0, GCMF_F64 = 1 } gcmf_dtype;

/* gcmf_apply / gcmf_laplacian flags */
#define GCMF_DEVICE_PTRS 0x1u /* in/out are device pointers on the plan's device (else host)  */
#define GCMF_OUT_F32 0x2u     /* f32 plan only: write f32 output (default: f64, as NumPy >= 2 */
                              /* promotes p[k]*T)                       */
#define GCMF_FORWARD_RECURRENCE 0x4u /* gcmf_apply: sum the polynomial by the reference's forward     */
                              /* recurrence with its accumulation scheme (filter.py:192-206: f64 running sum   */
                              /* also for f32 state) even where the library would evaluate it backwards        */
                              /* (Clenshaw: f64 flux-form plans, C-grid plans)                                  */
#define GCMF_NO_RESIDENT 0x8u /* gcmf_apply / gcmf_slab_apply_backward: never use the on-chip (resident) kernel,   */
                              /* csrc/gcmf_resident.hip -- the strip-marching launches of 5..8 levels instead (same bits) */
#define GCMF_BACKWARD_F32 0x10u /* gcmf_apply, f32 scalar and B-grid plans: evaluate backwards (Clenshaw, all f32) like the f64 */
                              /* plans.  Faster (1.1-1.5 x) and 2-45 x further from f64 arithmetic than the reference's own f32  */
                              /* path (filter.py:192-206: f32 T_k, f64 running sum), which is the default for these plans.       */
#define GCMF_MASK_FROM_NAN 0x20u /* gcmf_apply, whole-grid plans of REGULAR_WITH_LAND, REGULAR_WITH_LAND_AREA_WEIGHTED and                */
                              /* TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED (host or device pointers, any nbatch): batch entry b is          */
                              /* filtered with its OWN wet mask m_b = wet_mask * [in_b is not NaN], i.e. the result equals the            */
                              /* reference's filter_func with wet_mask replaced by m_b -- a NaN is a gap (land, no flux) instead of       */
                              /* the value 0 the stencil reads through nan_to_num.  The output is NaN exactly where the input is; a       */
                              /* static land cell with a finite value keeps sum_k p_k (-1)^k f; +-inf is data, not a gap; an entry        */
                              /* without NaN gives the bits of an unflagged call.  The per-entry mask bytes are derived on the device      */
                              /* into the plan's work buffer (1 byte per cell and entry); the plan's own mask is never modified, so        */
                              /* flagged and unflagged calls may alternate.  Runs the strip-marching launches (never the on-chip           */
                              /* kernel).  Other plans, gcmf_laplacian, the gcmf_cheb_* building blocks and the slab drivers return        */
                              /* GCMF_ERR_UNSUPPORTED for it.  The call's masks are the call's alone: the plan's queries (gcmf_has_land,  */
                              /* gcmf_clenshaw_cut[_batch], gcmf_bank_cut, gcmf_resident_supported) answer for the plan itself at any     */
                              /* time, from any thread, also while a flagged call runs on it.                                             */
#define GCMF_FACES_FROM_NAN 0x40u /* gcmf_apply, whole-grid f64 ORDINARY (not stacked) plans of IRREGULAR_WITH_LAND, MOM5U and MOM5T (host or     */
                              /* device pointers, any nbatch): the same contract as GCMF_MASK_FROM_NAN for the flux-form kinds -- batch    */
                              /* entry b is filtered with wet_mask * [in_b is not NaN]; the output is NaN exactly where the input is;      */
                              /* +-inf is data; an entry without NaN gives the values of an unflagged call.  The entry's face coefficients */
                              /* and land bytes are folded on the device from the plan's own planes (csrc/gcmf_gap_fold.hpp: cE, cN times  */
                              /* a 0 / 1 factor per face -- bit for bit the planes a plan built from wet_mask * [not NaN] holds) into the   */
                              /* plan's work buffer, 25 bytes per cell and entry (cE, cN, a copy of 1 / area, one land byte); a batch is    */
                              /* cut into consecutive launches so that this scratch stays at or under option "gap_scratch_mb" (default     */
                              /* 4096; at least one entry per launch).  The launches are those of a stacked plan (gcmf_plan_create_levels) */
                              /* whose levels are the entries: the backward evaluation's plain strips and k_land_fix, never the on-chip    */
                              /* kernel, the zipped strips or the wet-row tables; the result has the bits of such a plan built from the    */
                              /* explicit masks.  The plan's own planes are never written: flagged and unflagged calls may alternate.      */
                              /* GCMF_ERR_UNSUPPORTED, with a message that names the flag and the three grid types, for: any other grid     */
                              /* type, f32 plans, row slabs, stacked plans, gcmf_laplacian, the gcmf_cheb_* and gcmf_slab_* building blocks */
                              /* and gcmf_land_fix, the flag combined with GCMF_FORWARD_RECURRENCE or GCMF_MASK_FROM_NAN, and a polynomial  */
                              /* or grid for which the stacked strips offer no backward cut (fewer than five steps, nx not a multiple of 4, */
                              /* GCMF_CLENSHAW=0 ...).  The plan's queries answer for the plan itself at any time, as above.                */

/* Chebyshev step modes for gcmf_cheb_step */
#define GCMF_STEP_FIRST 0x1u /* T1 = A(T0);            fbar  = p0*T0 + p1*T1                  */
#define GCMF_STEP_LAST 0x2u  /* fbar result is finalised (divided by area) into fbar_out      */
#define GCMF_STEP_LAND_FIXED 0x8u /* gcmf_cheb_multi with GCMF_STEP_FIRST: the caller will overwrite the result of the cells
                                    gcmf_zero_land zeroes with gcmf_land_fix (or there are none), so the launch may take them as
                                    zero while it loads the field; the states it writes then satisfy GCMF_STEP_LAND_ZERO */
#define GCMF_STEP_CLENSHAW 0x10u /* gcmf_cheb_multi: S levels of the BACKWARD evaluation of the polynomial (see gcmf_clenshaw_cut) */
#define GCMF_STEP_LAND_ZERO 0x4u /* gcmf_cheb_multi[_vec]: the caller guarantees that the cells gcmf_zero_land zeroes are
                                    zero in both input states (lets the land-mask kernels drop their per-neighbour tests) */

typedef struct gcmf_plan gcmf_plan;

/* ---- plan ---------------------------------------------------------------------------------- */
typedef struct gcmf_plan_desc {
  int32_t grid_type;  /* gcmf_grid_type                                                        */
  int32_t dtype;      /* gcmf_dtype of the grid planes, the recurrence state T_k and L(f)      */
  int64_t ny, nx;     /* GLOBAL grid shape                                                     */
  int64_t row_begin;  /* rows [row_begin, row_end) of the global grid are owned by this plan   */
  int64_t row_end;    /*   single GPU: 0, ny                                                   */
  int32_t halo;       /* ghost rows kept on each slab edge that has a neighbour (0: one GPU)   */
  int32_t device;     /* HIP device ordinal                                                    */
  int32_t planes_on_device; /* grid planes are device pointers on `device`                     */
  int32_t flags;      /* GCMF_PLAN_* bits, 0 by default                                        */
} gcmf_plan_desc;

/* A plan that covers the whole (periodic, non-tripolar) grid but keeps `halo` ghost rows per edge like a slab whose
 * two neighbours are itself: the one-rank form of the row-slab driver (tests of the exchange path on a single GPU). */
#define GCMF_PLAN_SELF_RING 0x1
/* IRREGULAR_WITH_LAND: do not fail with GCMF_ERR_KAPPA_NONE_ONE.  For grid variables with leading (level / time) dims the
 * reference applies that check to the whole array (kernels.py:274-281), not per (y, x) plane; the Python layer then does
 * it itself and builds one plan per plane with this flag. */
#define GCMF_PLAN_SKIP_KAPPA_ONE 0x2

/*
 * Build a plan = the reference's `Laplacian(**grid_vars)` (kernels.py __post_init__ methods):
 * validates the grid planes, folds masks / kappas / metric ratios into coefficient planes resident
 * in HBM, and sizes the recurrence state.  `planes` holds `nplanes` GLOBAL (ny, nx) arrays of
 * `desc->dtype`, in the order of `required_grid_args()` of the reference class (kernels.py:58-63):
 *
 *   REGULAR: -            REGULAR_AREA_WEIGHTED: area      REGULAR_WITH_LAND: wet_mask
 *   REGULAR_WITH_LAND_AREA_WEIGHTED / TRIPOLAR_REGULAR_...: area, wet_mask
 *   IRREGULAR_WITH_LAND: wet_mask,dxw,dyw,dxs,dys,area,kappa_w,kappa_s
 *   MOM5U: wet_mask,dxt,dyt,dxu,dyu,area_u      MOM5T: wet_mask,dxt,dyt,dxu,dyu,area_t
 *   TRIPOLAR_POP_WITH_LAND: wet_mask,dxe,dye,dxn,dyn,tarea
 *   VECTOR_C_GRID: wet_mask_t,wet_mask_q,dxT,dyT,dxCu,dyCu,dxCv,dyCv,dxBu,dyBu,area_u,area_v,
 *                  kappa_iso,kappa_aniso
 *   VECTOR_B_GRID: DXU,DYU,HUS,HUW,HTE,HTN,UAREA,TAREA
 *
 * Returns GCMF_OK or a status; validation failures return the GCMF_ERR_KAPPA_x / GCMF_ERR_WET_x /
 * GCMF_ERR_Dxx_FOLD codes and create no plan.
 */
int gcmf_plan_create(const gcmf_plan_desc *desc, const void *const *planes, int nplanes, gcmf_plan **out);
void gcmf_plan_destroy(gcmf_plan *plan);

/*
 * A STACKED plan: grid variables with a leading level axis -- wet_mask(z, y, x), kappa(z, y, x): what the reference gets when
 * xarray.apply_ufunc broadcasts the leading dims of field and grid variables against each other (filter.py:478-486) -- folded into ONE
 * plan whose coefficient planes and land bytes are (nlev, ny, nx).  planes[i] is a C-ordered (plane_levels[i], ny, nx) array,
 * plane_levels[i] = 1 (shared by all levels) or nlev; the planes' order is gcmf_plan_create's.  Validation is the reference's on the
 * whole arrays (kernels.py:262-281): a kappa > 1 on any level fails, GCMF_ERR_KAPPA_NONE_ONE only when NO level has a kappa of 1.  The
 * plan has land (gcmf_has_land) when any level has.
 *   Scope: IRREGULAR_WITH_LAND, MOM5U, MOM5T; dtype f64; the whole grid (row_begin = 0, row_end = ny, no GCMF_PLAN_SELF_RING) --
 *   anything else returns GCMF_ERR_UNSUPPORTED and names the limit: build one plan per level.
 *   gcmf_apply(plan, ..., nbatch, ...) filters batch entry b with the grid of level b % nlev: a (..., nlev, ny, nx) field in C order is
 *   one call.  nbatch must be a multiple of nlev (GCMF_ERR_INVALID_ARG); host and device pointers are both taken (the chunks of the
 *   pipelined host path keep their place in the batch).  The call runs the backward evaluation's plain strips (k_ringc, one workgroup
 *   column per entry; never the on-chip kernel, "single_launch", the packed walk, the zipped strips or the wet-row tables) and
 *   gcmf_clenshaw_cut_batch answers for those launches; the result has the bits of nlev ordinary plans run entry by entry.  Where the
 *   backward evaluation is not on offer (gcmf_clenshaw_cut_batch returns 0: fewer than five steps, nx not a multiple of 4 on a grid
 *   with land, GCMF_CLENSHAW=0 ...) gcmf_apply returns GCMF_ERR_UNSUPPORTED, as it does for GCMF_FORWARD_RECURRENCE and
 *   GCMF_MASK_FROM_NAN; so do gcmf_laplacian, the gcmf_cheb_* / gcmf_slab_* / gcmf_resident_* building blocks, gcmf_prepare,
 *   gcmf_zero_land and gcmf_land_fix.  gcmf_last_kernel names the ordinary kernel (the launches are an instantiation of their own of
 *   it); gcmf_last_kernel_geometry appends " levels=<nlev>".
 * gcmf_plan_levels: nlev of a stacked plan, 1 for an ordinary one (0 for NULL).
 */
extern int gcmf_plan_create_levels(const gcmf_plan_desc *desc, const void *const *planes, const int64_t *plane_levels, int nplanes, int64_t nlev,
                                   gcmf_plan **out);
extern int64_t gcmf_plan_levels(const gcmf_plan *plan);

/* Static facts (no device needed). */
int gcmf_grid_nplanes(int grid_type);        /* number of grid planes, -1 if unknown           */
int gcmf_grid_ncomp(int grid_type);          /* 1 scalar, 2 vector                             */
int gcmf_grid_is_dimensional(int grid_type); /* kernels.py `is_dimensional`                    */
int gcmf_grid_is_tripolar(int grid_type);

/* Local (slab) geometry of a plan: rows allocated incl. ghosts, index of the first owned row
 * inside the allocation, number of owned rows.  State arrays passed to gcmf_cheb_step have
 * `rows_alloc` rows per batch entry. */
int gcmf_plan_rows(const gcmf_plan *plan, int64_t *rows_alloc, int64_t *first_owned, int64_t *rows_owned);

/* ---- whole filter: the body of filter_func / filter_func_vec (filter.py:185-210, 250-289) ---- */
/*
 * out = finalize( sum_k p[k] T_k ),  T_0 = prepare(in), T_1 = A(T_0), T_k = 2 A(T_{k-1}) - T_{k-2},
 * A(x) = -x - c L(x).   `p` has n_steps+1 entries (host memory), n_steps >= 1.
 * `c` = 2/s_max (dimensional Laplacians) or 2/(s_max*dx_min^2)   (filter.py:170-173).
 * `in` / `out`: ncomp pointers (1 scalar, 2 vector) to (nbatch, ny, nx) arrays; `in` has the plan
 * dtype and is not modified; `out` is f64 unless the plan is f32 and GCMF_OUT_F32 is given.
 * Only valid on single-slab plans (row_begin = 0, row_end = ny).
 * THE PLANES OF A CALL (gcmf_apply, gcmf_laplacian, gcmf_apply_bank[_gaps]; host and device pointers alike):
 *   - Element alignment suffices for every plane: 8 bytes for f64, 4 for f32 (a view into a larger buffer, a slice of a stack).  The
 *     result does not depend on the alignment, bit for bit.  These launches fall back when a plane of the call is not on a 16-byte
 *     boundary (same arithmetic per cell, other access widths):
 *       k_scalar_step            its VEC = 1 form (last template argument)
 *       k_cgrid_stream           k_cgrid_step
 *       k_bgrid_stream           k_bgrid_step
 *       k_cgrid_ringf            k_cgrid_stream2
 *       k_cgrid_ring             k_cgrid_stream2c, and at most five levels per launch instead of six
 *       k_pre_isolated (the fold of GCMF_FACES_FROM_NAN and gcmf_apply_bank_gaps)   element loads of the field instead of 16-byte ones
 *     Every other kernel (the k_ring* / k_ringc* families, k_scalar_multi, k_flux_multi2, k_cgrid_stream2[c], k_bgrid_stream2[c],
 *     k_fold_band, k_land_fix, k_resident, the banks and the stacked plans) takes element-aligned planes as they are; the alignment
 *     these check is that of the plan's own coefficient planes, which the library allocates.
 *   - `out` must not overlap `in` or another `out` plane, as BYTE RANGES: nbatch * ny * nx elements of the plan dtype from in[k],
 *     of the output type from out[q] (GCMF_ERR_INVALID_ARG names the two planes; nothing is written).  Later launches and k_land_fix
 *     re-read the input, so an `out` that begins a row or a batch entry into `in` is as wrong as out == in.  in[0] == in[1] is allowed.
 *   - Nothing outside these byte ranges is read into a result or written: not a vector past the last row, not a row past the
 *     last strip.  `in` is never modified.  (tests/test_gpu_caller_planes.py)
 * `stream`: hipStream_t to run on.  With GCMF_DEVICE_PTRS the work is enqueued asynchronously on exactly
 * that stream (NULL = the HIP default stream), ordered with the caller's other work on it.  A stream handed in here must stay
 * alive until the NEXT gcmf_apply on this plan has returned (or the plan is destroyed): when that next call arrives on another
 * stream it orders itself behind this one with an event recorded on this stream.  With host
 * pointers the call stages through HBM and is synchronous (NULL = a private stream of the plan); a batch of host
 * fields is cut into chunks whose upload, filtering and download overlap, and the input range is page-locked
 * (hipHostRegister, best effort) while the call runs -- see DESIGN.md section 6 and the GCMF_HOST_* variables.
 * Scheduling is internal: up to 8 (vector kinds: 4) recurrence steps per pass over HBM; flux-form scalar grids keep
 * cells with four closed faces (land) out of the recurrence state and add their neighbour-free polynomial at the end.
 * The result is the reference's for every cell, land included.
 */
int gcmf_apply(gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in,
               void *const *out, int64_t nbatch, uint32_t flags, void *stream);

/*
 * THE ADJOINT: out = F^T in, F being the linear map gcmf_apply(plan, p, n_steps, c, ., flags) applies to finite fields -- what a loss
 * that contains the filter needs for its gradient, and what variational methods call directly.  (The reference has no counterpart.)
 * No transposed stencil runs: for every grid type but one the transpose of the whole filter is the filter itself between two diagonal
 * scalings,  F^T = D F D^-1:
 *   REGULAR, REGULAR_WITH_LAND                                   D = 1
 *   REGULAR_AREA_WEIGHTED, REGULAR_WITH_LAND_AREA_WEIGHTED,
 *   TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED                     D = area^2    (a symmetric stencil between prepare, * area, and finalize, / area)
 *   IRREGULAR_WITH_LAND, MOM5U, MOM5T, TRIPOLAR_POP_WITH_LAND    D = area      (L = diag(1 / area) M, M symmetric: one coefficient per face, and
 *                                                                               the tripole fold i <-> nx-1-i is symmetric too)
 *   VECTOR_C_GRID                                                D = (area_u, area_v)
 *   VECTOR_B_GRID                                                none: GCMF_ERR_UNSUPPORTED (its Laplacian has no diagonal symmetrizer;
 *                                                                it needs a transposed stencil kernel)
 * D is 1 on land cells and on cells cut off from the sea (F is diagonal there, so the identity holds for any finite non-zero D, and
 * junk metrics on land never reach the result).  D is taken from the planes the plan holds: ra = 1 / area on the flux kinds (in * ra,
 * then out / ra: the exact symmetrizer of the operator the kernels apply), the area plane of the area-weighted kinds; a VECTOR_C_GRID
 * plan keeps copies of area_u and area_v for it -- two planes more per C-grid plan.  area_u / area_v <= 0 (where the reference zeroes a
 * row of L but not its column) break the identity; the library does not look for them.
 * How it runs: one streaming pass (in / D into a scratch plane of the plan), gcmf_apply's own schedule on that plane -- whatever path
 * gcmf_apply takes with these flags: on-chip, strips, zipped, tables, forward or backward --, one streaming pass over `out` (times D, in
 * place).  Both passes are forms of k_prepare (csrc/gcmf_scalar.hip); they use 16-byte accesses where the planes of the call allow and
 * element accesses otherwise.  gcmf_last_kernel, gcmf_last_kernel_geometry and gcmf_plan_last_path answer for the inner schedule;
 * gcmf_last_timing covers the schedule and the two passes (one launch per pass and component).
 * Layout, dtypes, GCMF_DEVICE_PTRS, GCMF_OUT_F32 and the other flags, the stream contract and THE PLANES OF A CALL are gcmf_apply's; `out`
 * must not overlap `in` or `like` as byte ranges (GCMF_ERR_INVALID_ARG).  Host pointers are staged through HBM one launch at a time
 * (`in`, `like` and `out`), without gcmf_apply's chunk pipeline.
 * `like`: NULL, or ncomp pointers to the forward call's input planes (plan dtype, `in`'s layout).  Only their NaN pattern is read: where
 * `like` is NaN, `in` is taken as 0 and the result is 0 -- a NaN input cell has no derivative (the forward shows it to its neighbours as
 * the value 0, at every step of the recurrence, and returns NaN in the cell itself).  The pre-scale therefore hands the schedule a NaN
 * in such a cell, so that it is read as 0 at every step again -- F restricted to the finite cells is the polynomial of a principal
 * submatrix, and so is its transpose -- and the post-scale writes 0 there.  (REGULAR and REGULAR_AREA_WEIGHTED, whose stencil does not
 * mask a NaN: the cell is set to 0 once.)  With GCMF_MASK_FROM_NAN or GCMF_FACES_FROM_NAN `like` is required (NULL:
 * GCMF_ERR_INVALID_ARG): the per-entry masks / faces are derived from `like`, exactly the forward call's.
 * Stacked plans (gcmf_plan_create_levels): entry b uses the scaling planes of level b % nlev, like the filter itself.
 * Scratch: one plane of the plan dtype per component and entry of a launch, in the plan's work buffer (grow-only, freed by
 * gcmf_plan_destroy).  Option "adjoint_scratch_mb" (default 4096) bounds it: a longer batch is cut into consecutive launches of at least
 * one entry each; same bits.
 * GCMF_ERR_UNSUPPORTED, naming the function and the limit: VECTOR_B_GRID, row slabs, GCMF_PLAN_SELF_RING; and whatever gcmf_apply
 * refuses for these flags.
 */
extern int gcmf_apply_adjoint(gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in, const void *const *like,
                              void *const *out, int64_t nbatch, uint32_t flags, void *stream);

/*
 * FILTER, THEN COARSE-GRAIN: gcmf_apply followed by weighted block means of its result, so that less than a full-resolution plane comes
 * back -- over PCIe, with host pointers, only the coarse planes.  (The reference has no counterpart: its users coarsen the fine result.)
 * THE RULE (csrc/gcmf_coarsen.hpp, which also holds a plain C++ restatement, coarsen_plane).  For factors (fy, fx) that divide (ny, nx),
 * the fine result F of one batch entry and its weight plane w, block (J, I) = rows [J fy, (J + 1) fy) x columns [I fx, (I + 1) fx):
 *     count(j,i)  = w(j,i) > 0  &&  F(j,i) == F(j,i)
 *     wsum(J,I)   = sum of w over the counted cells of the block
 *     coarse(J,I) = sum of w * F over the counted cells / wsum(J,I);   NaN (and wsum = 0) when no cell counts
 * +-inf in F is data.  A NaN in F (a gap of a flagged call, a NaN the caller put on land), a weight <= 0 and a NaN weight are SKIPPED,
 * never multiplied (0 * inf is NaN, and the fine result on land is finite junk): weights that are 0 on land keep land out of the means.
 * Everything is summed in f64 in ONE fixed order -- each fine column of a block from south to north, then the columns from west to east
 * -- without atomics, so the bits of a coarse cell depend on neither nbatch, the entry's place in the batch, pointer alignment, host or
 * device pointers, "coarsen_scratch_mb" nor the run.
 *
 * gcmf_coarsen_weights: the weight planes of the plan's later gcmf_apply_coarsen calls -- `nlev` >= 1 f64 planes of ny x nx, one after
 * the other, copied into HBM that the plan owns (freed with the plan, replaced by a later call).  Host planes by default, device planes
 * with GCMF_DEVICE_PTRS (the only flag taken; the copy is complete on return).  Entry b of a call uses level b % nlev, for any nlev >= 1,
 * whatever the plan's own levels.  w == NULL drops the weights: every cell has weight 1, the state of a new plan.  Takes the plan's
 * mutex and waits for the device: set the weights once per weights array, not once per call.
 *
 * gcmf_apply_coarsen: `plan`, `p`, `n_steps`, `c`, `in`, `nbatch`, `stream` and the flags GCMF_DEVICE_PTRS, GCMF_FORWARD_RECURRENCE,
 * GCMF_BACKWARD_F32, GCMF_MASK_FROM_NAN, GCMF_FACES_FROM_NAN (and GCMF_NO_RESIDENT) are gcmf_apply's and are handed to it: the gaps of a
 * flagged call are NaN in F and drop out of the means by the rule.  out[0]: nbatch planes of (ny / fy) x (nx / fx) f64, whatever the
 * plan dtype.  `wsum`: NULL, or wsum[0] of the same shape receives the sums of the counted weights.  `in`, `out` and `wsum` are all host
 * pointers, or all device pointers with GCMF_DEVICE_PTRS (then everything is enqueued on `stream`, as for gcmf_apply; the planes may
 * start at any element boundary).
 * How it runs: the schedule gcmf_apply takes for the plan and the flags (on-chip or strips, k_land_fix included) writes the fine f64
 * planes into a work buffer of the plan's, and ONE streaming launch behind it on the same stream -- a further form of k_prepare
 * (csrc/gcmf_coarsen.hip), the name of the plane passes before and after a schedule -- reads the fine plane and the weight plane once,
 * 16 bytes per load where nx is even and the planes lie on 16-byte boundaries and element by element otherwise, and writes the coarse
 * plane (and wsum).  gcmf_last_kernel, gcmf_last_kernel_geometry and gcmf_plan_last_path answer for the schedule; gcmf_last_timing
 * counts the pass as one launch more (its time covers the schedule).
 * Scratch: the fine planes of a run of entries (grow-only, freed by gcmf_plan_destroy); option "coarsen_scratch_mb" (default 4096) bounds
 * them: a longer batch is cut into consecutive runs of at least one entry each (a stacked plan's: of whole sets of levels).  With host
 * pointers a run's input and coarse planes are staged beside them, one run at a time, without gcmf_apply's chunk pipeline; the call is
 * synchronous.  Stacked plans (gcmf_plan_create_levels): entry b takes level b % nlev of the plan and of the weights, each with its own nlev.
 * GCMF_ERR_INVALID_ARG, naming the argument, nothing written: fy < 1, fx < 1 or a factor that does not divide its length; a null `in`
 * or `out` (or wsum[0]); `out` or `wsum` overlapping `in` or each other as byte ranges; a stacked plan's nbatch that is no multiple of
 * its levels.  GCMF_ERR_UNSUPPORTED, naming the function and the limit: vector plans (ncomp == 2), row slabs, GCMF_PLAN_SELF_RING,
 * GCMF_OUT_F32 (the coarse planes are always f64); and whatever gcmf_apply refuses for these flags.  nbatch == 0: GCMF_OK.
 */
extern int gcmf_coarsen_weights(gcmf_plan *plan, const void *w, int64_t nlev, uint32_t flags);
extern int gcmf_apply_coarsen(gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in, void *const *out,
                              void *const *wsum, int64_t nbatch, int fy, int fx, uint32_t flags, void *stream);

/*
 * SUBFILTER COVARIANCES: tau(f, g) = F(f g) - F(f) F(g) of `npair` pairs of fields in one call (g = f: the subfilter variance) -- what
 * eddy kinetic energy, eddy fluxes and subgrid-forcing datasets are made of.  (The reference has no counterpart: its users compose it
 * from three applications.)
 * THE RULE (csrc/gcmf_cov.hpp, which also holds a plain C++ restatement, cov_pre_plane and cov_post_plane).  Per cell of a pair, with
 * `common` = the call carries GCMF_MASK_FROM_NAN or GCMF_FACES_FROM_NAN:
 *     n  = (f == f) && (g == g)                         +-inf is data
 *     f' = (common && !n) ? NaN : f,   g' likewise      common gaps: all three entries of a pair see isnan(f) | isnan(g)
 *     fg = f' * g'                                      one rounding
 *     out = F(fg) - F(f') * F(g')                       two roundings, no fused multiply-add; NaN in any operand gives NaN
 * Without `common`, f and g reach the filter bit for bit.  out equals, bit for bit, the composition of three gcmf_apply calls on f' g',
 * f' and g' and the two roundings above, whatever npair, a pair's place in the call, pointer alignment, host or device pointers and
 * "cov_scratch_mb": an entry has the same bits alone and inside a batch.
 *
 * gcmf_apply_cov: `plan`, `p`, `n_steps`, `c`, `stream` are gcmf_apply's.  `f`, `g`, `out`: npair planes of ny x nx f64 each, one after
 * the other -- all host pointers, or all device pointers with GCMF_DEVICE_PTRS (then everything is enqueued on `stream`, as for
 * gcmf_apply; the planes may start at any element boundary).  g == NULL or g == f: the variance, which filters two entries per pair,
 * not three.  Flags handed to gcmf_apply with its usual checks: GCMF_FORWARD_RECURRENCE, GCMF_MASK_FROM_NAN, GCMF_FACES_FROM_NAN,
 * GCMF_NO_RESIDENT; the two NaN flags also switch on the common gaps of the rule (the faces of a pair are folded three times, once per
 * entry).
 * How it runs: a pre pass writes the batch [f'_0 .. f'_{N-1} | g'_0 .. | fg_0 ..] of a run of N pairs into scratch of the plan's (with
 * host pointers f and g are uploaded straight into their slots, and the pass only applies the common gaps and writes fg), ONE gcmf_apply
 * filters the 3 N (variance: 2 N) entries, and a post pass reads the filtered planes and writes out (a device `out` directly).  Both
 * passes are further forms of k_prepare (csrc/gcmf_cov.hip): 16 bytes per load and store where every plane of the call lies on a
 * 16-byte boundary and ny * nx is even, element by element otherwise, with the same bits.  gcmf_last_kernel and gcmf_plan_last_path
 * answer for the schedule; gcmf_last_timing sums the runs, the two passes included (launches of the schedule + 2 per run).
 * Scratch: 6 planes per pair of a run (4 for a variance), grow-only, freed by gcmf_plan_destroy; option "cov_scratch_mb" (default 4096)
 * bounds it: a longer call is cut into consecutive runs of at least one pair each, and under GCMF_FACES_FROM_NAN a run's entries are
 * also kept at or under "gap_scratch_mb".  Stacked plans (gcmf_plan_create_levels): pair i runs on level i % nlev -- entry k N + i of a
 * run's batch is level i % nlev, because a run is whole sets of levels.  With host pointers the call is synchronous.
 * GCMF_ERR_INVALID_ARG, naming the argument, nothing written: a null `plan`, `p`, `f` or `out`; n_steps < 1; npair < 0; `out`
 * overlapping `f` or `g` as byte ranges (f and g may overlap each other: nothing writes them); a stacked plan's npair that is no
 * multiple of its levels.  GCMF_ERR_UNSUPPORTED, naming the cause: vector plans (ncomp == 2), f32 plans and GCMF_OUT_F32 (tau is a small
 * difference of large numbers: f32 intermediates are not offered), GCMF_PLAN_SELF_RING, row slabs; and whatever gcmf_apply refuses for
 * these flags.  npair == 0: GCMF_OK.
 */
extern int gcmf_apply_cov(gcmf_plan *plan, const double *p, int n_steps, double c, const void *f, const void *g,
                          void *out, int64_t npair, uint32_t flags, void *stream);

/*
 * A FILTER BANK: nbank polynomials of ONE degree applied to the same nfield fields in one call -- a sweep over filter scales, whose
 * polynomials share n_steps, c and the grid (s_max does not depend on the filter scale) and differ in p alone:
 *     out[j * nfield + i] = the polynomial p[j * (n_steps + 1) .. (j + 1) * (n_steps + 1)) applied to in[i]      (j < nbank, i < nfield)
 * `p`: nbank x (n_steps + 1) host doubles, row-major.  `in`: (nfield, ny, nx) f64, `out`: (nbank, nfield, ny, nx) f64, device pointers
 * (GCMF_DEVICE_PTRS is required), which must not overlap.  `stream` as for gcmf_apply with device pointers.
 *   Scope: ordinary (not stacked) f64 plans of IRREGULAR_WITH_LAND, MOM5U, MOM5T and TRIPOLAR_POP_WITH_LAND that cover the whole grid (no
 *   row slab, no GCMF_PLAN_SELF_RING), and a polynomial for which gcmf_bank_cut offers a cut -- anything else returns GCMF_ERR_UNSUPPORTED and names
 *   the function and the limit: host pointers, an f32 plan, another grid type, a stacked plan, GCMF_FORWARD_RECURRENCE,
 *   GCMF_MASK_FROM_NAN, GCMF_FACES_FROM_NAN, GCMF_OUT_F32, fewer than five steps, nx not a multiple of 4 on a grid with land,
 *   GCMF_CLENSHAW=0.  GCMF_ERR_INVALID_ARG: nbank < 1, n_steps < 1, a null pointer, `in` overlapping `out`.  nfield = 0: GCMF_OK.
 *   The call runs the backward evaluation's plain strips with the nbank * nfield entries as the batch (k_ringc, one workgroup column per
 *   entry, every entry reading the coefficients of its own polynomial from a table on the device and the input plane of its own field)
 *   and k_land_fix in the same form; never the on-chip kernel, "single_launch", the packed walk, the zipped strips or the wet-row tables.
 *   On a plan with the tripole seam (TRIPOLAR_POP_WITH_LAND) the strips stop S rows below the seam and k_fold_band, in the same per-entry
 *   form and reading the same table, advances those rows beside or after EVERY strip launch (option "band_seq_cells" decides which, as for
 *   gcmf_apply; gcmf_last_timing counts both launches); k_fold_band stops at eight levels, so the launches of such a plan run 5 .. 8.
 *   More than 32768 entries are cut into consecutive launches.  out[j, i] has the bits of
 *   gcmf_apply(plan, p_j, ..., in_i, nbatch = 1, GCMF_NO_RESIDENT) -- the backward result does not depend on how the levels or the
 *   strips are cut -- NaN, +-inf and land cells included.  The two coefficient tables live in the plan (grow-only, freed by
 *   gcmf_plan_destroy) and are uploaded only when `p` differs from the previous call's, after the stream has drained.
 *   gcmf_last_timing, gcmf_last_kernel and gcmf_plan_last_path (GCMF_PATH_STRIPS) work as after gcmf_apply; gcmf_last_kernel names the
 *   ordinary kernel (the launches are an instantiation of their own of it), gcmf_last_kernel_geometry appends " bank=<nbank>".
 * gcmf_bank_cut: the launch depths (5 .. 9 levels each; 5 .. 8 on a plan with the tripole seam) gcmf_apply_bank uses for a polynomial of
 * n_steps steps and nentries = nbank * nfield entries, written to depths[0 .. return value); 0 = a bank is not on offer for this plan /
 * polynomial.  The answer is the same inside and outside a bank call, and it is gcmf_apply_bank_gaps' cut too.
 *
 * gcmf_apply_bank_gaps: a filter bank on GAPPY fields -- gcmf_apply_bank with GCMF_FACES_FROM_NAN's meaning, same arguments and layout:
 *     out[j * nfield + i] has the bits of gcmf_apply(plan, p_j, ..., in_i, nbatch = 1, GCMF_FACES_FROM_NAN | GCMF_DEVICE_PTRS)
 * -- field i filtered with wet_mask * [in_i is not NaN] at every one of the nbank scales; NaN, +-inf and land cells included (a gap is
 * land in its own field's mask, so it comes out NaN).  The face coefficients and land bytes are folded ONCE per field (k_pre_isolated's
 * gap form, as for GCMF_FACES_FROM_NAN), not once per entry: 25 bytes per cell and FIELD in the plan's work buffer, bounded by option
 * "gap_scratch_mb"; when nfield fields need more, the fields are cut into runs that fit (at least one field each) and every polynomial is
 * served for each run -- same bits.  The launches are the bank's plain strips with the level axis of a stacked plan: entry e reads row
 * e / nfield of the coefficient table and the input plane, the folded planes and the land bytes of field e % nfield (k_ringc and
 * k_land_fix, instantiations of their own again).
 *   Scope: ordinary whole-grid f64 plans of IRREGULAR_WITH_LAND, MOM5U and MOM5T, device pointers (`flags` must hold GCMF_DEVICE_PTRS),
 *   `in` and `out` not overlapping, a polynomial for which gcmf_bank_cut offers a cut (which needs nx to be a multiple of 4).
 *   GCMF_ERR_UNSUPPORTED, naming the function and the limit: TRIPOLAR_POP_WITH_LAND or any other grid type, an f32 plan, a stacked plan,
 *   a row slab, GCMF_PLAN_SELF_RING, host pointers, GCMF_FORWARD_RECURRENCE, GCMF_MASK_FROM_NAN, GCMF_OUT_F32, no cut.
 *   GCMF_ERR_INVALID_ARG as for gcmf_apply_bank.  nfield = 0: GCMF_OK.  GCMF_FACES_FROM_NAN in `flags` is accepted and implied;
 *   gcmf_apply_bank itself keeps refusing both NaN flags.  gcmf_last_kernel names the ordinary kernel,
 *   gcmf_last_kernel_geometry appends " levels=<fields of the launch> bank=<polynomials of the launch>".
 */
extern int gcmf_apply_bank(gcmf_plan *plan, const double *p, int nbank, int n_steps, double c, const void *in, void *out, int64_t nfield,
                           uint32_t flags, void *stream);
extern int gcmf_apply_bank_gaps(gcmf_plan *plan, const double *p, int nbank, int n_steps, double c, const void *in, void *out, int64_t nfield,
                                uint32_t flags, void *stream);
extern int gcmf_bank_cut(const gcmf_plan *plan, int n_steps, int64_t nentries, int *depths, int max_depths);

/* One application of the Laplacian: `ALL_KERNELS[grid_type](**grid_vars)(field)` (kernels.py
 * __call__ methods; no prepare/finalize).  `out` has the plan dtype. */
int gcmf_laplacian(gcmf_plan *plan, const void *const *in, void *const *out, int64_t nbatch,
                   uint32_t flags, void *stream);

/* ---- building blocks for the multi-GPU (row-slab) driver; device pointers only --------------- */
/*
 * One Chebyshev step on rows [row_lo, row_hi) of the slab allocation (see gcmf_plan_rows):
 *   t1:      T_{k-1}  (stencil input; rows row_lo-1 .. row_hi must be valid or wrap/fold)
 *   t2:      T_{k-2}  (centre only; ignored with GCMF_STEP_FIRST)
 *   fbar_in: running sum (centre only; ignored with GCMF_STEP_FIRST)
 *   t0:      T_k out  (may alias t2; may be NULL with GCMF_STEP_LAST)
 *   fbar_out: running sum out (may alias fbar_in); with GCMF_STEP_LAST it receives finalize(fbar)
 * coef0 = p[k] (or p[0] with FIRST), coef1 = p[1] (FIRST only).
 * fbar arrays are f64 for f64 plans; for f32 plans f64 unless GCMF_OUT_F32.
 * Asynchronous on `stream` (NULL = the HIP default stream).
 */
int gcmf_cheb_step(gcmf_plan *plan, const void *const *t1, const void *const *t2,
                   const void *const *fbar_in, void *const *t0, void *const *fbar_out, double coef0,
                   double coef1, double c, uint32_t mode, uint32_t flags, int64_t nbatch,
                   int64_t row_lo, int64_t row_hi, void *stream);

/*
 * S recurrence steps in ONE pass over HBM (temporal blocking, scalar grid types; S in 2..8):
 *   u = T_{k-1}, v = T_{k-2} (ignored with GCMF_STEP_FIRST)  ->  uo = T_{k-1+S}, vo = T_{k-2+S}
 *   fbar_out = fbar_in + sum_t pk[t] T_{k+t}  (t = 0..S-1; with FIRST: p0*T_0 + pk[0]*T_1 + ...)
 * on rows [row_lo, row_hi) of the slab allocation; the inputs must be valid on [row_lo-S, row_hi+S) (clipped
 * at a wrapped / closed / folded physical boundary, which the kernel handles).  uo / vo must not alias u / v;
 * fbar_out may alias fbar_in.  prepare() is fused with FIRST, finalize() with LAST (uo/vo then unused).
 * Results are bit-identical to S calls of gcmf_cheb_step.  gcmf_multi_supported tells whether a plan/S
 * combination is available (vector grids, odd nx, very short grids are not).
 */
int gcmf_multi_supported(const gcmf_plan *plan, int S);
/*
 * Backward (Clenshaw) evaluation of the same polynomial  sum_k p[k] T_k(A) f  (reference filter.py:162-212):
 *   b_{n+1} = b_{n+2} = 0,  b_k = p[k] f + 2 A(b_{k+1}) - b_{k+2}  (k = n..1),  result = p[0] f + A(b_1) - b_2.
 * The state is two planes instead of three (no fbar); every launch re-reads the constant input f: one plane less per launch.
 * Same NaN / land semantics as the forward recurrence; results differ from it in the last bits (<= 3e-15 relative) and are
 * identical however the levels are cut.  gcmf_apply uses it by default for the f64 flux-form grid types without a tripole fold
 * and for VECTOR_C_GRID (f32 state: the whole recurrence then runs in f32, 2e-6 from the f64-accumulated forward result at
 * n = 44); env GCMF_CLENSHAW = 0 off / 1 those / 2 also the other f64 scalar types.  gcmf_cheb_multi_vec (vector slab callers)
 * runs the forward recurrence.
 * gcmf_clenshaw_cut_batch: the launch depths (each 5..9, summing to n_steps) gcmf_apply uses for this plan, n_steps and a batch of
 * nbatch fields -- return value = their number, 0 = it runs the forward recurrence.  Nine levels per launch only where a launch of
 * nine runs and that saves a launch: whole f64 flux-form grids of 64 rows or more (tripolar ones only while k_ringcz advances the
 * seam inside the launch -- nx >= 256 and a multiple of 4, at most 64 fields, a batch the launcher would not pack -- so the answer
 * depends on nbatch) and row slabs of such grids without a seam when option "slab_nines" is on.  gcmf_clenshaw_cut: the same for
 * nbatch = 1.  gcmf_cheb_multi and gcmf_slab_apply_backward refuse (GCMF_ERR_UNSUPPORTED) a depth that cannot run for their own
 * batch and rows, so a cut is to be taken for the batch it is run with.  A slab caller does the same with gcmf_cheb_multi and
 * GCMF_STEP_CLENSHAW:  level l = 1..n_steps computes b_{n-l};  launch with levels l0 .. l0+S-1:  u = b_{n-l0+1}, v = b_{n-l0+2}
 * (FIRST, l0 = 1: ignored, the launch forms b_n = p0 * f itself: pass p0 = p[n]),  fbar_in = f,  pk[t] = p[n - (l0 + t)],
 * uo = b_{n-l0-S+1}, vo = b_{n-l0-S+2};  LAST (l0 + S - 1 = n): fbar_out = the result (finalize() applied), uo / vo unused.
 * Isolated (land) cells are taken as zero throughout: run gcmf_land_fix on the result when gcmf_has_land(plan).
 */
int gcmf_clenshaw_cut(const gcmf_plan *plan, int n_steps, int *depths, int max_depths);
int gcmf_clenshaw_cut_batch(const gcmf_plan *plan, int n_steps, int64_t nbatch, int *depths, int max_depths);
int gcmf_cheb_multi(gcmf_plan *plan, const void *u, const void *v, void *uo, void *vo, const void *fbar_in,
                    void *fbar_out, const double *pk, int S, double p0, double c, uint32_t mode, uint32_t flags,
                    int64_t nbatch, int64_t row_lo, int64_t row_hi, void *stream);

/*
 * The same for every grid type, with per-component pointer arrays like gcmf_cheb_step (ncomp entries each).
 * Scalar plans forward to gcmf_cheb_multi.  VECTOR_C_GRID (reference kernels.py:591-699 inside the recurrence of
 * filter.py:225-283) advances S in 2..5 steps per pass (f64 plans: 2..4); levels are processed by lock-step
 * workgroups of 4 (a batch that is not a multiple of 4 is padded internally, nothing is stored for the padding).
 * VECTOR_B_GRID (kernels.py:702-840): the same, f32 batches up to S = 6.
 */
int gcmf_multi_supported_vec(const gcmf_plan *plan, int S, int64_t nbatch);
int gcmf_cheb_multi_vec(gcmf_plan *plan, const void *const *u, const void *const *v, void *const *uo,
                        void *const *vo, const void *const *fbar_in, void *const *fbar_out, const double *pk,
                        int S, double p0, double c, uint32_t mode, uint32_t flags, int64_t nbatch,
                        int64_t row_lo, int64_t row_hi, void *stream);

/*
 * Land kept out of the recurrence state (flux-form and land-mask scalar grid types; what gcmf_apply does internally,
 * for slab drivers).  A land cell / a cell whose four faces are closed has L = 0 at every step (the wet mask zeroes
 * it or its fluxes, kernels.py:163-187, 286-315, 538-585) and evolves on its own.  gcmf_has_land: 1 if the plan has such cells and the two calls
 * below are available.  gcmf_zero_land: zero them in two state arrays (slab layout, e.g. the outputs of the first
 * gcmf_cheb_multi_vec call) so that NaN on land stops feeding the NaN / inf bookkeeping of the blocked kernels.
 * gcmf_land_fix: write their neighbour-free polynomial (prepare / finalize included, same operations and order as the
 * stencil kernels) over `out`, computed from the original field `in` (slab layout); p = n_steps + 1 host doubles.
 */
int gcmf_has_land(const gcmf_plan *plan);
int gcmf_zero_land(gcmf_plan *plan, void *const *a, void *const *b, int64_t nbatch, void *stream);
int gcmf_land_fix(gcmf_plan *plan, const double *p, int n_steps, double c, const void *const *in,
                  void *const *out, int64_t nbatch, uint32_t flags, void *stream);

/* ---- halo exchange of the row-slab driver, issued from C++ (RCCL send / recv over xGMI on a side stream) --------- */
/*
 * The reference has no spatial decomposition (filter.py:478-486 parallelises over non-core dims only); SURVEY 8e.
 * gcmf_comm_unique_id: 128 bytes (ncclUniqueId) generated on one rank and handed to every rank by the caller's own
 * channel (torch.distributed / MPI broadcast).  gcmf_comm_create: collective over `world` processes, one GPU each.
 * gcmf_halo_start: after everything enqueued on `stream` so far, send the `halo` owned edge rows of every block of the
 * `nstate` state arrays ((nblocks, rows_alloc, nx), nblocks = ncomp * nbatch, gcmf_dtype `dtype`) to the `south` / `north`
 * peer ranks (-1: physical boundary, nothing is exchanged there) and receive this slab's ghost rows; returns at once,
 * work enqueued on `stream` afterwards overlaps with the transfer.  gcmf_halo_finish: `stream` waits for the
 * exchange.  Between the two calls the caller may update any row except the 2 x halo sent and the ghost rows.
 */
typedef struct gcmf_comm gcmf_comm;
int gcmf_comm_unique_id(void *id128);
int gcmf_comm_create(const void *id128, int world, int rank, int device, gcmf_comm **out);
void gcmf_comm_destroy(gcmf_comm *comm);
/* What RCCL itself reports about the communicator: ncclGetVersion, ncclCommCount, ncclCommUserRank (-1 where unavailable). */
int gcmf_comm_info(gcmf_comm *comm, int *version, int *nranks, int *rank);
int gcmf_halo_start(gcmf_comm *comm, void *const *states, int nstate, int64_t nblocks, int64_t rows_alloc, int64_t nx,
                    int64_t first_owned, int64_t rows_owned, int halo, int dtype, int south, int north, void *stream);
int gcmf_halo_finish(gcmf_comm *comm, void *stream);

/* T_0 = prepare(field) = field * area for the AREA_WEIGHTED grid types (kernels.py:100-101),
 * a copy otherwise; rows [row_lo,row_hi) of the slab allocation. */
int gcmf_prepare(gcmf_plan *plan, const void *const *in, void *const *out, int64_t nbatch,
                 int64_t row_lo, int64_t row_hi, void *stream);

/* ---- timing of the last gcmf_apply (hipEvents on the stream the kernels ran on) -------------- */
/* ms_total: whole recurrence; n_launches: kernel launches it took. */
int gcmf_last_timing(const gcmf_plan *plan, float *ms_total, int *n_launches);
/* Enable/disable event timing inside gcmf_apply (adds two hipEventRecord per call).  enabled = 2: additionally one event
 * pair around every temporally blocked launch (the dominant kernel), read back with gcmf_last_kernel_timing: sum, count,
 * shortest and longest of the launches of the dominant kernel (gcmf_last_kernel) in the last gcmf_apply (device-resident calls, up to 32768 batch entries). */
int gcmf_set_timing(gcmf_plan *plan, int enabled);
int gcmf_last_kernel_timing(const gcmf_plan *plan, float *ms_sum, int *n_launches, float *ms_min, float *ms_max);
/* Name (as rocprofv3 prints it, without "void " and the argument list) of the recurrence kernel that advanced the most
 * steps per launch since this was last called; "" if none ran.  Reading resets it.  Instrumentation only: bench.py
 * refuses to quote profiled HBM traffic for a kernel other than the one that ran. */
int gcmf_last_kernel(gcmf_plan *plan, char *buf, int n);
/* Launch geometry of that kernel ("H=<rows per strip> nstrips=.. nwx=<column windows> xcd=<0|1> grid=XxY rows=..";
 * "" for kernels that are not strip-marched).  Survives gcmf_last_kernel's reset.  A PMC traffic record only
 * describes the kernel at the geometry it was profiled with.  A k_ringcz launch whose strips were cut from the wet rows of each
 * window (option "wet_rows") appends " units=<pairs of strips>" (0: a grid that is all land, nothing was launched); H is then the
 * tallest strip and nstrips twice the largest number of pairs of a window.  The tight cut (values 3 and 4 of the option) appends
 * " xoff=<columns>" after that: the column at which its window grid starts; " nt=1" after that: the launch streamed its state planes
 * (option "stream_state"). */
int gcmf_last_kernel_geometry(gcmf_plan *plan, char *buf, int n);
/* Wave strips of the register-ring kernels (k_ring) that met a NaN / inf since this was last called and were redone by the
 * general kernel (results are the same; each costs about two strip times).  Synchronises the device; reading resets.  A large
 * count on ocean data means non-finite values in wet cells (NaN on land is masked on load and costs nothing). */
int gcmf_ring_fallbacks(gcmf_plan *plan, int64_t *count);

/* ---- peer-to-peer halo exchange for the ranks of one node (csrc/gcmf_p2p.hip; SURVEY 8e "latency escape hatch": direct peer stores
 * into the neighbour's memory + flags instead of an RCCL group).  Every rank owns a mailbox block its two neighbours map through
 * HIP IPC: gcmf_p2p_create (mailbox_bytes >= the largest message: nstate * nblocks * halo * nx * sizeof(T)), gcmf_p2p_export (64-byte
 * hipIpcMemHandle_t, handed to the neighbours by the caller's own channel), gcmf_p2p_connect (south / north handles, NULL = a physical
 * boundary; *_is_self: that neighbour is this very process), then per exchange gcmf_p2p_start (after the launches that produced the edge
 * rows) ... interior launches ... gcmf_p2p_finish (before the next launch that reads the ghost rows), both enqueued on the caller's
 * compute stream: two small kernels, no events, no host round trip.  Arguments of gcmf_p2p_start as gcmf_halo_start.
 * The block is fine-grained device memory (coherent between agents while kernels run); remote memory is only written.
 * FAILURE IS LOUD: waits inside the kernels are bounded (GCMF_P2P_TIMEOUT_MS, default 30000; gcmf_p2p_set_timeout_ms).  A wait that runs
 * out marks this rank failed (sticky), raises `abort` in both neighbours (the failure travels round the ring at once), delivers NaN
 * ghost rows instead of stale ones, and gcmf_p2p_guard -- enqueued by the slab drivers after the last launch of an application --
 * turns the application's result into NaN.  gcmf_p2p_status reads the failure word from mapped host memory (0 ok, 1 timed out, 2
 * aborted by a neighbour; no device call); gcmf_p2p_start and gcmf_slab_apply_backward return GCMF_ERR_P2P_TIMEOUT on a failed
 * exchange.  gcmf_p2p_seq: exchanges started so far (equal on every rank of a healthy run).  gcmf_p2p_debug_skip_post: test hook,
 * drops the post of exchange number `seq` on this rank. */
typedef struct gcmf_p2p gcmf_p2p;
int gcmf_p2p_create(int device, int64_t mailbox_bytes, gcmf_p2p **out);
int gcmf_p2p_export(gcmf_p2p *p, void *handle64);
int gcmf_p2p_connect(gcmf_p2p *p, const void *south_handle64, const void *north_handle64, int south_is_self, int north_is_self);
int gcmf_p2p_start(gcmf_p2p *p, void *const *states, int nstate, int64_t nblocks, int64_t rows_alloc, int64_t nx, int64_t first_owned,
                   int64_t rows_owned, int halo, int dtype, void *stream);
int gcmf_p2p_finish(gcmf_p2p *p, void *stream);
int gcmf_p2p_guard(gcmf_p2p *p, void *out, int64_t bytes, void *stream);
int gcmf_p2p_status(gcmf_p2p *p, int *failed);
int gcmf_p2p_seq(gcmf_p2p *p, int64_t *seq);
int gcmf_p2p_set_timeout_ms(gcmf_p2p *p, int64_t ms);
int gcmf_p2p_debug_skip_post(gcmf_p2p *p, int seq);
void gcmf_p2p_destroy(gcmf_p2p *p);

/* ---- one whole filter application on this rank's slab, backward (Clenshaw) evaluation, scalar kinds, in ONE call: launches,
 * ghost-zone bookkeeping, the edge / interior split that overlaps the exchange, and the halo exchanges themselves (through `comm` --
 * RCCL -- or `p2p` -- mailboxes; both NULL for a slab without neighbours), all enqueued on `stream`.  X: this rank's input with its own rows
 * filled in, pool: four state planes, out: the result (f64; the state dtype with GCMF_OUT_F32), all (nbatch, rows_alloc, nx) device
 * arrays; cut / ncut: gcmf_clenshaw_cut_batch for this nbatch; halo: ghost rows per side (>= the deepest launch); south / north: peer ranks or -1; overlap != 0:
 * post the exchange between the edge strips and the interior of the launch that uses up the ghost zone (slabs of >= 4 halo rows).
 * What gcm_filters_amd/distributed.py otherwise does from Python, ~15 us of host time per launch and 13-33 us per exchange. */
int gcmf_slab_apply_backward(gcmf_plan *plan, gcmf_comm *comm, gcmf_p2p *p2p, int south, int north, const double *p, int n_steps, double c,
                             const int *cut, int ncut, void *X, void *const *pool, void *out, int64_t nbatch, int halo, int overlap,
                             uint32_t flags, void *stream);

/* The same for the VECTOR kinds (VECTOR_C_GRID, VECTOR_B_GRID; reference filter.py:217-291 filter_func_vec on a row slab): X / out = the two
 * components, pool = four state plane pairs (pool[2 q + component]); the levels are cut as gcmf_apply cuts them for this plan (at most four
 * per launch), the ghost zone (halo >= 4 rows) is refreshed -- both states of both components in one message per neighbour -- when the next
 * launch needs more rows than are left.  gcmf_slab_backward_vec_supported: does this plan / batch have a backward vector kernel (every
 * rank of a run must get the same answer; halo 0 = do not check the ghost depth)? */
int gcmf_slab_backward_vec_supported(const gcmf_plan *plan, int64_t nbatch, int halo);
int gcmf_slab_apply_backward_vec(gcmf_plan *plan, gcmf_comm *comm, gcmf_p2p *p2p, int south, int north, const double *p, int n_steps, double c,
                                 void *const *X, void *const *pool, void *const *out, int64_t nbatch, int halo, uint32_t flags, void *stream);

/* ---- the on-chip (resident) kernel, csrc/gcmf_resident.hip: the north star's "one persistent field per GPU with the whole n_steps
 * polynomial fused into a single launch, 2-D blocking with LDS-staged halo tiles", for fields that fit the register files + LDS of the
 * chip (the 300-row slab of an 8-way cut of 2400 x 3600 with its ghost rows; 512 x 512; up to ~1.5 M f64 cells).  One workgroup per CU owns
 * a 2-D tile for up to 64 levels of the backward (Clenshaw) evaluation of filter.py:162-212's polynomial; tiles trade their 4-cell edge
 * bands through the memory-side cache with per-tile epoch flags every 4 levels.  Bit-identical to the strip-marching launches.
 * gcmf_apply uses it by itself for whole grids up to ~420 k cells (one launch for the whole polynomial: IRREGULAR 512 x 512, n 63: 88 us
 * against 179 us); on the row slabs of a multi-GPU run it measured slower (a tile exchange costs ~9.5 us against ~1 us per level,
 * DESIGN.md 3.6), so gcmf_slab_apply_backward uses it only with env GCMF_RESIDENT=1 (=0 forbids it everywhere; GCMF_NO_RESIDENT per
 * call); these two entries are the building block and always available.
 * gcmf_resident_supported: can L levels with output rows [row_lo, row_hi) run in one resident launch?  gcmf_resident_levels: run them --
 * (u, v) = (b_{k+1}, b_{k+2}) (GCMF_STEP_FIRST: unused), f = the constant input, pk[l] = coefficient of level l + 1, p0 = p_n;
 * GCMF_STEP_LAST: `out` gets the result, otherwise (uo, vo) the new states.  Bit-identical to the same levels through gcmf_cheb_multi
 * with GCMF_STEP_CLENSHAW.  Two PROCESSES must not run resident launches on one GPU at the same time (see the file's header). */
int gcmf_resident_supported(const gcmf_plan *plan, int64_t row_lo, int64_t row_hi, int L);
int gcmf_resident_levels(gcmf_plan *plan, const void *u, const void *v, void *uo, void *vo, const void *f, void *out, const double *pk,
                         int L, double p0, double c, uint32_t mode, int64_t row_lo, int64_t row_hi, void *stream);

/* Which of the two bit-identical paths the last gcmf_apply of a plan took, and how often each was taken since the plan was made
 * ("make the path taken observable").  The reference has no counterpart (one numpy path, filter.py:177-212).
 *   GCMF_PATH_RESIDENT            the whole polynomial in on-chip launches (k_resident)
 *   GCMF_PATH_STRIPS              the strip-marching launches (BASELINE-size grids, batches, f32, vector kinds, GCMF_RESIDENT=0 ...)
 *   GCMF_PATH_STRIPS_LOCK_BUSY    the grid qualified for the on-chip kernel, but ANOTHER PROCESS holds this GPU's resident lock
 *   GCMF_PATH_STRIPS_DISABLED     the grid qualified, but an on-chip launch of this process timed out earlier (see gcmf_resident_status)
 * counts (optional): int64[5], indexed by the path codes. */
#define GCMF_PATH_NONE 0
#define GCMF_PATH_RESIDENT 1
#define GCMF_PATH_STRIPS 2
#define GCMF_PATH_STRIPS_LOCK_BUSY 3
#define GCMF_PATH_STRIPS_DISABLED 4
int gcmf_plan_last_path(const gcmf_plan *plan, int *path, int64_t *counts);
/* This process's standing with the on-chip kernel on `device`: GCMF_RESIDENT_OK (it holds the per-GPU lock file -- given back
 * GCMF_RESIDENT_LOCK_IDLE_S seconds, default 5, after its last on-chip launch finished; 0 = kept until exit), GCMF_RESIDENT_LOCK_BUSY
 * (another process holds it), GCMF_RESIDENT_DISABLED (an on-chip launch of this process timed out: NaN result, strip-marching launches
 * from then on), GCMF_RESIDENT_OFF (never asked / GCMF_RESIDENT=0 / a CU mask).  failures: time-outs seen so far.  A time-out is
 * returned as GCMF_ERR_HIP ONCE, by the next gcmf_apply of the plan that issued the launch (the same call on the synchronising host
 * path); calls on other plans are never failed for it. */
#define GCMF_RESIDENT_OK 0
#define GCMF_RESIDENT_LOCK_BUSY 1
#define GCMF_RESIDENT_DISABLED 2
#define GCMF_RESIDENT_OFF 3
int gcmf_resident_status(int device, int *state, uint64_t *failures);


/* Tunables: rows marched per wave of the single-step kernel (0 keeps the default); XCD-aware tile order
 * (bit 0: 1 on, 0 off; bits 1-2: neighbouring strips of the backward flux kernels march in opposite directions -- 1 off, 2 on, 0 keep;
 * <0 keeps both); temporal blocking: low byte = recurrence steps fused per HBM pass (1 = off,
 * 2..8), bits 8-23 = rows per wave strip (0 = auto), bits 24-27 = operand rows in flight of the general kernels, bits 28-29 =
 * backward evaluation (1 off, 2 flux kinds, 3 all scalar kinds; 0 keep); 0 keeps the default. */
int gcmf_set_tuning(gcmf_plan *plan, int rows_per_wave, int xcd_remap, int multi);
/* Named per-plan switches (A/B testing, the parity tests): "cgrid_ring" 1 / 0 (the static-ring C-grid kernel of batched f32 levels,
 * gcmf_cgrid_ring.hip; 0 = k_cgrid_stream2c everywhere), "cgrid_ring_smax" 4 / 5 / 6 (levels per launch), "cgrid_ring_ncarry" 0 / 1 (1 = round 5's form: only
 * the last level keeps its previous row's scaled copies in registers; same bits), "cgrid_ring_hmax" (tallest strip, 0 = 96 rows), "ringc9" 1 / 0 (nine levels per k_ringc launch on whole f64 flux grids), "ringc_zip" 1 / 0 (k_ringcz: strips of f64 flux plans without a tripole
 * seam marched in pairs away from a shared seam wherever that marches fewer rows; same bits; 2 / 3 = always its early-exit / whole-period form), "ringc_smax" 0 / 5..9
 * (backward scalar launches of at most this many levels; 0 = the default cut), "zip_fold" 1 / 0 (tripolar f64 flux plans evaluated backwards: k_ringcz advances the seam's rows itself -- strips that start
 * at the seam, zipped with the strips of their mirror windows -- instead of k_fold_band beside / after the launch; same bits), "slab_nines" 0 / 1 (row-slab plans of f64 flux grids without a tripole seam: gcmf_clenshaw_cut offers nine levels per launch where that saves one; the
 * ranks of a run must set it alike and own a ghost zone of at least nine rows -- SlabFilter decides it collectively), "band_seq_cells" N (tripolar plans: a blocked launch over at most N cells runs the seam's
 * k_fold_band after itself -- 1024 threads per tile -- instead of beside itself on a side stream; default 3000000, 0 = never; same bits), "pack_batch" 1 / 0 (batches on short
 * grids: the fields as one column of rows per window, k_ringcp; same bits), "single_launch" 0 / 1 (whole f64 flux-form grids of ANY size
 * whose n_steps is a multiple of 9 or 8: the whole polynomial in ONE persistent launch, csrc/gcmf_ringc_one.hip -- the passes over HBM
 * separated by grid-wide barriers instead of launch boundaries; same bits, measured 7 % slower at 2400 x 3600, hence opt-in; also env
 * GCMF_SINGLE_LAUNCH=1), "clenshaw_f32" 0 / 1 (GCMF_BACKWARD_F32
 * for every call of this plan, the slab drivers and gcmf_clenshaw_cut included), "ring_flux_f32" 1 / 0 (the forward ring kernel of the f32
 * flux kinds, gcmf_ring_flux_f32.hip; 0 = k_flux_multi2, same bits), "wet_rows" 3 / 0 / 1 / 2 / 4 (whole f64 flux grids with land, a lone field:
 * k_ringcz's strips are cut from the rows of each window that hold anything wet, so that no wave marches a tile that is all land;
 * 3 (the default) = the TIGHT cut -- rows that a window's OWNED columns need, not widened, the window grid shifted in x to where the
 * launch marches fewest rows (csrc/gcmf_wet_cut.hpp) -- where that marches at least 10 % fewer rows than the even cut, 4 = the tight
 * cut whenever eligible; 1 and 2 = the same two policies with the cut of round 7 (rows needed by a window's 128-column footprint,
 * widened by S + 1 rows, windows from column 0); 0 = never; same values -- the sign of an
 * exact zero next to land may differ; the FIRST eligible gcmf_apply of a plan builds the tables: it copies the plan's land bytes
 * (one byte per cell) to the host, synchronises the caller's stream and uploads the tables with a blocking copy -- once per plan and
 * launch depth, but not asynchronous and not legal inside a stream capture: capture after one warm-up call, or set 0),
 * "stream_state" 1 / 0 / 2 (nine-level launches from a wet-row table: the state planes, each byte of which is written by one launch and
 * read by the next only, are loaded and stored with the non-temporal policy, so that the constant planes every launch re-reads stay in the
 * 256 MiB memory-side cache; 1 (the default) = where the table's owned cells x 65 bytes exceed that cache -- a smaller launch finds its
 * state there and keeps the default policy --, 2 = whenever such a launch runs, 0 = never; same bits; gcmf_last_kernel_geometry appends
 * " nt=1" when the streaming form ran),
 * "gap_scratch_mb" N (GCMF_FACES_FROM_NAN: the most scratch, in MiB, the per-entry planes of one launch may take; default 4096; a batch
 * whose planes need more is cut into consecutive launches of at least one entry; same bits; gcmf_apply_bank_gaps: per field, not per
 * entry, and the FIELDS are cut into runs), "adjoint_scratch_mb" N (gcmf_apply_adjoint: the most scratch, in MiB, the pre-scaled planes
 * of one launch may take; default 4096; a longer batch is cut into consecutive launches of at least one entry; same bits),
 * "coarsen_scratch_mb" N (gcmf_apply_coarsen: the most scratch, in MiB, the fine planes of one run of entries may take; default 4096; a
 * longer batch is cut into consecutive runs of at least one entry; same bits), "cov_scratch_mb" N (gcmf_apply_cov: the most scratch, in
 * MiB, one run of pairs may take -- 6 planes per pair, 4 for a variance; default 4096; a longer call is cut into consecutive runs of at
 * least one pair; same bits).  Unknown
 * names: GCMF_ERR_INVALID_ARG. */
int gcmf_set_option(gcmf_plan *plan, const char *name, int value);

/* Last error text of the calling thread (never NULL). */
const char *gcmf_last_error(void);
int gcmf_version(void);
/* sha256 (64 hex digits) of the sources and compiler flags this binary was built from; the loader
 * (gcm_filters_amd/_lib.py load()) recomputes it from csrc/ + include/gcmf.h and refuses a binary that does not match. */
const char *gcmf_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* GCMF_H */
