// Plan-time coefficient folding + validation: the device-side counterpart of the reference Laplacians'
// __post_init__ methods (gcm_filters/kernels.py:163-170, 259-295, 345-349, 402-406, 454-467, 517-562,
// 630-645) and of the field-independent half of BgridVectorLaplacian.__call__ (kernels.py:746-809, which the
// reference recomputes on every call).  Runs once per plan; the results stay resident in HBM.
//
// Every kernel here works on GLOBAL (ny, nx) planes with periodic wrap in x and y (np.roll semantics) and
// the tripole fold where the grid type has one; row slabs for multi-GPU plans are cut out afterwards.
#include "gcmf_internal.hpp"
#include "gcmf_gap_fold.hpp"   // the per-entry fold rule of GCMF_FACES_FROM_NAN, shared with a host program

#include <cmath>

namespace gcmf {

// validation flag bits written by the kernels
enum : int {
  F_KW_GT1 = 1,       // some kappa_w > 1
  F_KS_GT1 = 2,       // some kappa_s > 1
  F_K_NEAR1 = 4,      // some kappa within 1e-5 of 1
  F_MASK_NONBIN = 8,  // wet mask has a value other than 0 / 1
};

__device__ __forceinline__ int wrapi(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

#define CELL_LOOP(ny, nx)                                                                             \
  const long long ncell_ = (long long)(ny) * (nx);                                                    \
  for (long long q_ = (long long)blockIdx.x * blockDim.x + threadIdx.x; q_ < ncell_;                  \
       q_ += (long long)gridDim.x * blockDim.x)
#define CELL_JI(nx) const int j = (int)(q_ / (nx)); const int i = (int)(q_ - (long long)j * (nx));
#define AT(p, jj, ii) (p)[(long long)(jj) * nx + (ii)]

// ---- land-mask neighbour bits (REGULAR_WITH_LAND*, TRIPOLAR_REGULAR*) -------------------------------
// FROM_NAN (GCMF_MASK_FROM_NAN, per call): `m` = the fields of a batch (gridDim.y entries of ny x nx cells), `wet` = the plan's own mask
// bytes; entry b gets its own plane of `bits` from the mask wet * [field_b is not NaN] -- the same neighbours, the same byte layout.
template <typename T, bool FROM_NAN = false>
__global__ void k_pre_mask(const T *m, uint8_t *bits, int ny, int nx, int tripolar, int *flags, const uint8_t *wet) {
  if constexpr (FROM_NAN) {
    m += (long long)blockIdx.y * ny * nx;
    bits += (long long)blockIdx.y * ny * nx;
  }
  auto open = [&](int jj, int ii) -> bool {   // is cell (jj, ii) wet?
    const T v = AT(m, jj, ii);
    if constexpr (FROM_NAN) return (AT(wet, jj, ii) & 1u) && v == v;
    else return v != T(0);
  };
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int ie = wrapi(i + 1, nx), iw = wrapi(i - 1, nx);
    if constexpr (!FROM_NAN) {
      const T mc = AT(m, j, i);
      if (!(mc == T(0) || mc == T(1))) atomicOr(flags, F_MASK_NONBIN);
    }
    unsigned b = open(j, i) ? 1u : 0u;
    if (open(j, ie)) b |= 2u;
    if (open(j, iw)) b |= 4u;
    bool mn, ms;
    if (tripolar) {  // extended mask: row ny is row ny-1 mirrored; row 0's south is that ghost row (kernels.py:461-466)
      mn = (j < ny - 1) ? open(j + 1, i) : open(ny - 1, nx - 1 - i);
      ms = (j > 0) ? open(j - 1, i) : open(ny - 1, nx - 1 - i);
    } else {
      mn = open(wrapi(j + 1, ny), i);
      ms = open(wrapi(j - 1, ny), i);
    }
    if (mn) b |= 8u;
    if (ms) b |= 16u;
    b |= (unsigned)__popc((b >> 1) & 0xFu) << 5;  // bits 5-7: number of wet neighbours (saves the kernels a popcount)
    bits[q_] = (uint8_t)b;
  }
}

// The mask bytes of every entry of a batch of fields (whole-grid K_MASK plans; `wet`: the plan's own bytes, `bits`: nbatch planes of
// rows x nx bytes)
int launch_field_masks(gcmf_plan *pl, const uint8_t *wet, const void *fields, uint8_t *bits, int64_t nbatch, hipStream_t s) {
  const int ny = (int)pl->d.ny, nx = (int)pl->d.nx;
  const long long plane = (long long)ny * nx;
  dim3 block(256), grid((unsigned)std::min<long long>((plane + 255) / 256, 4096), (unsigned)nbatch);
  if (pl->d.dtype == GCMF_F64)
    hipLaunchKernelGGL((k_pre_mask<double, true>), grid, block, 0, s, (const double *)fields, bits, ny, nx, pl->tripolar ? 1 : 0,
                       (int *)nullptr, wet);
  else
    hipLaunchKernelGGL((k_pre_mask<float, true>), grid, block, 0, s, (const float *)fields, bits, ny, nx, pl->tripolar ? 1 : 0,
                       (int *)nullptr, wet);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

// ---- cells that exchange nothing with their neighbours ---------------------------------------------------
// flux form: all four faces of the cell are closed (and, on the tripole seam, the partner's face onto it)
//
// GAPS (GCMF_FACES_FROM_NAN, per call; f64, nx a multiple of 4, no tripole seam): cE / cN / ra = an ordinary plan's planes, `field` = the
// fields of a batch (gridDim.y entries of ny x nx cells); entry b gets its own cEo / cNo / rao planes and plane of `bits`, folded from the
// plan's planes and the entry's NaNs by the rule of gcmf_gap_fold.hpp (MOM5: the reference's transposed mask pairs) -- ONE streaming pass:
// a lane owns four consecutive cells of a row, reads three rows of the field (columns i0 - 1 .. i0 + 4: 16-byte loads where the caller's
// array allows them), cE at i0 - 1 .. i0 + 3, cN and ra of its row and cN of the row below, and writes 2 x 32 bytes of coefficients, 32
// bytes of ra and the four land bytes as one 32-bit word.  The fold needs the west and south neighbours' ENTRY coefficients for the byte:
// they are recomputed from the same loads, not read back.
template <typename T> struct alignas(16) GapPair { T a, b; };
template <typename T> __device__ __forceinline__ void gap_load4(const T *p, bool al16, T *v) {
  if (al16) {
    const GapPair<T> lo = *reinterpret_cast<const GapPair<T> *>(p), hi = *reinterpret_cast<const GapPair<T> *>(p + 2);
    v[0] = lo.a; v[1] = lo.b; v[2] = hi.a; v[3] = hi.b;
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
}
template <typename T> __device__ __forceinline__ void gap_store4(T *p, const T *v) {   // (the work buffer's planes: always aligned)
  *reinterpret_cast<GapPair<T> *>(p) = GapPair<T>{v[0], v[1]};
  *reinterpret_cast<GapPair<T> *>(p + 2) = GapPair<T>{v[2], v[3]};
}

template <typename T, bool GAPS = false, bool MOM5 = false>
__global__ void k_pre_isolated(const T *cE, const T *cN, uint8_t *bits, int ny, int nx, int tripolar, int *count, const T *field,
                               T *cEo, T *cNo, const T *ra, T *rao) {
  if constexpr (GAPS) {
    static_assert(sizeof(T) == 8, "the per-entry fold exists for f64 plans");
    const long long plane = (long long)ny * nx, eoff = (long long)blockIdx.y * plane;
    field += eoff; cEo += eoff; cNo += eoff; rao += eoff; bits += eoff;
    const bool al16 = (reinterpret_cast<uintptr_t>(field) & 15u) == 0;   // (nx % 4 == 0: one answer for every quad of the entry)
    const int nq = nx >> 2;
    const long long nquad = (long long)ny * nq;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (long long)gridDim.x * blockDim.x) {
      const int j = (int)(q / nq), i0 = (int)(q - (long long)j * nq) * 4;
      const int iw = wrapi(i0 - 1, nx), ie = wrapi(i0 + 4, nx);
      const long long rj = (long long)j * nx, rn = (long long)wrapi(j + 1, ny) * nx, rs = (long long)wrapi(j - 1, ny) * nx;
      // n[r][k]: is the field present at row (south, own, north)[r], column i0 - 1 + k
      bool n[3][6];
      const long long rows[3] = {rs, rj, rn};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        T v[4];
        gap_load4(field + rows[r] + i0, al16, v);
        n[r][0] = gap_present(field[rows[r] + iw]);
#pragma unroll
        for (int k = 0; k < 4; ++k) n[r][1 + k] = gap_present(v[k]);
        n[r][5] = gap_present(field[rows[r] + ie]);
      }
      T e[5], cn[4], cs[4], rv[4];
      e[0] = cE[rj + iw];
      gap_load4(cE + rj + i0, true, e + 1);
      gap_load4(cN + rj + i0, true, cn);
      gap_load4(cN + rs + i0, true, cs);
      gap_load4(ra + rj + i0, true, rv);
      T eb[5], nb[4];
      unsigned word = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) eb[k] = gap_fold_cE<T, MOM5>(e[k], n[1][k], n[1][k + 1], n[2][k]);   // columns i0 - 1 .. i0 + 3
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        nb[k] = gap_fold_cN<T, MOM5>(cn[k], n[1][k + 1], n[1][k + 2], n[2][k + 1]);
        const T sb = gap_fold_cN<T, MOM5>(cs[k], n[0][k + 1], n[0][k + 2], n[1][k + 1]);   // the southern neighbour's north face
        word |= gap_land_byte(eb[k + 1], eb[k], nb[k], sb) << (8 * k);
      }
      gap_store4(cEo + rj + i0, eb + 1);
      gap_store4(cNo + rj + i0, nb);
      gap_store4(rao + rj + i0, rv);
      *reinterpret_cast<unsigned *>(bits + rj + i0) = word;
    }
    return;
  }
  int mine = 0;
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int iw = wrapi(i - 1, nx);
    bool open = (AT(cE, j, i) != T(0)) || (AT(cE, j, iw) != T(0)) || (AT(cN, j, i) != T(0));
    if (tripolar) {
      if (j > 0) open = open || (AT(cN, j - 1, i) != T(0));
      if (j == ny - 1) open = open || (AT(cN, ny - 1, nx - 1 - i) != T(0));
    } else {
      open = open || (AT(cN, wrapi(j - 1, ny), i) != T(0));
    }
    bits[q_] = open ? 1u : 0u;
    if (!open) ++mine;
  }
  if (mine) atomicAdd(count, mine);
}
__global__ void k_count_land(const uint8_t *bits, long long n, int *count) {
  int mine = 0;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x)
    mine += (bits[q] & 1u) ? 0 : 1;
  if (mine) atomicAdd(count, mine);
}

// ---- IRREGULAR_WITH_LAND: W/S-face form -> east/north-face coefficient planes ------------------------
// reference: wflux = (g - W g)/dxw*dyw * (m*W m*kappa_w); L = (E wflux - wflux + N sflux - sflux)/area
template <typename T>
__global__ void k_pre_irregular(const T *m, const T *dxw, const T *dyw, const T *dxs, const T *dys, const T *area,
                                const T *kw, const T *ks, T *cE, T *cN, T *ra, int ny, int nx, int *flags) {
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int ie = wrapi(i + 1, nx), jn = wrapi(j + 1, ny);
    const T kwc = AT(kw, j, i), ksc = AT(ks, j, i);
    int f = 0;
    if (kwc > T(1)) f |= F_KW_GT1;
    if (ksc > T(1)) f |= F_KS_GT1;
    if (fabs((double)kwc - 1.0) <= 1e-5 || fabs((double)ksc - 1.0) <= 1e-5) f |= F_K_NEAR1;
    if (f & ~*(volatile int *)flags) atomicOr(flags, f);
    // east face of (j,i) == west face of (j,i+1)
    cE[q_] = AT(dyw, j, ie) / AT(dxw, j, ie) * (AT(m, j, ie) * AT(m, j, i) * AT(kw, j, ie));
    // north face of (j,i) == south face of (j+1,i)
    cN[q_] = AT(dxs, jn, i) / AT(dys, jn, i) * (AT(m, jn, i) * AT(m, j, i) * AT(ks, jn, i));
    ra[q_] = T(1) / AT(area, j, i);
  }
}

// ---- TRIPOLAR_POP_WITH_LAND: E/N-face form with the north fold ---------------------------------------
template <typename T>
__global__ void k_pre_pop(const T *m, const T *dxe, const T *dye, const T *dxn, const T *dyn, const T *tarea, T *cE,
                          T *cN, T *ra, int ny, int nx) {
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int ie = wrapi(i + 1, nx);
    const T mc = AT(m, j, i);
    const T mn = (j < ny - 1) ? AT(m, j + 1, i) : AT(m, ny - 1, nx - 1 - i);
    cE[q_] = AT(dye, j, i) / AT(dxe, j, i) * (mc * AT(m, j, ie));
    cN[q_] = AT(dxn, j, i) / AT(dyn, j, i) * (mc * mn);
    ra[q_] = T(1) / AT(tarea, j, i);
  }
}

// ---- MOM5U / MOM5T (kernels.py:345-372, 402-429) ------------------------------------------------------
// Both reduce to north-face / east-face flux form.  NB the reference masks the axis -2 ("fx") difference
// with m*E(m) and the axis -1 ("fy") difference with m*N(m); reproduced as written.
template <typename T>
__global__ void k_pre_mom5(const T *m, const T *dxt, const T *dyt, const T *dxu, const T *dyu, const T *area, T *cE,
                           T *cN, T *ra, int ny, int nx, int is_u) {
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int ie = wrapi(i + 1, nx), iw = wrapi(i - 1, nx), jn = wrapi(j + 1, ny), js = wrapi(j - 1, ny);
    const T mc = AT(m, j, i);
    const T mask_a = mc * AT(m, j, ie);
    const T mask_b = mc * AT(m, jn, i);
    T cn, ce;
    if (is_u) {
      cn = T(2) / (AT(dxt, jn, i) + AT(dxt, jn, ie)) * mask_a * (T(0.5) * (AT(dyu, j, i) + AT(dyu, jn, i)));
      ce = T(2) / (AT(dyt, j, ie) + AT(dyt, jn, ie)) * mask_b * (T(0.5) * (AT(dxu, j, i) + AT(dxu, j, ie)));
    } else {
      cn = T(2) / (AT(dxu, j, i) + AT(dxu, j, iw)) * mask_a * (T(0.5) * (AT(dyt, j, i) + AT(dyt, jn, i)));
      ce = T(2) / (AT(dyu, j, i) + AT(dyu, js, i)) * mask_b * (T(0.5) * (AT(dxt, j, i) + AT(dxt, j, ie)));
    }
    cN[q_] = cn;
    cE[q_] = ce;
    ra[q_] = T(1) / AT(area, j, i);
  }
}

// ---- VECTOR_C_GRID (kernels.py:630-645 + the field-independent factors of 647-696) -------------------
// planes out: 0 1/dyCu  1 1/dxCu  2 1/dxCv  3 1/dyCv
//             4 a1 = -(k_iso + k_aniso/2) * dyT/dxT*mt * dyT^2     5 a2 = -(..)*dxT/dyT*mt * dyT^2   6 rh = dxT^2/dyT^2
//             7 b1 = -k_iso * dyBu/dxBu*mq * dxBu^2                8 b2 = -k_iso*dxBu/dyBu*mq*dxBu^2  9 rq = dyBu^2/dxBu^2
//             10 rau/dyCu   11 rau/dxCu   12 rav/dyCv   13 rav/dxCv        (rau = area_u>0 ? 1/area_u : 0)
// so that  P = dy2h*str_xx = a1*(u~ - W u~) - a2*(v~ - S v~),  dx2h*str_xx = rh*P,
//          R = dx2q*str_xy = b1*(E v^ - v^) + b2*(N u^ - u^),  dy2q*str_xy = rq*R.
template <typename T> struct CgridIn {
  const T *mt, *mq, *dxT, *dyT, *dxCu, *dyCu, *dxCv, *dyCv, *dxBu, *dyBu, *area_u, *area_v, *kiso, *kaniso;
};
template <typename T> struct Planes14 { T *p[14]; };

template <typename T> __global__ void k_pre_cgrid(const CgridIn<T> in, Planes14<T> o, int ny, int nx) {
  CELL_LOOP(ny, nx) {
    const long long q = q_;
    const T dxT = in.dxT[q], dyT = in.dyT[q], dxBu = in.dxBu[q], dyBu = in.dyBu[q];
    const T dx_dyT = dxT / dyT * in.mt[q], dy_dxT = dyT / dxT * in.mt[q];
    const T dx_dyBu = dxBu / dyBu * in.mq[q], dy_dxBu = dyBu / dxBu * in.mq[q];
    const T dx2h = dxT * dxT, dy2h = dyT * dyT, dx2q = dxBu * dxBu, dy2q = dyBu * dyBu;
    const T au = in.area_u[q], av = in.area_v[q];
    const T rau = au > T(0) ? T(1) / au : T(0), rav = av > T(0) ? T(1) / av : T(0);
    const T kxx = -(in.kiso[q] + T(0.5) * in.kaniso[q]), kxy = -in.kiso[q];
    o.p[0][q] = T(1) / in.dyCu[q];
    o.p[1][q] = T(1) / in.dxCu[q];
    o.p[2][q] = T(1) / in.dxCv[q];
    o.p[3][q] = T(1) / in.dyCv[q];
    o.p[4][q] = kxx * dy_dxT * dy2h;
    o.p[5][q] = kxx * dx_dyT * dy2h;
    o.p[6][q] = dx2h / dy2h;
    o.p[7][q] = kxy * dy_dxBu * dx2q;
    o.p[8][q] = kxy * dx_dyBu * dx2q;
    o.p[9][q] = dy2q / dx2q;
    o.p[10][q] = rau / in.dyCu[q];
    o.p[11][q] = rau / in.dxCu[q];
    o.p[12][q] = rav / in.dyCv[q];
    o.p[13][q] = rav / in.dxCv[q];
  }
}

// ---- VECTOR_B_GRID: the ten POP stencil weights, in the reference's operation order ------------------
// pass 1: kxt = (HTE - N HTE)/TAREA, kyt = (HTN - E HTN)/TAREA       (kernels.py:773, 780)
template <typename T>
__global__ void k_pre_bgrid1(const T *HTE, const T *HTN, const T *TAREA, T *kxt, T *kyt, int ny, int nx) {
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const T rt = T(1) / AT(TAREA, j, i);
    kxt[q_] = (AT(HTE, j, i) - AT(HTE, wrapi(j + 1, ny), i)) * rt;
    kyt[q_] = (AT(HTN, j, i) - AT(HTN, j, wrapi(i + 1, nx))) * rt;
  }
}
// pass 2: planes out: 0 cc  1 DUN  2 DUS  3 DUE  4 DUW  5 DMC  6 DMN  7 DME      (DMS = -DMN, DMW = -DME)
template <typename T> struct BgridIn { const T *DXU, *DYU, *HUS, *HUW, *HTE, *HTN, *UAREA, *kxt, *kyt; };
template <typename T> struct Planes8 { T *p[8]; };

template <typename T> __global__ void k_pre_bgrid2(const BgridIn<T> in, Planes8<T> o, int ny, int nx) {
  CELL_LOOP(ny, nx) {
    CELL_JI(nx)
    const int iw = wrapi(i - 1, nx), js = wrapi(j - 1, ny);
    const T ru = T(1) / AT(in.UAREA, j, i), rdx = T(1) / AT(in.DXU, j, i), rdy = T(1) / AT(in.DYU, j, i);
    auto w1 = [&](int jj, int ii) { return AT(in.HUS, jj, ii) / AT(in.HTE, jj, ii); };
    auto w2 = [&](int jj, int ii) { return AT(in.HUW, jj, ii) / AT(in.HTN, jj, ii); };
    const T dus = w1(j, i) * ru, dun = w1(j, iw) * ru;
    const T duw = w2(j, i) * ru, due = w2(js, i) * ru;
    const T kxu = (AT(in.HUW, js, i) - AT(in.HUW, j, i)) * ru;
    const T kyu = (AT(in.HUS, j, iw) - AT(in.HUS, j, i)) * ru;
    // averages of kxt / kyt: a(jj,ii) = 0.5*(k + W k), b(jj,ii) = 0.5*(k + S k)
    auto ax = [&](const T *k, int jj, int ii) { return T(0.5) * (AT(k, jj, ii) + AT(k, jj, wrapi(ii - 1, nx))); };
    auto ay = [&](const T *k, int jj, int ii) { return T(0.5) * (AT(k, jj, ii) + AT(k, wrapi(jj - 1, ny), ii)); };
    const T dxkx = (ax(in.kxt, js, i) - ax(in.kxt, j, i)) * rdx;
    const T dykx = (ay(in.kxt, j, iw) - ay(in.kxt, j, i)) * rdy;
    const T dyky = (ay(in.kyt, j, iw) - ay(in.kyt, j, i)) * rdy;
    const T dxky = (ax(in.kyt, js, i) - ax(in.kyt, j, i)) * rdx;
    const T dum = -(dxkx + dyky + T(2) * (kxu * kxu + kyu * kyu));
    const T dmc = dxky - dykx;
    const T dme = (T(2) * kyu) / (AT(in.HTN, j, i) + AT(in.HTN, js, i));
    const T dmn = -(T(2) * kxu) / (AT(in.HTE, j, i) + AT(in.HTE, j, iw));
    const T duc = -(dun + dus + due + duw);
    o.p[0][q_] = duc + dum;
    o.p[1][q_] = dun;
    o.p[2][q_] = dus;
    o.p[3][q_] = due;
    o.p[4][q_] = duw;
    o.p[5][q_] = dmc;
    o.p[6][q_] = dmn;
    o.p[7][q_] = dme;
  }
}

// ------------------------------------------------------------------------------------------------------
static int dev_alloc(gcmf_plan *pl, void **p, size_t bytes) {
  GCMF_HIP(hipMalloc(p, bytes));
  pl->owned.push_back(*p);
  return GCMF_OK;
}

// cut rows [first .. first+rows) (mod ny when periodic) of a global plane into a slab allocation
static int cut_rows(gcmf_plan *pl, const void *global_plane, void **slab, size_t elem, hipStream_t s) {
  const int64_t ny = pl->d.ny, nx = pl->d.nx;
  const size_t row_bytes = (size_t)nx * elem;
  int rc = dev_alloc(pl, slab, (size_t)pl->rows_alloc * row_bytes);
  if (rc) return rc;
  const int64_t g0 = pl->d.row_begin - pl->first_owned;
  for (int64_t r = 0; r < pl->rows_alloc;) {  // copy maximal contiguous runs
    int64_t gj = ((g0 + r) % ny + ny) % ny;
    int64_t run = std::min<int64_t>(pl->rows_alloc - r, ny - gj);
    GCMF_HIP(hipMemcpyAsync((char *)*slab + r * row_bytes, (const char *)global_plane + gj * row_bytes, run * row_bytes,
                            hipMemcpyDeviceToDevice, s));
    r += run;
  }
  return GCMF_OK;
}

template <typename T> static int host_rows(const void *dplane, const void *hplane, int64_t row, int64_t nx, std::vector<T> &out) {
  out.resize(nx);
  if (hplane) {
    const T *p = (const T *)hplane + row * nx;
    std::copy(p, p + nx, out.begin());
  } else {
    GCMF_HIP(hipMemcpy(out.data(), (const T *)dplane + row * nx, nx * sizeof(T), hipMemcpyDeviceToHost));
  }
  return GCMF_OK;
}

// tripolar checks of kernels.py:458-459 / 521-522 (southern row all land) and 547-562 (fold of dxn / dyn)
template <typename T>
static int check_tripolar(gcmf_plan *pl, const void *const *dp, const void *const *hp, int mask_idx, int dxn_idx,
                          int dyn_idx) {
  const int64_t ny = pl->d.ny, nx = pl->d.nx;
  std::vector<T> m0, mtop, dxn, dyn;
  int rc = host_rows<T>(dp[mask_idx], hp ? hp[mask_idx] : nullptr, 0, nx, m0);
  if (rc) return rc;
  for (int64_t i = 0; i < nx; ++i)
    if (m0[i] != T(0)) {
      set_error("Wet mask requires zeros in southernmost row");
      return GCMF_ERR_WET_SOUTH_ROW;
    }
  if (dxn_idx < 0) return GCMF_OK;
  if ((rc = host_rows<T>(dp[mask_idx], hp ? hp[mask_idx] : nullptr, ny - 1, nx, mtop))) return rc;
  if ((rc = host_rows<T>(dp[dxn_idx], hp ? hp[dxn_idx] : nullptr, ny - 1, nx, dxn))) return rc;
  if ((rc = host_rows<T>(dp[dyn_idx], hp ? hp[dyn_idx] : nullptr, ny - 1, nx, dyn))) return rc;
  if (nx % 2) {
    set_error("tripolar fold check needs an even nx (the reference raises a broadcast ValueError for odd nx)");
    return GCMF_ERR_INVALID_ARG;
  }
  const int64_t h = nx / 2;
  auto wet_only = [&](const std::vector<T> &a, int64_t i) {  // where(n_wet_mask == 1, a, 0) on row ny-1
    return (mtop[i] * mtop[nx - 1 - i] == T(1)) ? a[i] : T(0);
  };
  for (int64_t i = 0; i < h; ++i) {
    const T left = wet_only(dxn, h - 1 - i), right = wet_only(dxn, h + i);
    if (!(left == right)) {
      set_error("Northernmost row of dxn does not fold onto itself. This is a requirement for using a tripole boundary condition.");
      return GCMF_ERR_DXN_FOLD;
    }
  }
  for (int64_t i = 0; i < h; ++i) {  // np.allclose(a, b): |a-b| <= 1e-8 + 1e-5 |b|, finite only
    const double a = (double)wet_only(dyn, h - 1 - i), b = (double)wet_only(dyn, h + i);
    const bool close = (a == b) || (std::isfinite(a) && std::isfinite(b) && std::fabs(a - b) <= 1e-8 + 1e-5 * std::fabs(b));
    if (!close) {
      set_error("Northernmost row of dyn does not fold onto itself. This is a requirement for using a tripole boundary condition.");
      return GCMF_ERR_DYN_FOLD;
    }
  }
  return GCMF_OK;
}

template <typename T> static int precompute_t(gcmf_plan *pl, const void *const *dp, const void *const *hp) {
  const int ny = (int)pl->d.ny, nx = (int)pl->d.nx;
  const size_t plane = (size_t)ny * nx;
  hipStream_t s = pl->stream;
  const dim3 block(256), grid((unsigned)std::min<size_t>((plane + 255) / 256, 8192));
  Geom &g = pl->g;
  int *dflags = nullptr;
  GCMF_HIP(hipMalloc((void **)&dflags, sizeof(int)));
  struct FlagGuard { int *p; ~FlagGuard() { (void)hipFree(p); } } guard{dflags};
  GCMF_HIP(hipMemsetAsync(dflags, 0, sizeof(int), s));
  auto P = [&](int k) { return (const T *)dp[k]; };

  std::vector<void *> gplanes;  // global coefficient planes produced below (T unless noted)
  std::vector<void *> temps;
  struct TempGuard { std::vector<void *> &v; ~TempGuard() { for (void *p : v) (void)hipFree(p); } } tguard{temps};
  auto galloc = [&](void **p, size_t bytes) -> int {
    GCMF_HIP(hipMalloc(p, bytes));
    temps.push_back(*p);
    return GCMF_OK;
  };
  int rc;
  uint8_t *gbits = nullptr;
  int area_idx = -1;
  const int gt = pl->d.grid_type;

  switch (gt) {
    case GCMF_REGULAR: break;
    case GCMF_REGULAR_AREA_WEIGHTED: area_idx = 0; break;
    case GCMF_REGULAR_WITH_LAND:
    case GCMF_REGULAR_WITH_LAND_AREA_WEIGHTED:
    case GCMF_TRIPOLAR_REGULAR_WITH_LAND_AREA_WEIGHTED: {
      const int mi = (gt == GCMF_REGULAR_WITH_LAND) ? 0 : 1;
      if (gt != GCMF_REGULAR_WITH_LAND) area_idx = 0;
      if (pl->tripolar && (rc = check_tripolar<T>(pl, dp, hp, mi, -1, -1))) return rc;
      if ((rc = galloc((void **)&gbits, plane))) return rc;
      hipLaunchKernelGGL(k_pre_mask<T>, grid, block, 0, s, P(mi), gbits, ny, nx, pl->tripolar ? 1 : 0, dflags, (const uint8_t *)nullptr);
      break;
    }
    case GCMF_IRREGULAR_WITH_LAND:
    case GCMF_MOM5U:
    case GCMF_MOM5T:
    case GCMF_TRIPOLAR_POP_WITH_LAND: {
      if (gt == GCMF_TRIPOLAR_POP_WITH_LAND && (rc = check_tripolar<T>(pl, dp, hp, 0, 3, 4))) return rc;
      T *c[3];
      for (auto &p : c) {
        if ((rc = galloc((void **)&p, plane * sizeof(T)))) return rc;
        gplanes.push_back(p);
      }
      if (gt == GCMF_IRREGULAR_WITH_LAND)
        hipLaunchKernelGGL(k_pre_irregular<T>, grid, block, 0, s, P(0), P(1), P(2), P(3), P(4), P(5), P(6), P(7), c[0],
                           c[1], c[2], ny, nx, dflags);
      else if (gt == GCMF_TRIPOLAR_POP_WITH_LAND)
        hipLaunchKernelGGL(k_pre_pop<T>, grid, block, 0, s, P(0), P(1), P(2), P(3), P(4), P(5), c[0], c[1], c[2], ny, nx);
      else
        hipLaunchKernelGGL(k_pre_mom5<T>, grid, block, 0, s, P(0), P(1), P(2), P(3), P(4), P(5), c[0], c[1], c[2], ny, nx,
                           gt == GCMF_MOM5U ? 1 : 0);
      break;
    }
    case GCMF_VECTOR_C_GRID: {
      CgridIn<T> in{P(0), P(1), P(2), P(3), P(4), P(5), P(6), P(7), P(8), P(9), P(10), P(11), P(12), P(13)};
      Planes14<T> o;
      for (auto &p : o.p) {
        if ((rc = galloc((void **)&p, plane * sizeof(T)))) return rc;
        gplanes.push_back(p);
      }
      hipLaunchKernelGGL(k_pre_cgrid<T>, grid, block, 0, s, in, o, ny, nx);
      break;
    }
    case GCMF_VECTOR_B_GRID: {
      T *kxt, *kyt;
      if ((rc = galloc((void **)&kxt, plane * sizeof(T)))) return rc;
      if ((rc = galloc((void **)&kyt, plane * sizeof(T)))) return rc;
      hipLaunchKernelGGL(k_pre_bgrid1<T>, grid, block, 0, s, P(4), P(5), P(7), kxt, kyt, ny, nx);
      BgridIn<T> in{P(0), P(1), P(2), P(3), P(4), P(5), P(6), kxt, kyt};
      Planes8<T> o;
      for (auto &p : o.p) {
        if ((rc = galloc((void **)&p, plane * sizeof(T)))) return rc;
        gplanes.push_back(p);
      }
      hipLaunchKernelGGL(k_pre_bgrid2<T>, grid, block, 0, s, in, o, ny, nx);
      break;
    }
    default: set_error("unknown grid type %d", gt); return GCMF_ERR_INVALID_ARG;
  }
  GCMF_HIP(hipGetLastError());

  // scalar plans: which cells never exchange with a neighbour (see gcmf_plan::lbits), in slab-row layout
  int *dcount = nullptr;
  uint8_t *gisol = nullptr;
  const bool flux_kind = (gt == GCMF_IRREGULAR_WITH_LAND || gt == GCMF_MOM5U || gt == GCMF_MOM5T || gt == GCMF_TRIPOLAR_POP_WITH_LAND);
  if (gbits || flux_kind) {
    if ((rc = galloc((void **)&dcount, sizeof(int)))) return rc;
    GCMF_HIP(hipMemsetAsync(dcount, 0, sizeof(int), s));
    if (gbits) {
      hipLaunchKernelGGL(k_count_land, grid, block, 0, s, gbits, (long long)plane, dcount);
    } else {
      if ((rc = galloc((void **)&gisol, plane))) return rc;
      hipLaunchKernelGGL(k_pre_isolated<T>, grid, block, 0, s, (const T *)gplanes[0], (const T *)gplanes[1], gisol, ny, nx,
                         pl->tripolar ? 1 : 0, dcount, (const T *)nullptr, (T *)nullptr, (T *)nullptr, (const T *)nullptr, (T *)nullptr);
    }
    GCMF_HIP(hipGetLastError());
  }

  // validation results
  int flags = 0;
  GCMF_HIP(hipMemcpyAsync(&flags, dflags, sizeof(int), hipMemcpyDeviceToHost, s));
  GCMF_HIP(hipStreamSynchronize(s));
  if (gt == GCMF_IRREGULAR_WITH_LAND) {
    if (flags & F_KW_GT1) {
      set_error("There are kappa_w values > 1 and this can cause the filter to blow up.Please make sure all kappa_w are <=1.");
      return GCMF_ERR_KAPPA_W_GT1;
    }
    if (flags & F_KS_GT1) {
      set_error("There are kappa_s values > 1 and this can cause the filter to blow up.Please make sure all kappa_s are <=1.");
      return GCMF_ERR_KAPPA_S_GT1;
    }
    if (!(flags & F_K_NEAR1) && !(pl->d.flags & GCMF_PLAN_SKIP_KAPPA_ONE)) {
      set_error("At least one place in the domain must have either kappa_w = 1 or kappa_s = 1. Otherwise the filter's "
                "scale will not be equal to filter_scale anywhere in the domain.");
      return GCMF_ERR_KAPPA_NONE_ONE;
    }
  }
  if (flags & F_MASK_NONBIN) {
    set_error("wet_mask must contain only 0 and 1");
    return GCMF_ERR_UNSUPPORTED;
  }

  // slab cut: coefficient planes live in slab-row layout (== global layout for a single slab)
  for (size_t k = 0; k < gplanes.size(); ++k) {
    void *slab = nullptr;
    if ((rc = cut_rows(pl, gplanes[k], &slab, sizeof(T), s))) return rc;
    g.coef[k] = slab;
  }
  if (gbits) {
    void *slab = nullptr;
    if ((rc = cut_rows(pl, gbits, &slab, 1, s))) return rc;
    g.mbits = (const uint8_t *)slab;
  }
  if (dcount) {
    int n_land = 0;
    GCMF_HIP(hipMemcpyAsync(&n_land, dcount, sizeof(int), hipMemcpyDeviceToHost, s));
    GCMF_HIP(hipStreamSynchronize(s));
    pl->n_land = n_land;  // of the whole grid
    if (gisol) {
      void *slab = nullptr;
      if ((rc = cut_rows(pl, gisol, &slab, 1, s))) return rc;
      pl->lbits = (const uint8_t *)slab;
    } else {
      pl->lbits = g.mbits;
    }
  }
  if (area_idx >= 0) {
    void *slab = nullptr;
    if ((rc = cut_rows(pl, dp[area_idx], &slab, sizeof(T), s))) return rc;
    g.area = slab;
  }
  if (gt == GCMF_VECTOR_C_GRID)   // area_u, area_v: the diagonal of gcmf_apply_adjoint's similarity (gcmf_plan::adj_area)
    for (int k = 0; k < 2; ++k) {
      void *slab = nullptr;
      if ((rc = cut_rows(pl, dp[10 + k], &slab, sizeof(T), s))) return rc;
      pl->adj_area[k] = slab;
    }
  GCMF_HIP(hipStreamSynchronize(s));
  return GCMF_OK;
}

// A stacked plan (gcmf_plan_create_levels; the caller has checked: an f64 flux kind without a seam, the whole grid): the fold kernels of
// the ordinary plan run once per level into (nlev, ny, nx) coefficient planes and land bytes -- a whole grid's slab layout is the global
// one, nothing is cut.  Plane k of the input has plane_levels[k] planes: 1 = shared by all levels.  Validation as the reference applies it
// to grid variables with leading dims (kernels.py:262-281 on the whole arrays): a kappa > 1 on any level fails, and "no kappa equals 1"
// fails only when no level has one -- the flag word is shared by the levels.
int precompute_levels(gcmf_plan *pl, const void *const *dp, const int64_t *plane_levels) {
  using T = double;
  const int ny = (int)pl->d.ny, nx = (int)pl->d.nx, gt = pl->d.grid_type;
  const size_t plane = (size_t)ny * nx;
  const int64_t nlev = pl->nlev;
  hipStream_t s = pl->stream;
  const dim3 block(256), grid((unsigned)std::min<size_t>((plane + 255) / 256, 8192));
  int *dflags = nullptr;   // [0] validation flags of all levels, [1] isolated cells of the level that runs now
  GCMF_HIP(hipMalloc((void **)&dflags, 2 * sizeof(int)));
  struct FlagGuard { int *p; ~FlagGuard() { (void)hipFree(p); } } guard{dflags};
  GCMF_HIP(hipMemsetAsync(dflags, 0, 2 * sizeof(int), s));
  int rc;
  T *c[3];
  for (auto &p : c)
    if ((rc = dev_alloc(pl, (void **)&p, (size_t)nlev * plane * sizeof(T) + 256))) return rc;
  uint8_t *isol = nullptr;
  if ((rc = dev_alloc(pl, (void **)&isol, (size_t)nlev * plane + 256))) return rc;
  int64_t n_land = 0;
  for (int64_t l = 0; l < nlev; ++l) {
    auto P = [&](int k) { return (const T *)dp[k] + (plane_levels[k] > 1 ? (size_t)l * plane : 0); };
    T *cE = c[0] + (size_t)l * plane, *cN = c[1] + (size_t)l * plane, *ra = c[2] + (size_t)l * plane;
    if (gt == GCMF_IRREGULAR_WITH_LAND)
      hipLaunchKernelGGL(k_pre_irregular<T>, grid, block, 0, s, P(0), P(1), P(2), P(3), P(4), P(5), P(6), P(7), cE, cN, ra, ny, nx, dflags);
    else
      hipLaunchKernelGGL(k_pre_mom5<T>, grid, block, 0, s, P(0), P(1), P(2), P(3), P(4), P(5), cE, cN, ra, ny, nx, gt == GCMF_MOM5U ? 1 : 0);
    hipLaunchKernelGGL(k_pre_isolated<T>, grid, block, 0, s, (const T *)cE, (const T *)cN, isol + (size_t)l * plane, ny, nx, 0, dflags + 1,
                       (const T *)nullptr, (T *)nullptr, (T *)nullptr, (const T *)nullptr, (T *)nullptr);
    GCMF_HIP(hipGetLastError());
    int got[2] = {0, 0};   // (per level: the count of a deep stack would not fit an int)
    GCMF_HIP(hipMemcpyAsync(got, dflags, sizeof got, hipMemcpyDeviceToHost, s));
    GCMF_HIP(hipMemsetAsync(dflags + 1, 0, sizeof(int), s));
    GCMF_HIP(hipStreamSynchronize(s));
    n_land += got[1];
    if (l + 1 < nlev) continue;
    const int flags = got[0];
    if (gt == GCMF_IRREGULAR_WITH_LAND) {
      if (flags & F_KW_GT1) {
        set_error("There are kappa_w values > 1 and this can cause the filter to blow up.Please make sure all kappa_w are <=1.");
        return GCMF_ERR_KAPPA_W_GT1;
      }
      if (flags & F_KS_GT1) {
        set_error("There are kappa_s values > 1 and this can cause the filter to blow up.Please make sure all kappa_s are <=1.");
        return GCMF_ERR_KAPPA_S_GT1;
      }
      if (!(flags & F_K_NEAR1) && !(pl->d.flags & GCMF_PLAN_SKIP_KAPPA_ONE)) {
        set_error("At least one place in the domain must have either kappa_w = 1 or kappa_s = 1. Otherwise the filter's "
                  "scale will not be equal to filter_scale anywhere in the domain.");
        return GCMF_ERR_KAPPA_NONE_ONE;
      }
    }
  }
  for (int k = 0; k < 3; ++k) pl->g.coef[k] = c[k];
  pl->lbits = isol;
  pl->n_land = n_land;   // of all levels: a plan with land on any level has land
  return GCMF_OK;
}

// The planes of every entry of a batch of fields (GCMF_FACES_FROM_NAN; the caller has checked: a whole f64 plan of IRREGULAR_WITH_LAND,
// MOM5U or MOM5T, nx % 4 == 0; the outputs are nbatch planes each, 16-byte aligned)
int launch_gap_fold(gcmf_plan *pl, const double *cE, const double *cN, const double *ra, const void *fields, double *cEo, double *cNo,
                    double *rao, uint8_t *bits, int64_t nbatch, hipStream_t s) {
  const int ny = (int)pl->d.ny, nx = (int)pl->d.nx;
  if (nx % 4 || pl->d.dtype != GCMF_F64 || nbatch < 1 || nbatch > 65535) {
    set_error("k_pre_isolated (GCMF_FACES_FROM_NAN): needs an f64 plan, nx a multiple of 4 and 1 .. 65535 entries");
    return GCMF_ERR_INVALID_ARG;
  }
  const long long nquad = (long long)ny * (nx / 4);
  dim3 block(256), grid((unsigned)std::min<long long>((nquad + 255) / 256, 4096), (unsigned)nbatch);
  if (pl->d.grid_type == GCMF_IRREGULAR_WITH_LAND)
    hipLaunchKernelGGL((k_pre_isolated<double, true, false>), grid, block, 0, s, cE, cN, bits, ny, nx, 0, (int *)nullptr, (const double *)fields,
                       cEo, cNo, ra, rao);
  else
    hipLaunchKernelGGL((k_pre_isolated<double, true, true>), grid, block, 0, s, cE, cN, bits, ny, nx, 0, (int *)nullptr, (const double *)fields,
                       cEo, cNo, ra, rao);
  GCMF_HIP(hipGetLastError());
  return GCMF_OK;
}

int precompute(gcmf_plan *pl, const void *const *dplanes, const void *const *hplanes) {
  return pl->d.dtype == GCMF_F64 ? precompute_t<double>(pl, dplanes, hplanes) : precompute_t<float>(pl, dplanes, hplanes);
}

}  // namespace gcmf
