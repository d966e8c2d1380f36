// k_ringc: the static-ring kernel (gcmf_ring_impl.hpp) evaluating the filter polynomial BACKWARDS (Clenshaw):
//
//     b_{n+1} = b_{n+2} = 0,   b_k = p_k f + 2 A(b_{k+1}) - b_{k+2}  (k = n .. 1),   result = p_0 f + A(b_1) - b_2,
//     A(x) = -x - c L(x)                                   == sum_k p_k T_k(A) f  of reference filter.py:162-212
//
// The forward recurrence carries three planes per field (T_{k-1}, T_{k-2}, fbar: fbar is read AND written by every launch); the
// backward one carries two (b_{k+1}, b_{k+2}) and re-reads the constant input f: one plane less per launch (8 instead of 9 for
// the flux kinds, 5 + 1 byte instead of 6 + 1 byte for the land-mask kinds), and the kernels run at the rate the memory
// system gives.  Same stencils, same time skewing, rings, halo geometry and launch structure as k_ring:
// b_n = p_n f needs no stencil: the first launch forms it as it loads f (its "input state" is (b_n, 0)); "level" l = 1 .. n of a
// filter produces b_{n-l}, level n the result (its 2 A(.) is A(.)); the n levels are cut into launches of S = 5 .. 8 -- as
// many Laplacian applications and launches as the forward recurrence.
//
//   * same NaN semantics as the reference: the stencil sees nan_to_num of its operands, "-x", b_{k+2} and p_k f keep a NaN, so
//     an input NaN in a wet cell stays in that cell's state and result and its column of the stencil is zero -- exactly
//     what happens to T_k in the forward recurrence.  The fast march only WATCHES (last level); a strip that meets a
//     non-finite value is redone by the SAME march with nan_to_num on the stencil operands (SANI = true), which needs no
//     other kernel: no fbar is accumulated, so a strip is always re-computable from its inputs.
//   * isolated (land) cells: f is masked to zero as it is loaded (every launch: +1 byte per cell), so they stay zero in the
//     state; k_land_fix writes their own polynomial (forward recurrence, as the reference computes it) at the end.
//   * prepare() / finalize() of the area-weighted types: f * area as it is loaded, result / area as it is stored.
//   * rounding differs from the forward recurrence in the last bits (measured <= 3e-15 relative): results are NOT bit-identical
//     with the single-step kernels; they are bit-identical across different cuts of the levels into launches.
//
// f64 state (all scalar kinds) and f32 state of the flux kinds (four cells per lane, f64 result).  On tripolar plans the launch stops S rows
// below the seam and k_fold_band's backward form (gcmf_foldband.hip) advances those rows beside it.
#pragma once
#include "gcmf_ring_impl.hpp"
#include "gcmf_ringc_table.hpp"
#include "gcmf_wet_cut.hpp"

namespace gcmf {

static_assert(RINGC_MASKZ == K_MASKZ, "gcmf_ringc_table.hpp names the land-mask kind of the kernels");

// the VEC bytes (mask bits / land bits) of a lane's cells in one load
template <int VEC> __device__ __forceinline__ unsigned cell_bytes(const uint8_t *p) {
  if constexpr (VEC == 2) return *reinterpret_cast<const unsigned short *>(p);
  else return *reinterpret_cast<const unsigned *>(p);
}

// one march of a strip; returns whether this wave met a non-finite value in its last level (wave-uniform)
// XE: early exits also for the flux kinds (k_ringcs: slabs that do not own a tripole seam, see below)
// ZIP: two strips of one window that share a boundary ("seam") march AWAY from it, side by side in one workgroup (k_ringcz, round 6): neither
// warms its levels up over S ghost rows on that side -- at its first row every level takes the flux across the seam from the row the partner
// has just produced (one row per level through LDS, a workgroup barrier per level: S - 1 of them in the first ring period), so a strip
// marches H + S + 1 rows instead of H + 2 S and all its levels start within S + 1 phases.  Same operands, same operations: same bits.
// (wx: the wave's window; [a, b): the rows it owns; boff: its field's offset in the planes; odd: odd strips of the flux kinds march upwards;
// zmine / zpart: ZIP -- this wave's and its partner's S - 1 rows of LDS)
// (Tried on top of it, round 6: the three coefficient rings of a wave in LDS instead of accumulation registers -- a VALU instruction cannot
// read an accumulation register, so every level pays twelve v_accvgpr_read per row, a third of its non-arithmetic VALU work; from LDS
// they are three 16-byte reads.  3 983 -> 1 460 v_accvgpr_read in the eight-level kernel, 30 registers fewer, and SLOWER everywhere: 300 x
// 3600 424 -> 360 G, 1080 x 1440 457 -> 432 G, 1440 x 2880 617 -> 535 G -- one wave per SIMD has nothing to hide the LDS latency behind.
// Removed.)
template <bool ZIP> constexpr bool ringc_ramp_on(int t, int ph) { return ZIP ? (t == 1 ? ph >= 1 : ph >= t + 1) : ph >= 2 * t - 1; }

// ZIP, fold (wave-uniform, k_ringcz on the plan that owns the TRIPOLE SEAM): the strip starts at the grid's top row and its partner is the
// strip of the MIRROR window -- the northern neighbour of cell (rows - 1, i) is (rows - 1, nx - 1 - i) (reference kernels.py:33-40,
// 517-585) -- so the row the partner hands over is read with the lanes (and a lane's cells) reversed, level 1's seam flux comes from the
// partner's row of the input state as well (one more exchange), and the face coefficient is the top row's own north face (folded at plan
// time).  pos_at: the window's first column instead of wx * WI - M; [klo, khi): the columns this window keeps.
// PF: the launch carries one plane of mask bytes per batch entry (MultiP::mper, GCMF_MASK_FROM_NAN) -- an instantiation of k_ringc of its
// own (see k_ring, gcmf_ring_impl.hpp: the kernel of an ordinary launch is the code it was before).
// LV: a stacked plan (gcmf_plan_create_levels; the f64 flux kinds' plain strips) -- the coefficient planes and the land bytes have a level
// axis and batch entry b marches with the planes of level (P.lev0 + b) % P.nlev: one wave-uniform offset on row pointers that are scalar
// already, and, like PF, an instantiation of its own.
// XO (round 8: k_ringcz's table launches, whose window grid may start at any even column): `wx` is the window's first FOOTPRINT column x0
// instead of its number, and a lane owns its cells below column khi (the table's limit, nx + the grid's offset) instead of below nx -- a
// compile-time form of its own again: every other instantiation is the instruction stream it was.
// PB: a filter bank (gcmf_apply_bank; the f64 flux kinds' plain strips of an ordinary plan) -- batch entry e = P.ent0 + blockIdx.y is polynomial
// e / P.nfield applied to field e % P.nfield: the constant input comes from that field's plane, the state and result planes stay the entry's
// own, and the coefficients of the launch's levels come from row e / nfield of a table in device memory (MultiP::ptab) instead of from the
// kernel arguments -- wave-uniform addresses read once per march through the constant address space (scalar loads into scalar registers,
// where the kernel arguments' P.pk[] live too).  Like PF, LV and XO an instantiation of its own.
// PB and LV TOGETHER: a filter bank over per-field planes (gcmf_apply_bank_gaps) -- the launcher sets nlev = nfield and lev0 = ent0 % nfield,
// so LV's level (lev0 + blockIdx.y) % nlev = (ent0 + blockIdx.y) % nfield is PB's field index: entry e marches with row e / nfield of the table
// on the input plane, the coefficient planes and the land bytes of field e % nfield.  Both halves as they are; an instantiation of its own.
// NT (round 10; a table march only, nothing outside `if constexpr (XO)` reads it): the STATE planes are streamed -- the loads of b_{k+1} and
// b_{k+2} and the stores of the two new states carry the non-temporal policy (mload / mstore<NT>), because each of those bytes is written by
// one launch, read by the next and dead afterwards, while the four constant planes and the land bytes are read again by every launch: on a
// grid whose launch moves more than the memory-side cache holds, state lines that do not stay there leave the constants in it
// (experiments/mall_probe march; the policy is the host's, stream_state_ok in gcmf_wet_cut.hpp).  The constant input f, the coefficient
// planes and the land bytes keep the default policy; so does every access of the nan_to_num redo march.
template <typename T, int KIND, int S, bool FIRST, bool SANI, bool XE = false, bool ZIP = false, bool PF = false, bool LV = false, bool XO = false,
          bool PB = false, bool NT = false>
__device__ __forceinline__ bool ringc_march(const MultiP<T, T> &P, const int wx, const int a, const int b, const long long boff, const bool odd,
                                            T *zmine = nullptr, const T *zpart = nullptr, const bool fold = false, const int pos_at = 0,
                                            const int klo = -(1 << 30), const int khi = 1 << 30) {
  constexpr int VEC = 16 / sizeof(T);
  constexpr int W = 64 * VEC;
  constexpr int M = (S + VEC - 1) / VEC * VEC;
  constexpr int WI = W - 2 * M;
  constexpr int R = RingGeom::R, D = RingGeom::D, RU = RingGeom::RU, RV = RingGeom::RV;
  static_assert(R >= S + D && R % 3 == 0 && R % RU == 0 && R % RV == 0 && RU >= 3 + D && RV >= 1 + D, "ring periods");
  constexpr bool FLUX = (KIND == K_FLUX), MASK = (KIND == K_MASKZ);
  static_assert(!ZIP || FLUX, "the seam exchange is the flux kinds' (a carried face flux per level)");
  static_assert(!LV || (FLUX && !ZIP && !PF), "stacked plans: the flux kinds' plain strips");
  static_assert(!XO || ZIP, "a window origin per pair: k_ringcz's table launches");
  static_assert(!NT || (XO && !SANI && sizeof(T) == 8), "streamed state planes: the f64 table march, not its redo");
  static_assert(!PB || (FLUX && sizeof(T) == 8 && !ZIP && !XE && !PF), "filter banks: the f64 flux kinds' plain strips");
  constexpr bool WATCH = (KIND != K_REG) && !SANI;  // K_REG has no nan_to_num in the reference: NaN spreads by plain arithmetic
  constexpr bool FUSED = true;   // nothing here is bit-identical with numpy anyway: every multiply-add pair is one fma

  const int lane = threadIdx.x & 63;
  const int nx = P.nx, rows = P.rows;
  const int pos = (XO ? wx : (ZIP && fold) ? pos_at : wx * WI - M) + lane * VEC;
  int col_s = pos % nx;
  if (col_s < 0) col_s += nx;
  const unsigned col = (unsigned)col_s;
  const unsigned colT = col * (unsigned)sizeof(T);
  const bool keep = (lane * VEC >= M) && (lane * VEC < W - M) && (XO || pos < nx) && (!ZIP || (pos >= klo && pos < khi));
  const T c = (T)P.c;
  const bool last = P.last;

  T G0[RU][VEC];     // rows of b_{k+1} (the newer input state), slot = (row - r_begin) mod RU
  T G[S][3][VEC];    // G[t], t = 1..S-1: rows of level t, slot = (row - r_begin) mod 3
  T FN[S + 1][VEC];  // K_FLUX: carried north-face flux per level
  T cE[R][VEC], cN[R][VEC], ra[R][VEC];
  unsigned B[R];     // K_MASKZ: mask bytes
  T Ff[R][VEC];      // rows of the constant input f (prepared: * area, land -> 0), slot as the coefficient rows
  unsigned Zc[R];    // land bits of those rows
  T ARc[R][VEC];     // area of those rows (area-weighted types)
  T V[RV][VEC];      // rows of b_{k+2}
  unsigned Zu[RU];   // FIRST: land bits of the rows of f that become b_n (slots of G0)
  T ARu[RU][VEC];    // FIRST, area-weighted types: their area
  T cNs[VEC];        // ZIP: the seam face's coefficient
#pragma unroll
  for (int k = 0; k < VEC; ++k) cNs[k] = T(0);
#pragma unroll
  for (int t = 0; t < S; ++t) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) G[t][0][k] = G[t][1][k] = G[t][2][k] = FN[t + 1][k] = T(0);
  }
#pragma unroll
  for (int l = 0; l < RU; ++l) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) G0[l][k] = ARu[l][k] = T(0);
    Zu[l] = 0u;
  }
#pragma unroll
  for (int l = 0; l < R; ++l) {  // rings start at zero (see k_ring: the NaN watch also sees the levels of the first rows)
    B[l] = 0u;
    Zc[l] = 0u;
#pragma unroll
    for (int k = 0; k < VEC; ++k) cE[l][k] = cN[l][k] = ra[l][k] = Ff[l][k] = ARc[l][k] = T(0);
  }
#pragma unroll
  for (int l = 0; l < RV; ++l) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) V[l][k] = T(0);
  }

  const bool wrap = P.wrap;
  const int r_begin = ZIP ? a - 1 : a - S, r_last = b + S - 1;   // (ZIP: march row a - 1 is the partner's first row)
  // Odd strips of the flux kinds march UPWARDS (P.zigzag): the march below runs in "march order" m = r_begin - 1, r_begin, ... and
  // visits the grid row  mir - m  instead of m  (mir = a + b - 1 maps the strip and its ghost rows onto themselves).  Two strips that
  // share a boundary then reach it at the same time -- both at the start or both at the end of their marches -- so that the 2 S rows
  // each of them re-reads from the other's territory are found in the L2 / the memory-side cache instead of in HBM (same-direction
  // marches read them a whole march apart).  The arithmetic is the same instruction stream: "north" in march order is the grid's
  // south, the row of cN that travels with a centre row j is that of row j - 1, the carried flux is minus the grid's north flux, and
  // (fe - fw) + (fn - fs) is bit-for-bit symmetric under that exchange.
  const bool up = FLUX && (ZIP || P.zigzag) && odd;
  const int mir = a + b - 1;
  int cj, cj_prev;
  bool cout_, cout_prev;
  int cr = up ? mir - (r_begin - 1) : r_begin - 1;   // the cursor's grid row
  {
    const int r = cr;
    const bool lo = r < 0, hi = r >= rows;
    cj = wrap ? (r + (lo ? rows : 0) - (hi ? rows : 0)) : (lo ? 0 : (hi ? rows - 1 : r));
    cout_ = !wrap && (lo || hi);
    cj_prev = cj;
    cout_prev = cout_;
  }
  auto advance = [&]() {
    cj_prev = cj;
    cout_prev = cout_;
    if (!up) {
      ++cr;
      const int jn = cj + ((wrap || cr > 0) ? 1 : 0);
      const bool hit = (jn >= rows);
      cj = hit ? (wrap ? 0 : rows - 1) : jn;
    } else {
      --cr;
      const int jn = cj - ((wrap || cr < rows - 1) ? 1 : 0);
      const bool hit = (jn < 0);
      cj = hit ? (wrap ? rows - 1 : 0) : jn;
    }
    cout_ = !wrap && (cr < 0 || cr >= rows);
  };
  const T *fplane = P.fb_in + boff;  // the constant input f (Clenshaw has no fbar: the pointer slot is reused)
  T pbk[S + 1];   // PB: p_n (a first launch's) and the coefficients of levels 1 .. S, from the entry's row of the table
  if constexpr (PB) {   // (wave-uniform: blockIdx.y and kernel arguments only)
    typedef const __attribute__((address_space(4))) double *ctab_t;   // (nothing writes the table while a launch runs)
    const int ent = P.ent0 + (int)blockIdx.y;
    const int pol = ent / P.nfield;
    fplane = P.fb_in + (long long)(ent - pol * P.nfield) * P.bstride;
    const ctab_t row = (ctab_t)P.ptab + ((long long)pol * P.pstride + P.poff);
#pragma unroll
    for (int t = 0; t <= S; ++t) pbk[t] = (T)row[t];
  }
  const long long moff = (MASK && PF) ? boff : 0;   // (wave-uniform) the entry's own plane of mask bytes
  const long long loff = LV ? (long long)((P.lev0 + (int)blockIdx.y) % P.nlev) * P.lstride : 0;   // (wave-uniform) the entry's level
  const bool has_land = P.lbits != nullptr;
  const uint8_t *zbase = has_land ? P.lbits + moff : reinterpret_cast<const uint8_t *>(P.fb_in);  // (valid bytes, ignored)
  // (LV adds its offset in branches of its own, here and in load_centre: with the offset folded into the ordinary expressions --
  // "P.cE + loff" with loff = 0 -- the kernels of ordinary launches came out with another register allocation; this way they are the
  // instruction stream they were, compared in the assembly)
  if constexpr (LV) zbase = has_land ? P.lbits + loff : zbase;
  const bool weigh = !FLUX && P.area_weighted;
  const T *abase = weigh ? P.area : P.fb_in;  // (an unconditional load, ignored when there is no area)

  // XO (round 9): a table march keeps its rows as RUNNING BYTE OFFSETS inside a plane instead of row numbers.  xco is the cursor row's
  // offset, cj nx sizeof(T), a 32-bit scalar; it moves by xstep (one row, down or up the grid) and on reaching xlim (one row beyond the
  // grid's end on that side) becomes xreset, the other end: the table is taken on grids that wrap in y only, and only where
  // rows nx sizeof(T) < 2^32 (table_rows_ok, gcmf_wet_cut.hpp; the launcher asks).  A strip of a table starts inside the grid -- the
  // cursor's first row is mid - 2 or mid + 1 of a pair lo + 2 <= mid <= hi - 2 -- so this is the whole of advance().  A lane's address
  // is a wave-uniform plane base + ONE 32-bit offset per row, xvc (cursor) / xvp (the row before it, the centre row), shared by all
  // planes: the scalar-base form of the global loads and stores; the bases never change during a march.  The store rows trail the cursor
  // by a fixed number of phases and lie inside [a, b): one more running offset, xsu, no wrap.
  unsigned xco = 0u, xstep = 0u, xlim = 0u, xreset = 0u, xsu = 0u, xhv = 0u;
  unsigned xvc = 0u, xvp = 0u;
  const char *xbE = nullptr, *xbN = nullptr, *xbA = nullptr, *xbF = nullptr, *xbZ = nullptr, *xbU = nullptr, *xbV = nullptr;
  char *xbSu = nullptr, *xbSv = nullptr;
  T xtwo = T(2);
  if constexpr (XO) {
    const unsigned rowB = (unsigned)nx * (unsigned)sizeof(T);
    xstep = up ? 0u - rowB : rowB;
    xlim = up ? 0u - rowB : (unsigned)rows * rowB;
    xreset = up ? (unsigned)(rows - 1) * rowB : 0u;
    xco = (unsigned)cr * rowB;
    xvc = xco + colT;
    xvp = xvc;
    xbE = reinterpret_cast<const char *>(P.cE);
    xbN = reinterpret_cast<const char *>(P.cN);
    xbA = reinterpret_cast<const char *>(P.ra);
    xbF = reinterpret_cast<const char *>(fplane);
    xbZ = reinterpret_cast<const char *>(zbase);
    xbU = reinterpret_cast<const char *>(P.u0 + boff);
    xbV = reinterpret_cast<const char *>(P.v0 + boff);
    xbSu = reinterpret_cast<char *>((last ? P.fb_out : P.uo) + boff);
    xbSv = reinterpret_cast<char *>(P.vo + boff);
    const int m0 = r_begin - S;   // the first phase's store row in march order
    xsu = (unsigned)(up ? mir - m0 : m0) * rowB;   // (mod 2^32: exact whenever the row lies inside [a, b))
    xhv = last ? 0u : (unsigned)(b - a);   // (a last launch stores no second state)
    xtwo = last ? T(1) : T(2);
  }
  auto xadvance = [&]() {
    xvp = xvc;
    const unsigned t = xco + xstep;
    if (__builtin_expect(t == xlim, 0)) {
      xco = xreset;
    } else {
      xco = t;
    }
    xvc = xco + colT;
  };
  auto xat = [](auto *base, unsigned off) { return base + off; };   // (uniform base) + (zero-extended 32-bit lane offset)

  auto load_u = [&](auto slot_c) {  // the cursor's row of b_{k+1}; in a first launch that is b_n = p_n f, formed from the row of f
    constexpr int sl = decltype(slot_c)::value;
    if constexpr (XO) {
      if constexpr (!FIRST) {
        mload<T, VEC, NT>(G0[sl], reinterpret_cast<const T *>(xat(xbU, xvc)));
      } else {
        mload<T, VEC>(G0[sl], reinterpret_cast<const T *>(xat(xbF, xvc)));
        Zu[sl] = cell_bytes<VEC>(reinterpret_cast<const uint8_t *>(xat(xbZ, xvc / (unsigned)sizeof(T))));
      }
      return;
    }
    const long long rcur = (long long)(cj * nx);
    if constexpr (!FIRST) {
      mload<T, VEC>(G0[sl], lane_ptr(P.u0 + boff + rcur, colT));
    } else {
      mload<T, VEC>(G0[sl], lane_ptr(fplane + rcur, colT));
      Zu[sl] = cell_bytes<VEC>(lane_ptr(zbase + rcur, col));
      if constexpr (!FLUX) mload<T, VEC>(ARu[sl], lane_ptr(abase + rcur, colT));
    }
  };
  auto load_centre = [&](auto slot_c, auto vslot_c) {  // what travels with the row before it: b_{k+2}, f, coefficients / mask bits
    constexpr int sl = decltype(slot_c)::value;
    constexpr int vs = decltype(vslot_c)::value;
    if constexpr (XO) {
      // (the empty asm makes the offset a value of THIS basic block: with the zero-extension hoisted to the block of the phase before,
      // where the same offset served the cursor's loads, instruction selection takes a 64-bit vector add per load instead of the
      // scalar-base form)
      unsigned oc = xvp, on = up ? xvc : xvp;   // (an upward march: the cursor row's north face)
      asm("" : "+v"(oc));
      asm("" : "+v"(on));
      mload<T, VEC>(cE[sl], reinterpret_cast<const T *>(xat(xbE, oc)));
      mload<T, VEC>(cN[sl], reinterpret_cast<const T *>(xat(xbN, on)));
      mload<T, VEC>(ra[sl], reinterpret_cast<const T *>(xat(xbA, oc)));
      mload<T, VEC>(Ff[sl], reinterpret_cast<const T *>(xat(xbF, oc)));
      Zc[sl] = cell_bytes<VEC>(reinterpret_cast<const uint8_t *>(xat(xbZ, oc / (unsigned)sizeof(T))));
      if constexpr (!FIRST) mload<T, VEC, NT>(V[vs], reinterpret_cast<const T *>(xat(xbV, oc)));
      return;
    }
    const bool out_c = cout_prev;
    const long long rc = (long long)(cj_prev * nx);
    if constexpr (FLUX) {
      const T *pE = out_c ? P.zrow : P.cE + rc;
      // (an upward march: the face between the centre row and the row the cursor is on -- grid row j - 1's north face)
      const T *pN = !up ? (out_c ? P.zrow : P.cN + rc) : ((out_c || cout_) ? P.zrow : P.cN + (long long)(cj * nx));
      const T *pA = out_c ? P.zrow : P.ra + rc;
      if constexpr (LV) {   // (zrow has no level axis)
        pE = out_c ? pE : pE + loff;
        pN = (!up ? out_c : (out_c || cout_)) ? pN : pN + loff;
        pA = out_c ? pA : pA + loff;
      }
      mload<T, VEC>(cE[sl], lane_ptr(pE, colT));
      mload<T, VEC>(cN[sl], lane_ptr(pN, colT));
      mload<T, VEC>(ra[sl], lane_ptr(pA, colT));
    }
    if constexpr (MASK) {
      const uint8_t *mp = lane_ptr(out_c ? (const uint8_t *)P.zrow : P.mbits + moff + rc, col);
      B[sl] = cell_bytes<VEC>(mp);
    }
    mload<T, VEC>(Ff[sl], lane_ptr(fplane + rc, colT));
    Zc[sl] = cell_bytes<VEC>(lane_ptr(zbase + rc, col));
    if constexpr (!FLUX) mload<T, VEC>(ARc[sl], lane_ptr(abase + rc, colT));
    if constexpr (!FIRST) mload<T, VEC>(V[vs], lane_ptr(P.v0 + boff + rc, colT));  // a first launch: b_{n+1} = 0
  };

  bool bad = false;
  T out_v[VEC], out_u[VEC];

  auto level = [&](auto tt, auto ph_c) {
    constexpr int t = decltype(tt)::value;
    constexpr int ph = decltype(ph_c)::value;
    constexpr int sS = pmod(ph - t - 1, 3), sC = pmod(ph - t, 3), sN = pmod(ph - t + 1, 3);
    constexpr int sl = pmod(ph - t + 1, R);
    const T(&rS)[VEC] = (t == 1) ? G0[pmod(ph - 2, RU)] : G[t >= 2 ? t - 1 : 1][sS];
    const T(&rC)[VEC] = (t == 1) ? G0[pmod(ph - 1, RU)] : G[t >= 2 ? t - 1 : 1][sC];
    const T(&rN)[VEC] = (t == 1) ? G0[pmod(ph, RU)] : G[t >= 2 ? t - 1 : 1][sN];
    // what the stencil sees: its operands through nan_to_num in the redo pass (kernels.py:175, 300), as they are otherwise
    T gS[VEC], gC[VEC], gN[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      gS[k] = SANI ? msan(rS[k]) : rS[k];
      gC[k] = SANI ? msan(rC[k]) : rC[k];
      gN[k] = SANI ? msan(rN[k]) : rN[k];
    }
    const T ev = from_upper_lane0(gC[0]);
    T fev[VEC], few = T(0), wv = T(0);
    if constexpr (FLUX) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const T xE = (k == VEC - 1) ? ev : gC[k < VEC - 1 ? k + 1 : k];
        fev[k] = (xE - gC[k]) * cE[sl][k];
      }
      few = from_lower_lane0(fev[VEC - 1]);
    } else {
      wv = from_lower_lane0(gC[VEC - 1]);
    }
    // the last level of the last launch is the result  p_0 f + A(b_1) - b_2: A, not 2 A
    T two;
    if constexpr (XO) two = (t == S) ? xtwo : T(2);   // (chosen once per march)
    else two = (last && t == S) ? T(1) : T(2);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const T xC = gC[k];
      T L;
      if constexpr (FLUX) {
        const T fe = fev[k];
        const T fw = (k == 0) ? few : fev[k > 0 ? k - 1 : 0];
        const T fn = (gN[k] - xC) * cN[sl][k];
        L = ((fe - fw) + (fn - FN[t][k])) * ra[sl][k];
        FN[t][k] = fn;
      } else {
        const T xW = (k == 0) ? wv : gC[k > 0 ? k - 1 : 0];
        const T xE = (k == VEC - 1) ? ev : gC[k < VEC - 1 ? k + 1 : k];
        if constexpr (MASK) {
          const unsigned bb = (B[sl] >> (8 * k)) & 0xFFu;
          const T wf = (T)(bb >> 5);
          L = rfma(-wf, xC, xE);
          L = L + xW;
          L = L + gN[k];
          L = L + gS[k];
          L = (bb & 1u) ? L : T(0);
        } else {
          L = rfma(T(-4), xC, xE);
          L = L + xW;
          L = L + gN[k];
          L = L + gS[k];
        }
      }
      const T av = cheb_a<FUSED>(rC[k], c, L);  // "-x" takes the raw value: a NaN stays in its cell (filter.py:166-175)
      const T x2 = (t == 1) ? V[ph % RV][k] : (t == 2 ? G0[pmod(ph - 2, RU)][k] : G[t >= 3 ? t - 2 : 1][sC][k]);
      T tk;
      if (FUSED) {
        tk = rfma(two, av, -x2);
        if constexpr (PB) tk = rfma(pbk[t], Ff[sl][k], tk);
        else tk = rfma((T)P.pk[t - 1], Ff[sl][k], tk);
      } else {
        tk = two * av - x2;
        tk = tk + (T)P.pk[t - 1] * Ff[sl][k];
      }
      if (t < S) G[t < S ? t : 0][sC][k] = tk;
      if (t == S - 1) out_v[k] = tk;
      if (t == S) {
        out_u[k] = tk;
        if (WATCH) bad = bad || !(mabs(tk) <= MLim<T>::big());
      }
    }
  };

  auto phase = [&](auto ph_c, int r, auto pro_c) {
    constexpr int ph = decltype(ph_c)::value;
    // the strip's first period: level t starts with phase 2 t - 1 (below).  Flux kinds only: the land-mask / REGULAR kernels lose 3-4 % at
    // full size with the peeled period (config 2: 82 -> 85 us per launch on one box) and gain 3 % on 1/4-degree grids.
    constexpr bool PRO = decltype(pro_c)::value && FLUX;
    if constexpr (XO) xadvance();
    else advance();
    load_centre(ic<(ph + D) % R>{}, ic<(ph + D) % RV>{});
    load_u(ic<(ph + D) % RU>{});
    if constexpr (FIRST) {  // the row of f that has just arrived becomes a row of b_n = p_n f (prepared, land out)
      constexpr int su = ph % RU;
      T pn = (T)P.p0;
      if constexpr (PB) pn = pbk[0];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (!FLUX) G0[su][k] = weigh ? G0[su][k] * ARu[su][k] : G0[su][k];
        if constexpr (XO) G0[su][k] = ((Zu[su] >> (8 * k)) & 1u) ? pn * G0[su][k] : T(0);   // (a table is cut from the land bytes: there are some)
        else G0[su][k] = (!has_land || ((Zu[su] >> (8 * k)) & 1u)) ? pn * G0[su][k] : T(0);
      }
    }
    {  // the f row level 1 uses now: prepare() and land out (once per row; the later levels find it that way in the ring)
      constexpr int s1 = ph % R;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (!FLUX) Ff[s1][k] = weigh ? Ff[s1][k] * ARc[s1][k] : Ff[s1][k];
        if constexpr (XO) Ff[s1][k] = ((Zc[s1] >> (8 * k)) & 1u) ? Ff[s1][k] : T(0);
        else Ff[s1][k] = (!has_land || ((Zc[s1] >> (8 * k)) & 1u)) ? Ff[s1][k] : T(0);
      }
    }
    // The ramp: phase q of a strip (q = 0 at row r_begin = a - S) produces row a - S + q - t of level t, and the strip needs level t from
    // row a - (S - t) on -- phase 2 t.  One phase earlier the level has to run for the flux it carries to its next row (its value there
    // is never used); before that it would compute rows nobody reads.  S^2 of the (H + 2 S) S level-rows of a strip: 8 % at 80 rows, a
    // quarter of the instruction stream of a 12-row strip (8-way slabs, 1/4-degree grids).
    // ZIP: the strip starts AT the seam (q = 0 at march row a - 1, the partner's first row): level 1 runs from phase 1 (for the seam face's
    // flux, out of its own two rows), level t >= 2 from phase t + 1 -- its first row, with the seam face's flux from the exchange below.
    if constexpr (ZIP && PRO && ph == 1) {
      if (fold) mload<T, VEC>(cNs, lane_ptr(P.cN + (long long)(rows - 1) * nx, colT));   // the top row's north face: the fold
      else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) cNs[k] = cN[1][k];   // (the coefficient row of march row a - 1: its face towards row a)
      }
    }
    if constexpr (!PRO || ringc_ramp_on<ZIP>(1, ph)) level(ic<1>{}, ph_c);
    if constexpr (S >= 2 && (!PRO || ringc_ramp_on<ZIP>(2, ph))) level(ic<2>{}, ph_c);
    if constexpr (S >= 3 && (!PRO || ringc_ramp_on<ZIP>(3, ph))) level(ic<3>{}, ph_c);
    if constexpr (S >= 4 && (!PRO || ringc_ramp_on<ZIP>(4, ph))) level(ic<4>{}, ph_c);
    if constexpr (S >= 5 && (!PRO || ringc_ramp_on<ZIP>(5, ph))) level(ic<5>{}, ph_c);
    if constexpr (S >= 6 && (!PRO || ringc_ramp_on<ZIP>(6, ph))) level(ic<6>{}, ph_c);
    if constexpr (S >= 7 && (!PRO || ringc_ramp_on<ZIP>(7, ph))) level(ic<7>{}, ph_c);
    if constexpr (S >= 8 && (!PRO || ringc_ramp_on<ZIP>(8, ph))) level(ic<8>{}, ph_c);
    if constexpr (S >= 9 && (!PRO || ringc_ramp_on<ZIP>(9, ph))) level(ic<9>{}, ph_c);
    if constexpr (ZIP && PRO && ph == 1) {
      // (launch-uniform: in a launch with fold strips EVERY workgroup meets at this barrier -- pairs and fold strips share workgroups)
      if (P.fold_rows > 0 && !fold) __syncthreads();
      if (fold) {   // level 1's seam flux: the partner's top row of the input state (slot 1 of the ring of b_{k+1}; a first launch has just formed it)
        T own[VEC], oth[VEC], rev[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) own[k] = G0[1][k];
        mstore<T, VEC>(zmine + (S - 1) * W + lane * VEC, own);
        __syncthreads();
        mload<T, VEC>(rev, zpart + (S - 1) * W + (63 - lane) * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) oth[k] = rev[VEC - 1 - k];
#pragma unroll
        for (int k = 0; k < VEC; ++k) FN[1][k] = ((SANI ? msan(own[k]) : own[k]) - (SANI ? msan(oth[k]) : oth[k])) * cNs[k];
      }
    }
    if constexpr (ZIP && PRO && ph >= 2 && ph <= S) {
      // level ph - 1 has just produced the strip's first row (slot 1 of its ring): the partner's level ph needs it for the flux across the
      // seam, this wave's level ph needs the partner's -- what the march row before the first one would have left in FN[ph]
      constexpr int t = ph - 1;
      T own[VEC], oth[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) own[k] = G[t < S ? t : 1][1][k];
      mstore<T, VEC>(zmine + (t - 1) * W + lane * VEC, own);
      __syncthreads();
      {
        T got[VEC];
        mload<T, VEC>(got, zpart + (t - 1) * W + (fold ? 63 - lane : lane) * VEC);
#pragma unroll
        for (int k = 0; k < VEC; ++k) oth[k] = fold ? got[VEC - 1 - k] : got[k];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) FN[t + 1][k] = ((SANI ? msan(own[k]) : own[k]) - (SANI ? msan(oth[k]) : oth[k])) * cNs[k];
    }
    if constexpr (XO) {   // (f64 flux kinds: no finalize(), no f64 copy of an f32 state)
      const unsigned q = (unsigned)(r - S - a);   // the store row in march order, from a: the mirror maps [a, b) onto itself
      if (q < (unsigned)(b - a)) {  // wave-uniform
        if (keep) mstore<T, VEC, NT>(reinterpret_cast<T *>(xat(xbSu, xsu + colT)), out_u);
      }
      if (q + 1u < xhv) {
        if (keep) mstore<T, VEC, NT>(reinterpret_cast<T *>(xat(xbSv, xsu + xstep + colT)), out_v);
      }
      xsu += xstep;
      return;
    }
    const int ju = up ? mir - (r - S) : r - S;
    if (ju >= a && ju < b) {  // wave-uniform
      const long long off = boff + (long long)ju * nx;
      if (keep) {
        if (!last) {
          mstore<T, VEC>(lane_ptr(P.uo + off, colT), out_u);
        } else {
          if (!FLUX && P.area_weighted) {  // finalize(): / area (kernels.py:103-104)
            T ar[VEC];
            mload<T, VEC>(ar, lane_ptr(P.area + (long long)ju * nx, colT));
#pragma unroll
            for (int k = 0; k < VEC; ++k) out_u[k] = out_u[k] / ar[k];
          }
          if (P.d_out) {   // (wave-uniform) f32 state, f64 result: NumPy >= 2 promotes p[k] * T
            double dd[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) dd[k] = (double)out_u[k];
            mstore<double, VEC>(lane_ptr(P.d_out + off, 2 * colT), dd);
          } else {
            mstore<T, VEC>(lane_ptr(P.fb_out + off, colT), out_u);
          }
        }
      }
    }
    const int jv = up ? mir - (r - S + 1) : r - S + 1;
    if (!last && jv >= a && jv < b) {
      T *rowp = P.vo + boff + (long long)jv * nx;
      if (keep) mstore<T, VEC>(lane_ptr(rowp, colT), out_v);
    }
  };

  if constexpr (XO) xadvance();
  else advance();
  load_centre(ic<0>{}, ic<0>{});
  load_u(ic<0>{});
  if constexpr (XO) xadvance();
  else advance();
  load_centre(ic<1>{}, ic<1>{});
  load_u(ic<1>{});
  if constexpr (XO) xadvance();
  else advance();
  load_centre(ic<2>{}, ic<2>{});
  load_u(ic<2>{});
  static_assert(D == 3, "prologue");
  // The flux kinds march whole periods: every early exit costs this kernel dozens of registers (146 -> 204 AGPRs with an exit
  // every four rows), and on tripolar plans k_fold_band's waves have to fit on the SIMDs NEXT to these (gcmf_foldband.hip).
  constexpr bool EARLY = (KIND != K_FLUX) || XE;
  // k_ringcz: an exit every second row.  Nine levels: 52 bytes of scratch that way; a second form with its exits after rows 2, 6, 10 instead of
  // 4, 8, 12 (for strips whose march is 4 k + 2 rows) fits (506 registers) but runs 7 % longer per row -- 1080 x 1440: 26 rows in 34.4 us
  // against 28 rows in 32.5 us -- and was dropped.
  constexpr bool XE2 = ZIP && XE && S <= 8;
  if constexpr (FLUX) {  // the first period, peeled: the ramp of the levels
    constexpr std::integral_constant<bool, true> pro{};
    phase(ic<0>{}, r_begin, pro);
    phase(ic<1>{}, r_begin + 1, pro);
    phase(ic<2>{}, r_begin + 2, pro);
    phase(ic<3>{}, r_begin + 3, pro);
    phase(ic<4>{}, r_begin + 4, pro);
    phase(ic<5>{}, r_begin + 5, pro);
    phase(ic<6>{}, r_begin + 6, pro);
    phase(ic<7>{}, r_begin + 7, pro);
    phase(ic<8>{}, r_begin + 8, pro);
    phase(ic<9>{}, r_begin + 9, pro);
    phase(ic<10>{}, r_begin + 10, pro);
    phase(ic<11>{}, r_begin + 11, pro);
    if (WATCH && __any(bad)) return true;
    if (r_begin + 11 >= r_last) return false;   // (a last strip of one or two rows at S = 5)
  }
  constexpr std::integral_constant<bool, false> run{};
  for (int r0 = FLUX ? r_begin + R : r_begin;; r0 += R) {
    bool done = true;
    do {
      phase(ic<0>{}, r0, run);
      phase(ic<1>{}, r0 + 1, run);
      if (XE2 && r0 + 1 >= r_last) break;
      phase(ic<2>{}, r0 + 2, run);
      phase(ic<3>{}, r0 + 3, run);
      if (EARLY && r0 + 3 >= r_last) break;     // (the last period is left after the strip's last row, see k_ring)
      phase(ic<4>{}, r0 + 4, run);
      phase(ic<5>{}, r0 + 5, run);
      if (XE2 && r0 + 5 >= r_last) break;
      phase(ic<6>{}, r0 + 6, run);
      phase(ic<7>{}, r0 + 7, run);
      if (EARLY && r0 + 7 >= r_last) break;
      phase(ic<8>{}, r0 + 8, run);
      phase(ic<9>{}, r0 + 9, run);
      if (XE2 && r0 + 9 >= r_last) break;
      phase(ic<10>{}, r0 + 10, run);
      phase(ic<11>{}, r0 + 11, run);
      done = (r0 + 11 >= r_last);
    } while (false);
    if (WATCH && __any(bad)) return true;
    if (done) break;
  }
  return false;
}

// What wave `wid` of a launch marches.  gridDim.y = the batch (P.npack == 0): the strip st = wid / nwx of field blockIdx.y.  Packed batches
// (P.npack > 0, round 6): the fields of the batch are ONE column of npack * nrows rows per window, cut into runs of P.H rows; a wave walks
// its run, which crosses at most one field boundary (H <= nrows): up to two (field, row range) segments, each a march of its own with its
// 2 S warm-up rows.  16 fields x 33 windows of a 300-row slab tile 1024 wave slots at ~70 % as whole strips (a strip cannot cross from one
// field into the next) and at ~95 % this way.
template <typename T, int KIND, int S, bool FIRST, bool XE, bool PACK, bool PF = false, bool LV = false, bool PB = false>   // (PF, LV, PB: never packed, ringc_cut)
__device__ __forceinline__ void ringc_walk(const MultiP<T, T> &P, const int wid) {
  const int wx = wid % P.nwx, st = wid / P.nwx;
  if constexpr (!PACK) {   // one strip of one field (the instruction stream of rounds 2-5: the walk below costs the land-mask kernel 5 %)
    const int a = P.out_lo + st * P.H;
    const int b = min(a + P.H, P.out_hi);
    const long long boff = (long long)blockIdx.y * P.bstride;
    if (ringc_march<T, KIND, S, FIRST, false, XE, false, PF, LV, false, PB>(P, wx, a, b, boff, (st & 1) != 0)) {
      if constexpr (KIND != K_REG) {
        if (P.nfb && (threadIdx.x & 63) == 0) atomicAdd(P.nfb, 1u);                      // instrumentation: gcmf_ring_fallbacks
        ringc_march<T, KIND, S, FIRST, true, XE, false, PF, LV, false, PB>(P, wx, a, b, boff, (st & 1) != 0);   // the same strip again, operands through nan_to_num
      }
    }
    return;
  }
  const int nrows = P.out_hi - P.out_lo;
  int v0 = st * P.H;   // (rows of the batch's column: the launcher keeps batch x rows below 2^30)
  const int v1 = min(v0 + P.H, P.npack * nrows);
  while (v0 < v1) {   // (wave-uniform: scalar registers)
    const int fld = v0 / nrows, r = v0 - fld * nrows;
    const int len = min(v1 - v0, nrows - r);
    const int a = P.out_lo + r, b = a + len;
    const long long boff = (long long)fld * P.bstride;
    if (ringc_march<T, KIND, S, FIRST, false, XE>(P, wx, a, b, boff, (st & 1) != 0)) {
      if constexpr (KIND != K_REG) {
        if (P.nfb && (threadIdx.x & 63) == 0) atomicAdd(P.nfb, 1u);
        ringc_march<T, KIND, S, FIRST, true, XE>(P, wx, a, b, boff, (st & 1) != 0);
      }
    }
    v0 += len;
  }
}

// PF and LV TOGETHER (neither means anything beside the other: a plane of mask bytes per entry is the land-mask kinds', a level axis the flux
// kinds') name the filter bank's form, ringc_march<PB>: the kernel keeps its six template arguments, and with them the names of all its
// other instantiations
// PF ALONE on the flux kinds (which have no mask bytes) names the bank over per-field planes, ringc_march<PB, LV> (gcmf_apply_bank_gaps)
template <typename T, int KIND, int S, bool FIRST, bool PF = false, bool LV = false>
__global__ __launch_bounds__(256, 1) void k_ringc(const MultiP<T, T> P) {
  int bx = blockIdx.x;
  if (P.xcd_per > 0 && bx < 8 * P.xcd_per) bx = (bx & 7) * P.xcd_per + (bx >> 3);
  const int wid = bx * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= P.nwaves) return;
  constexpr bool PBL = (KIND == K_FLUX) && PF && !LV;
  constexpr bool PB = (PF && LV) || PBL;
  ringc_walk<T, KIND, S, FIRST, false, false, PF && !PB, (LV && !PB) || PBL, PB>(P, wid);
}

// ... and for packed batches (ringc_walk<PACK>): XE = the early-exit form of the flux kinds (k_ringcs)
template <typename T, int KIND, int S, bool FIRST, bool XE>
__global__ __launch_bounds__(256, 1) void k_ringcp(const MultiP<T, T> P) {
  int bx = blockIdx.x;
  if (P.xcd_per > 0 && bx < 8 * P.xcd_per) bx = (bx & 7) * P.xcd_per + (bx >> 3);
  const int wid = bx * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= P.nwaves) return;
  ringc_walk<T, KIND, S, FIRST, XE, true>(P, wid);
}

// The flux kinds with early exits: for ROW SLABS that own no tripole seam (the ranks of a multi-GPU run, the row blocks of the host
// pipeline).  Their strips are short -- 300 rows of an 8-way slab: 11 + 2 S rows per strip -- so rows up to the next whole ring period
// are a third of the march, and nothing has to fit beside these waves (the extra ~60 registers of the exits are free here).
template <typename T, int S, bool FIRST>
__global__ __launch_bounds__(256, 1) void k_ringcs(const MultiP<T, T> P) {
  int bx = blockIdx.x;
  if (P.xcd_per > 0 && bx < 8 * P.xcd_per) bx = (bx & 7) * P.xcd_per + (bx >> 3);
  const int wid = bx * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= P.nwaves) return;
  ringc_walk<T, K_FLUX, S, FIRST, true, false>(P, wid);
}

// k_ringcz: strips ZIPPED in pairs at a shared seam (ringc_march<ZIP>), early exits: mid-size whole grids and row slabs of the f64 flux kinds
// without a tripole seam, where a strip is as short as its ghost zones.  The rows [out_lo, out_hi) of a window are cut into P.nstrips / 2
// pairs of (almost) equal height; a pair is cut in the middle: the lower strip marches down the grid from the cut, the upper one up.  A
// workgroup = the two pairs of two neighbouring windows (pair (2 bx + w / 2), member w % 2); a pair past the end idles through the barriers.
// A non-finite value met by ANY wave of the workgroup sends all four through the nan_to_num march (they meet at its barriers).
// TAB (round 7): the pairs come from the launch's table (MultiP::utab: strips cut from the rows of each window that hold anything wet,
// wet_table in gcmf_ringc_zip.hip) -- a kernel of its own, k_ringcz<T, S, FIRST, XE, true>: as a wave-uniform branch inside the one kernel
// the table cost the ordinary launch 3-4 % (these marches are paced by their instruction stream, see PF above and DESIGN.md 6).
// Round 8: a pair's first int is its window's first footprint column x0 (ringc_march<XO>), so that the window grid of a table may start at
// any even column; the column limit of ownership travels in MultiP::nfw, which a table launch (no fold strips) has no other use for.
// NT (round 10): a table launch that streams its state planes (ringc_march<NT>) -- a kernel of its own again, k_ringcz<T, S, FIRST, XE, true, true>;
// the redo march is the one every table launch has.
template <typename T, int S, bool FIRST, bool XE, bool TAB, bool NT = false>
__device__ __forceinline__ void ringcz_body(const MultiP<T, T> &P, T (*zl)[S * 64 * (16 / sizeof(T))]) {
  constexpr int VEC = 16 / sizeof(T), W = 64 * VEC, M = (S + VEC - 1) / VEC * VEC, WI = W - 2 * M;
  int bx = blockIdx.x;
  if (P.xcd_per > 0 && bx < 8 * P.xcd_per) bx = (bx & 7) * P.xcd_per + (bx >> 3);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int np = P.nstrips >> 1, nnorm = P.nwx * np;
  const int unit = bx * 2 + (w >> 1);   // a pair of waves: a pair of strips, or (after the pairs) a window of the top rows and its mirror image
  const bool fold = !TAB && unit >= nnorm;
  const long long boff = (long long)blockIdx.y * P.bstride;
  const bool upper = (w & 1) != 0;
  bool active, odd;
  int wx = 0, a, b, pos_at = 0, klo = -(1 << 30), khi = 1 << 30;
  if (TAB) {
    active = unit < P.nunits;
    const int4 e = P.utab[active ? unit : 0];   // (wave-uniform: scalar loads)
    wx = e.x;        // (x0)
    khi = P.nfw;     // (the table's column limit)
    a = upper ? e.z : e.y;
    b = upper ? e.w : e.z;
    odd = !upper;
  } else if (!fold) {
    const int pid = unit;
    active = true;
    wx = pid % P.nwx;
    const int pp = pid / P.nwx;
    const long long nrows = P.out_hi - P.fold_rows - P.out_lo;
    const int lo = P.out_lo + (int)((long long)pp * nrows / np), hi = P.out_lo + (int)((long long)(pp + 1) * nrows / np), mid = lo + (hi - lo) / 2;
    a = upper ? mid : lo;
    b = upper ? hi : mid;
    odd = !upper;
  } else {   // a window of the western half (even wave) and its mirror image (odd wave), both marching down the grid from the seam
    const int fid = unit - nnorm;
    active = fid < P.nfw;
    a = P.out_hi - P.fold_rows;
    b = P.out_hi;
    odd = true;
    const int pw = fid * WI - M;
    pos_at = upper ? P.nx - pw - W : pw;
    klo = upper ? P.nx / 2 : 0;
    khi = upper ? P.nx : P.nx / 2;
  }
  const int nbar = P.fold_rows > 0 ? S : S - 1;   // (barriers of a march: one more in a launch with fold strips)
  bool bad = false;
  if (active) bad = ringc_march<T, K_FLUX, S, FIRST, false, XE, true, false, false, TAB, false, NT>(P, wx, a, b, boff, odd, zl[w], zl[w ^ 1], fold, pos_at, klo, khi);
  else
    for (int k = 0; k < nbar; ++k) __syncthreads();
  if (__syncthreads_or(bad ? 1 : 0)) {
    if (active) {
      if (P.nfb && (threadIdx.x & 63) == 0) atomicAdd(P.nfb, 1u);
      ringc_march<T, K_FLUX, S, FIRST, true, XE, true, false, false, TAB>(P, wx, a, b, boff, odd, zl[w], zl[w ^ 1], fold, pos_at, klo, khi);
    } else {
      for (int k = 0; k < nbar; ++k) __syncthreads();
    }
  }
}
template <typename T, int S, bool FIRST, bool XE>
__global__ __launch_bounds__(256, 1) void k_ringcz(const MultiP<T, T> P) {
  __shared__ __attribute__((aligned(16))) T zl[4][S * 64 * (16 / sizeof(T))];   // (row S - 1: the fold strips' exchange of the input state)
  ringcz_body<T, S, FIRST, XE, false>(P, zl);
}
template <typename T, int S, bool FIRST, bool XE, bool TAB>
__global__ __launch_bounds__(256, 1) void k_ringcz(const MultiP<T, T> P) {
  static_assert(TAB, "the even cut is k_ringcz<T, S, FIRST, XE>");
  __shared__ __attribute__((aligned(16))) T zl[4][S * 64 * (16 / sizeof(T))];
  ringcz_body<T, S, FIRST, XE, true>(P, zl);
}
template <typename T, int S, bool FIRST, bool XE, bool TAB, bool NT>
__global__ __launch_bounds__(256, 1) void k_ringcz(const MultiP<T, T> P) {
  static_assert(TAB && NT, "the table launch that streams its state planes");
  __shared__ __attribute__((aligned(16))) T zl[4][S * 64 * (16 / sizeof(T))];
  ringcz_body<T, S, FIRST, XE, true, true>(P, zl);
}

// What every backward scalar launch passes to its kernel: the caller's planes, the plan's coefficient planes, and the cut (ringc_cut,
// gcmf_ringc_cut.hpp) -- nothing about the geometry is worked out here
template <typename T> static void ringc_params(MultiP<T, T> &P, const gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &c) {
  const Geom g = view_geom(pl, cv);
  P.u0 = (const T *)a.u0;
  P.v0 = (const T *)a.v0;
  P.uo = (T *)a.uo;
  P.vo = (T *)a.vo;
  P.fb_in = (const T *)a.fb_in;   // the constant input f
  P.fb_out = (T *)a.fb_out;       // the result (last launch)
  P.d_out = nullptr;
  if (sizeof(T) == 4 && !a.fb_is_f32) {   // f32 state: the result is f64 unless the caller asked for f32 (GCMF_OUT_F32)
    P.d_out = (double *)a.fb_out;
    P.fb_out = nullptr;
  }
  P.cE = (const T *)g.coef[0];
  P.cN = (const T *)g.coef[1];
  P.ra = (const T *)g.coef[2];
  P.zrow = (const T *)pl->zero_row;
  P.nfb = pl->ring_nfb;
  P.mbits = g.mbits;
  P.lbits = (cv.n_land > 0) ? cv.lbits : nullptr;
  P.mper = cv.mask_per_field;
  P.lstride = cv.stacked ? (long long)g.rows * g.nx : 0;
  P.nlev = (int)cv.nlev;
  P.lev0 = (int)(cv.entry0 % cv.nlev);
  P.area = (const T *)g.area;
  P.nx = g.nx;
  P.rows = g.rows;
  P.out_lo = a.row_lo;
  P.out_hi = a.row_hi;
  P.nwx = c.nwx;
  P.H = c.H;
  P.nstrips = c.nstrips;
  P.npack = c.npack;
  P.fold_rows = c.fold_rows;
  P.nfw = c.nfw;
  P.nwaves = c.nwx * c.nstrips;
  P.wrap = g.south_wrap && g.north_wrap;
  P.first = a.first ? 1 : 0;
  P.last = a.last;
  P.area_weighted = (pl->kind == K_FLUX) ? 0 : g.area_weighted;
  P.bstride = (long long)g.rows * g.nx;
  for (int t = 0; t < MAX_PK; ++t) P.pk[t] = t < a.S ? a.pk[t] : 0.0;
  P.p0 = a.p0;
  P.c = a.c;
  P.xcd_per = pl->xcd_remap ? (int)(c.grid_x / 8) : 0;
  P.zigzag = pl->zigzag;   // (k_ringcz's pairs always march away from each other)
}

template <typename T, int S, bool FIRST>
int launch_ringc_zip_sf(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  const int nrows = a.row_hi - a.row_lo;
  const bool folds = cut.form == RINGC_ZIP_FOLD;
  if (cut.pairs < 1 || nrows - cut.fold_rows < 2 * cut.pairs) {
    set_error("k_ringcz: %d rows cannot be cut into pairs of strips", nrows);
    return GCMF_ERR_INVALID_ARG;
  }
  // (round 7) whole grids with land, a lone field: the pairs cut from the rows of each window that hold anything wet -- the wave slots
  // of all-land tiles go to the wet part, and every strip gets shorter (wet_table, gcmf_ringc_zip.hip)
  const WetTable *tab = nullptr;
  // (round 9: the table march addresses a plane with 32-bit byte offsets and knows no closed end -- a plane of 4 GiB or more, or a grid
  // that does not wrap in y, keeps the even cut)
  if (sizeof(T) == 8 && cv.wet_now && !folds && table_rows_ok(pl->g.rows, pl->g.nx, (long long)sizeof(T), pl->g.south_wrap && pl->g.north_wrap)) {
    int rc = GCMF_OK;
    tab = wet_table(pl, cv, a, cut.march, s, &rc);
    if (rc) return rc;
    if (tab && !pl->pool_clean) {   // cells no pair owns are read as ghost cells: they must be finite (gcmf_plan::pool_clean)
      if (FIRST) {                  // (a first launch reads no state: nothing the fill could destroy)
        GCMF_HIP(hipMemsetAsync(pl->pool_base, 0, pl->pool_bytes, s));
        pl->pool_clean = true;
      } else {
        // A later launch of an application whose FIRST launch took no table (the policy refused that depth, or another kernel ran it):
        // the planes hold live state, so no fill, and this launch keeps the even cut -- as will the later launches of every such
        // application, silently (option 2 never gets here: every launch of an eligible call takes its table, the first one too).
        // clenshaw_cut puts the deepest launches first; where the policy of option 1 refuses those and would take a shallower
        // later one, that one is lost.
        tab = nullptr;
      }
    }
  }
  RingcCut c = cut;
  if (tab) {   // the table's strips instead of the even cut's
    c.nstrips = tab->nstrips;
    c.H = tab->H;
    c.grid_x = (unsigned)((tab->nunits + 1) / 2);
    c.xe = ringc_zip_exits(tab->H, S, pl->ringc_zip);
  }
  MultiP<T, T> P;
  ringc_params(P, pl, cv, a, c);
  if (tab) {
    P.utab = (const int4 *)tab->dev;
    P.nunits = tab->nunits;
    P.nfw = tab->xlim;   // (no fold strips in a table launch: the field carries the column limit of ownership, ringcz_body)
  }
  const bool xe = c.xe;
  dim3 block(256), grid(c.grid_x, c.grid_y);
  // (round 10) nine levels from a table: the state planes streamed where the launch moves more than the memory-side cache holds (option
  // "stream_state": 0 never, 1 by stream_state_ok, 2 whenever such a launch runs) -- same arithmetic, same bits
  constexpr bool STREAMS = S == 9 && sizeof(T) == 8;
  const bool nt = STREAMS && tab && grid.x > 0 && (pl->stream_state >= 2 || (pl->stream_state == 1 && stream_state_ok(tab->cells)));
  if (tab) {
    if constexpr (sizeof(T) == 8) {   // (f64 only: wet_table)
      if (grid.x > 0) {   // (a grid that is all land has no pair: k_land_fix writes the whole result)
        if constexpr (STREAMS) {   // (nt is false at every other depth)
          if (nt && xe) hipLaunchKernelGGL((k_ringcz<T, S, FIRST, true, true, true>), grid, block, 0, s, P);
          if (nt && !xe) hipLaunchKernelGGL((k_ringcz<T, S, FIRST, false, true, true>), grid, block, 0, s, P);
        }
        if (!nt && xe) hipLaunchKernelGGL((k_ringcz<T, S, FIRST, true, true>), grid, block, 0, s, P);
        if (!nt && !xe) hipLaunchKernelGGL((k_ringcz<T, S, FIRST, false, true>), grid, block, 0, s, P);
      }
    }
  } else if (xe) {
    hipLaunchKernelGGL((k_ringcz<T, S, FIRST, true>), grid, block, 0, s, P);
  } else {
    hipLaunchKernelGGL((k_ringcz<T, S, FIRST, false>), grid, block, 0, s, P);
  }
  GCMF_HIP(hipGetLastError());
  note_kernel(pl, tab ? kernel_name("k_ringcz", {tyname<T>(), S, FIRST, xe, true}) : kernel_name("k_ringcz", {tyname<T>(), S, FIRST, xe}), S,
              launch_geom(P.H, P.nstrips, P.nwx, P.xcd_per > 0, grid.x, grid.y, nrows) + (tab ? " units=" + std::to_string(tab->nunits) + (tab->tight ? " xoff=" + std::to_string(tab->xlim - P.nx) : std::string()) + (nt ? " nt=1" : "") : std::string()));
  return GCMF_OK;
}

// k_ringc / k_ringcs (XE) on whole strips, k_ringcp on a packed batch: as the cut says.
// PF / LV: the per-entry forms of k_ringc<double, K_FLUX, ...>, which take the same two booleans -- always the plain strips (ringc_cut),
// reported under the ordinary kernel's name (as the land-mask kinds' per-entry-mask instantiation is) with the form behind the geometry:
//   LV      a stacked plan (gcmf_plan_create_levels): " levels=<nlev>"
//   PF, LV  a filter bank (gcmf_apply_bank): " bank=<nbank>"
//   PF      a filter bank over per-field planes (gcmf_apply_bank_gaps: the view is stacked, one level per field): " levels=<nfield> bank=<nbank>"
template <typename T, int KIND, int S, bool FIRST, bool XE, bool PF, bool LV>
int launch_ringc_sf(gcmf_plan *pl, const CallView &cv, const MultiArgs &a, const RingcCut &cut, hipStream_t s) {
  constexpr bool ENTRY = PF || LV, BANK = PF, STACKED = PF != LV;
  static_assert(!ENTRY || (KIND == K_FLUX && sizeof(T) == 8 && !XE), "the per-entry forms are the f64 flux kinds' plain strips");
  if constexpr (ENTRY) {
    bool ok = cut.form == RINGC_PLAIN && !cut.xe && pl->kind == K_FLUX && pl->d.dtype == GCMF_F64 && cv.stacked == STACKED;
    if constexpr (BANK) ok = ok && cv.bank_n >= 1 && cv.bank_rev && a.lvl >= 1 && (size_t)(a.lvl - 1 + S) < cv.bank_stride;
    if constexpr (BANK && STACKED) ok = ok && cv.nlev == cv.bank_nfield && !pl->g.fold;
    if (!ok) {
      set_error(!BANK     ? "k_ringc (stacked plan): the cut is not the plain strips of an f64 flux plan"
                : !STACKED ? "k_ringc (filter bank): the cut is not the plain strips of an ordinary f64 flux plan inside gcmf_apply_bank"
                           : "k_ringc (filter bank over per-field planes): the cut is not the plain strips of an f64 flux plan without a seam inside gcmf_apply_bank_gaps");
      return GCMF_ERR_INVALID_ARG;
    }
  }
  MultiP<T, T> P;
  ringc_params(P, pl, cv, a, cut);   // (a bank over per-field planes: lev0 = entry0 % nlev is the field of the launch's first entry)
  if constexpr (BANK) {
    P.ptab = cv.bank_rev;
    P.pstride = (int)cv.bank_stride;
    P.poff = a.lvl - 1;
    P.nfield = (int)cv.bank_nfield;
    P.ent0 = (int)cv.entry0;
  }
  dim3 block(256), grid(cut.grid_x, cut.grid_y);
  std::string name = kernel_name("k_ringc", {tyname<T>(), KIND, S, FIRST});
  std::string geom = launch_geom(P.H, P.nstrips, P.nwx, P.xcd_per > 0, grid.x, grid.y, a.row_hi - a.row_lo);
  if constexpr (ENTRY) {
    hipLaunchKernelGGL((k_ringc<T, KIND, S, FIRST, PF, LV>), grid, block, 0, s, P);
    if (STACKED) geom += " levels=" + std::to_string((long long)cv.nlev);
    if (BANK) geom += " bank=" + std::to_string(cv.bank_n);
  } else if (cut.form == RINGC_PACKED) {
    hipLaunchKernelGGL((k_ringcp<T, KIND, S, FIRST, XE>), grid, block, 0, s, P);
    name = kernel_name("k_ringcp", {tyname<T>(), KIND, S, FIRST, XE});
  } else if constexpr (XE) {
    hipLaunchKernelGGL((k_ringcs<T, S, FIRST>), grid, block, 0, s, P);
    name = kernel_name("k_ringcs", {tyname<T>(), S, FIRST});
    // (the early-exit units have always compiled the plain k_ringc of their depths as well, which nothing launches from here: named so
    // that their code objects stay what they were -- dropping it is a change of the device code, to be made and measured on its own)
    (void)&k_ringc<T, KIND, S, FIRST>;
  } else {
    bool own = false;   // (GCMF_MASK_FROM_NAN: the instantiation that adds the entry's offset to its mask row pointers)
    if constexpr (KIND == K_MASKZ) {
      own = cv.mask_per_field != 0;
      if (own) hipLaunchKernelGGL((k_ringc<T, KIND, S, FIRST, true>), grid, block, 0, s, P);
    }
    if (!own) hipLaunchKernelGGL((k_ringc<T, KIND, S, FIRST>), grid, block, 0, s, P);
  }
  GCMF_HIP(hipGetLastError());
  note_kernel(pl, name, S, geom);
  return GCMF_OK;
}

}  // namespace gcmf
