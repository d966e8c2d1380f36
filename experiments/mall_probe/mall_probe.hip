// Two questions about the 256 MB memory-side cache (MALL / Infinity Cache), no arithmetic in either.
//   ./mall_probe sweep   Does a working set that fits the cache stream faster than one that does not?  A 6-read : 2-write plane pass
//                        (the mix of a k_ringc launch) over a working set of W MB, repeated; GB/s by working-set size.
//   ./mall_probe march   Do non-temporal state loads / stores keep the constants of the nine-level table march cached?  The traffic of
//                        config 3's later k_ringcz launches: 1020 lone waves (17 windows with rows [1200, 2400), 17 with [0, 2400), 60-row
//                        strips zipped in pairs at a shared seam, 108 owned of 128 footprint columns, 10 ghost rows at the far end), per
//                        row four constant planes and a byte plane read, two state planes read, two written; seven launches back to back
//                        over a pool of four state planes, as gcmf_apply rotates them.  Variants alternate in one process.
//   hipcc --offload-arch=gfx950 -O3 -o mall_probe mall_probe.hip && ./mall_probe march
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct P { const double2 *r[6]; double2 *w[2]; long long n; };

__global__ __launch_bounds__(256) void k_pass(P p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride) {
    double2 a = p.r[0][i], b = p.r[1][i], c = p.r[2][i], d = p.r[3][i], e = p.r[4][i], f = p.r[5][i];
    double2 u, v;
    u.x = a.x + b.x * c.x + d.x; u.y = a.y + b.y * c.y + d.y;
    v.x = e.x - f.x * a.x;       v.y = e.y - f.y * a.y;
    p.w[0][i] = u;
    p.w[1][i] = v;
  }
}

static int sweep() {
  const size_t maxb = 1200ull << 20;
  char *buf;
  CK(hipMalloc(&buf, maxb));
  CK(hipMemset(buf, 0, maxb));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int mb : {32, 64, 96, 128, 160, 192, 224, 256, 320, 384, 512, 768, 1100}) {
    const size_t plane = ((size_t)mb << 20) / 8 / 16 * 16;   // bytes per plane, 8 planes in the working set
    P p;
    for (int q = 0; q < 6; ++q) p.r[q] = (const double2 *)(buf + q * plane);
    for (int q = 0; q < 2; ++q) p.w[q] = (double2 *)(buf + (6 + q) * plane);
    p.n = plane / 16;
    const int reps = 30;
    for (int blocks : {2048, 8192}) {
      for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_pass, dim3(blocks), dim3(256), 0, 0, p);
      CK(hipEventRecord(e0));
      for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_pass, dim3(blocks), dim3(256), 0, 0, p);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      printf("working set %4d MB, %5d blocks: %7.1f us per pass, %6.2f TB/s\n", mb, blocks, ms / reps * 1e3, 8.0 * plane * reps / (ms * 1e-3) / 1e12);
    }
  }
  return 0;
}

// ---- the table march's traffic ----
typedef double v2d __attribute__((ext_vector_type(2)));
constexpr int NX = 3600, ROWS = 2400, H = 60, GHOST = 10, WI = 108, MX = 10, XOFF = 36, NWAVES = 1020, U = 3;
struct M { const double *cE, *cN, *ra, *f; const unsigned char *z; const double *u0, *v0; double *uo, *vo; };

// POL bit 0: nt state stores, bit 1: nt state loads, bit 2: nt loads of f
template <bool NT> __device__ __forceinline__ v2d ld(const double *p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const v2d *>(p));
  else return *reinterpret_cast<const v2d *>(p);
}
template <bool NT> __device__ __forceinline__ void st(double *p, v2d x) {
  if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<v2d *>(p));
  else *reinterpret_cast<v2d *>(p) = x;
}

template <int POL>
__global__ __launch_bounds__(256) void k_march(const M p) {
  constexpr bool NTS = POL & 1, NTL = (POL & 2) != 0, NTF = (POL & 4) != 0;
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wid >= NWAVES) return;
  // 17 groups of 60 waves: window 2 g holds rows [1200, 2400) (20 strips), window 2 g + 1 rows [0, 2400) (40 strips)
  const int g = wid / 60, k = wid % 60;
  const int win = 2 * g + (k >= 20), strip = k >= 20 ? k - 20 : k;
  const int a = (k >= 20 ? 0 : 1200) + strip * H, b = a + H;
  const bool up = !(strip & 1);   // strips 2 i and 2 i + 1 share the seam between them and march away from it
  const int col = (XOFF + win * WI - MX + lane * 2) % NX;   // (even, so col + 1 < NX)
  const bool keep = lane * 2 >= MX && lane * 2 < 128 - MX;
  v2d acc = {0.0, 0.0};
  // march row m = 0 is the partner's first row, 1 .. H the strip's own, H + 1 .. H + GHOST - 1 the ghost rows at the far end
  for (int m0 = 0; m0 < H + GHOST; m0 += U) {
    v2d x[U][6];
    unsigned zz[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int m = min(m0 + q, H + GHOST - 1);
      int r = up ? b - m : a - 1 + m;
      r = r < 0 ? r + ROWS : (r >= ROWS ? r - ROWS : r);
      const long long o = (long long)r * NX + col;
      x[q][0] = ld<false>(p.cE + o); x[q][1] = ld<false>(p.cN + o); x[q][2] = ld<false>(p.ra + o);
      x[q][3] = ld<NTF>(p.f + o);
      zz[q] = *reinterpret_cast<const unsigned short *>(p.z + o);
      x[q][4] = ld<NTL>(p.u0 + o); x[q][5] = ld<NTL>(p.v0 + o);
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int m = m0 + q;
      if (m >= H + GHOST) break;
      const v2d s0 = x[q][0] + x[q][1] + x[q][4] + acc, s1 = x[q][2] + x[q][3] + x[q][5] + (double)zz[q];
      if (m >= 1 && m <= H) {   // wave-uniform
        const int r = up ? b - m : a - 1 + m;
        const long long o = (long long)r * NX + col;
        if (keep) { st<NTS>(p.uo + o, s0); st<NTS>(p.vo + o, s1); }
      } else {
        acc += s0 * s1;   // (a ghost row's loads stay live: see below)
      }
    }
  }
  if (acc.x == 12345.0) st<false>(p.uo + (long long)a * NX + col, acc);   // (never: the planes hold zeros)
}

template <int POL> static void launch7(const M &m0) {
  M m = m0;
  for (int l = 0; l < 7; ++l) {
    hipLaunchKernelGGL((k_march<POL>), dim3((NWAVES + 3) / 4), dim3(256), 0, 0, m);
    const double *u = m.uo, *v = m.vo;   // the two planes of the pool that hold neither u nor v are the ones just read
    m.uo = const_cast<double *>(m.u0); m.vo = const_cast<double *>(m.v0);
    m.u0 = u; m.v0 = v;
  }
}

static int march() {
  const size_t plane = (size_t)NX * ROWS * sizeof(double);
  double *pl[8];
  for (int q = 0; q < 8; ++q) { CK(hipMalloc((void **)&pl[q], plane)); CK(hipMemset(pl[q], 0, plane)); }
  unsigned char *z;
  CK(hipMalloc((void **)&z, (size_t)NX * ROWS)); CK(hipMemset(z, 0, (size_t)NX * ROWS));
  const M m{pl[0], pl[1], pl[2], pl[3], z, pl[4], pl[5], pl[6], pl[7]};
  const char *name[5] = {"all default", "nt state stores", "nt state loads", "nt state stores + loads", "nt state stores + loads + nt f"};
  void (*run[5])(const M &) = {launch7<0>, launch7<1>, launch7<2>, launch7<3>, launch7<7>};
  const int rounds = 20, reps = 3;
  std::vector<float> us[5];
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int rd = 0; rd < rounds; ++rd) {
    for (int v = 0; v < 5; ++v) {
      run[v](m);   // (the cache holds what this variant leaves there, not its predecessor's)
      CK(hipEventRecord(e0));
      for (int i = 0; i < reps; ++i) run[v](m);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      us[v].push_back(ms * 1e3f / (7 * reps));
    }
  }
  CK(hipGetLastError());
  const double owned = (double)NWAVES * H * WI, moved = (double)NWAVES * ((H + GHOST) * 64.0 * (6 * 16 + 2) + H * 54.0 * 32);
  printf("table march model: %d waves, %.2f M owned cells, %.0f MB per launch with the halos; us per launch over %d rounds of %d x 7 launches\n",
         NWAVES, owned / 1e6, moved / 1e6, rounds, reps);
  for (int v = 0; v < 5; ++v) {
    std::sort(us[v].begin(), us[v].end());
    const float med = us[v][rounds / 2];
    printf("%-32s min %6.1f  median %6.1f  max %6.1f  (%.2f TB/s at the median)\n", name[v], us[v].front(), med, us[v].back(), moved / (med * 1e-6) / 1e12);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "march")) return march();
  printf("usage: mall_probe sweep | march\n");
  return 2;
}
