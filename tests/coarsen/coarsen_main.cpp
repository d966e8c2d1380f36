// Stand-alone driver of the block-mean rule (gcm_filters_amd/csrc/gcmf_coarsen.hpp), for tests/test_coarsen_rule.py.
//   coarsen_main IN OUT
// IN:  int32 ncases, then per case: int32 ny, nx, fy, fx, has_weights; float64 fine[ny * nx]; has_weights: float64 w[ny * nx]
// OUT: per case: float64 coarse[(ny / fy) * (nx / fx)], wsum[(ny / fy) * (nx / fx)]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gcmf_coarsen.hpp"

template <typename T> static bool get(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T> static bool put(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  int32_t ncases = 0;
  if (!get(in, &ncases, 1)) return 3;
  for (int32_t c = 0; c < ncases; ++c) {
    int32_t hdr[5];
    if (!get(in, hdr, 5) || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1 || hdr[3] < 1 || hdr[0] % hdr[2] || hdr[1] % hdr[3]) return 3;
    const size_t n = (size_t)hdr[0] * hdr[1], nc = (size_t)(hdr[0] / hdr[2]) * (hdr[1] / hdr[3]);
    std::vector<double> f(n), w(hdr[4] ? n : 0), coarse(nc), wsum(nc);
    if (!get(in, f.data(), n) || (hdr[4] && !get(in, w.data(), n))) return 3;
    gcmf::coarsen_plane(f.data(), hdr[4] ? w.data() : nullptr, hdr[0], hdr[1], hdr[2], hdr[3], coarse.data(), wsum.data());
    if (!put(out, coarse.data(), nc) || !put(out, wsum.data(), nc)) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
