// Stand-alone driver of the per-entry fold rule (gcm_filters_amd/csrc/gcmf_gap_fold.hpp), for tests/test_gap_fold_rule.py.
//   gap_fold_main IN OUT
// IN:  int32 ncases, then per case: int32 ny, nx, mom5; float64 field[ny * nx], cE[ny * nx], cN[ny * nx]
// OUT: per case: float64 cE_b[ny * nx], cN_b[ny * nx]; uint8 land[ny * nx]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gcmf_gap_fold.hpp"

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
    int32_t hdr[3];
    if (!get(in, hdr, 3) || hdr[0] < 1 || hdr[1] < 1) return 3;
    const size_t n = (size_t)hdr[0] * hdr[1];
    std::vector<double> f(n), cE(n), cN(n), cEb(n), cNb(n);
    std::vector<unsigned char> land(n);
    if (!get(in, f.data(), n) || !get(in, cE.data(), n) || !get(in, cN.data(), n)) return 3;
    gcmf::gap_fold_plane<double>(f.data(), cE.data(), cN.data(), hdr[0], hdr[1], hdr[2] != 0, cEb.data(), cNb.data(), land.data());
    if (!put(out, cEb.data(), n) || !put(out, cNb.data(), n) || !put(out, land.data(), n)) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
