// Stand-alone driver of the covariance rules (gcm_filters_amd/csrc/gcmf_cov.hpp), for tests/test_cov_rule.py.  Build it with
// -ffp-contract=off, as the library is built: the post rule is a product and a difference, never a fused multiply-add.
//   cov_main IN OUT
// IN:  int32 ncases, then per case: int32 n, common, variance; float64 f[n]; !variance: float64 g[n]; float64 a[n], b[n]; !variance: c[n]
// OUT: per case: float64 fo[n]; !variance: go[n]; fg[n]; out[n]      (pre rule on f, g; post rule on a, b, c)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gcmf_cov.hpp"

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
  for (int32_t k = 0; k < ncases; ++k) {
    int32_t hdr[3];
    if (!get(in, hdr, 3) || hdr[0] < 1) return 3;
    const size_t n = (size_t)hdr[0];
    const bool common = hdr[1] != 0, var = hdr[2] != 0;
    std::vector<double> f(n), g(var ? 0 : n), a(n), b(n), c(var ? 0 : n), fo(n), go(var ? 0 : n), fg(n), res(n);
    if (!get(in, f.data(), n) || (!var && !get(in, g.data(), n)) || !get(in, a.data(), n) || !get(in, b.data(), n) ||
        (!var && !get(in, c.data(), n)))
      return 3;
    gcmf::cov_pre_plane(f.data(), var ? nullptr : g.data(), (long long)n, common, fo.data(), var ? nullptr : go.data(), fg.data());
    gcmf::cov_post_plane(a.data(), b.data(), var ? nullptr : c.data(), (long long)n, res.data());
    if (!put(out, fo.data(), n) || (!var && !put(out, go.data(), n)) || !put(out, fg.data(), n) || !put(out, res.data(), n)) return 4;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
