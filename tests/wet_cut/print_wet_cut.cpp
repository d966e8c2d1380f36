// Prints the tight cut of the wet-row table (csrc/gcmf_wet_cut.hpp) for masks read from standard input; compiled by tests/test_wet_cut.py
// with g++ against that header alone -- no HIP, no library, no GPU.
//
// Input, any number of times:  "rows nx S row_lo row_hi list" and then rows lines of nx characters, '1' = the cell exchanges with a neighbour.
// Output per mask:  "ok=<0|1> xoff=.. units=.. H=.. nstrips=.. march=.. owned=.." and, with list = 1, one line "x0 lo mid hi" per pair.
#include <cstdio>
#include <string>
#include <vector>

#include "gcmf_wet_cut.hpp"

int main() {
  int rows, nx, S, row_lo, row_hi, list;
  while (std::scanf("%d %d %d %d %d %d", &rows, &nx, &S, &row_lo, &row_hi, &list) == 6) {
    if (rows < 1 || nx < 1 || rows > (1 << 20) || nx > (1 << 20)) return 2;
    std::vector<uint8_t> bits((size_t)rows * nx);
    std::vector<char> line((size_t)nx + 2);
    for (int r = 0; r < rows; ++r) {
      const std::string fmt = "%" + std::to_string(nx) + "s";
      if (std::scanf(fmt.c_str(), line.data()) != 1) return 3;
      for (int i = 0; i < nx; ++i) {
        if (line[i] != '0' && line[i] != '1') return 4;
        bits[(size_t)r * nx + i] = line[i] == '1' ? 0x81 : 0x80;   // (only bit 0 counts)
      }
    }
    const gcmf::WetCut c = gcmf::wet_cut_tight(bits.data(), rows, nx, S, row_lo, row_hi);
    std::printf("ok=%d xoff=%d units=%zu H=%d nstrips=%d march=%d owned=%lld\n", c.ok ? 1 : 0, c.xoff, c.units.size(), c.H, c.nstrips, c.march, c.owned);
    if (list)
      for (const gcmf::WetUnit &u : c.units) std::printf("%d %d %d %d\n", u.x0, u.lo, u.mid, u.hi);
  }
  return 0;
}
