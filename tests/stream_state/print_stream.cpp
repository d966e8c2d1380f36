// stream_state_ok() and table_owned_cells() of csrc/gcmf_wet_cut.hpp, compiled alone (tests/test_stream_predicate.py) -- no HIP, no library,
// no GPU.
//
// Input, any number of times, one of
//   "c cells"                         a count of owned cells
//   "m rows nx S" and then rows lines of nx characters, '1' = the cell exchanges with a neighbour: the tight table of the whole grid
// Output per request:  "cells=.. stream=<0|1> budget=.. cell_bytes=.."
#include <cstdio>
#include <string>
#include <vector>

#include "gcmf_wet_cut.hpp"

static void answer(long long cells) {
  std::printf("cells=%lld stream=%d budget=%lld cell_bytes=%lld\n", cells, gcmf::stream_state_ok(cells) ? 1 : 0, gcmf::STREAM_CACHE_BYTES, gcmf::STREAM_CELL_BYTES);
}

int main() {
  char what;
  while (std::scanf(" %c", &what) == 1) {
    if (what == 'c') {
      long long cells;
      if (std::scanf("%lld", &cells) != 1) return 2;
      answer(cells);
      continue;
    }
    int rows, nx, S;
    if (what != 'm' || std::scanf("%d %d %d", &rows, &nx, &S) != 3 || rows < 1 || nx < 1 || rows > (1 << 20) || nx > (1 << 20)) return 2;
    std::vector<uint8_t> bits((size_t)rows * nx);
    std::vector<char> line((size_t)nx + 2);
    const std::string fmt = "%" + std::to_string(nx) + "s";
    for (int r = 0; r < rows; ++r) {
      if (std::scanf(fmt.c_str(), line.data()) != 1) return 3;
      for (int i = 0; i < nx; ++i) {
        if (line[i] != '0' && line[i] != '1') return 4;
        bits[(size_t)r * nx + i] = line[i] == '1' ? 0x81 : 0x80;   // (only bit 0 counts)
      }
    }
    const gcmf::WetCut c = gcmf::wet_cut_tight(bits.data(), rows, nx, S, 0, rows);
    if (!c.ok) return 5;
    answer(gcmf::table_owned_cells(c.units.data(), c.units.size(), S, nx + c.xoff));
  }
  return 0;
}
