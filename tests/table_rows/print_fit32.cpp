// table_rows_fit32() / table_rows_ok() of csrc/gcmf_wet_cut.hpp, compiled alone (tests/test_table_rows_predicate.py): "rows nx cell" per line in,
// "fit32 ok(wraps) ok(closed)" per line out
#include <cstdio>

#include "gcmf_wet_cut.hpp"

int main() {
  long long rows, nx, cell;
  while (std::scanf("%lld %lld %lld", &rows, &nx, &cell) == 3) std::printf("%d %d %d\n", gcmf::table_rows_fit32(rows, nx, cell) ? 1 : 0, gcmf::table_rows_ok(rows, nx, cell, true) ? 1 : 0, gcmf::table_rows_ok(rows, nx, cell, false) ? 1 : 0);
  return 0;
}
