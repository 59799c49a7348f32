// Host program of tests/test_fused_walk_cpu.py: steps through csrc/fused_walk.h with callbacks
// that print what the kernel's callbacks would load and multiply.
//
//   fused_walk_host < parts
//
// reads one part per line -- rb0 cb0 count triangular n_cb unit_base -- and prints its calls,
// one per line, then "done":
//   R stage unit column inside      request
//   B rb                            row_begin
//   C stage first rb cb             consume
//   M                               move (stage 1's operands into stage 0)
//   E rb                            row_end
#include <cstdio>

#include "fused_walk.h"

static void run(const tc::FusedPart& part) {
  tc::fused_walk(
      part,
      [](auto stage, unsigned unit, int column, bool inside) {
        std::printf("R %d %u %d %d\n", decltype(stage)::value, unit, column, inside ? 1 : 0);
      },
      [](int rb) { std::printf("B %d\n", rb); },
      [](auto stage, bool first, int rb, int cb) {
        std::printf("C %d %d %d %d\n", decltype(stage)::value, first ? 1 : 0, rb, cb);
      },
      []() { std::printf("M\n"); }, [](int rb) { std::printf("E %d\n", rb); });
}

int main() {
  tc::FusedPart part;
  std::printf("depth %d\n", tc::kFusedRingDepth);
  while (std::scanf("%d %d %d %d %d %u", &part.rb0, &part.cb0, &part.count, &part.triangular,
                    &part.n_cb, &part.unit_base) == 6) {
    run(part);
    std::printf("done\n");
  }
  return 0;
}
