// Host program of tests/test_fused_share_cpu.py: steps through the sharing rules of
// csrc/fused_skip.h -- the list of items the waves of predict_fused_kernel take their last r
// pass from, and the mask bits by which an item of one group leaves the other group out of a
// part's walk (csrc/fused_walk.h) -- in integer arithmetic.
//
//   fused_share_host < commands
//
// Commands, one after the other until the end of the input (integers separated by white space):
//   items share               ->  "count n", then "item index tile part select" per item
//   walk  select guard rb0 cb0 count triangular n_cb n_blocks d[4 n_blocks][32]
//       one tile's integer densities, rows = columns of the component.  Steps through the part
//       as an item with `select` (0 both groups, 1 the even columns', 2 the odd ones') does: the
//       masks of these densities if guard is 1, no zero-block bits if it is 0, the selection
//       bits either way.  Prints
//         "P rb cb g"     a product issued for group g
//         "C rb g"        group g's accumulators cleared in block row rb
//         "E rb g"        group g's accumulators added to its sums at the end of block row rb
//         "F g c value"   the sum of group g, draw c
//         "G g c value"   the same from every product of the part
//       then "done".
// Stands alone: c++ -std=c++17 -fsanitize=address,undefined -I tabcorr_amd/csrc
// tests/fused_share_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fused_skip.h"
#include "fused_walk.h"

namespace {

bool next_token(std::string* token) {
  token->clear();
  int ch;
  while ((ch = std::getchar()) != EOF && (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r')) {}
  if (ch == EOF) return false;
  do {
    token->push_back((char)ch);
  } while ((ch = std::getchar()) != EOF && ch != ' ' && ch != '\n' && ch != '\t' && ch != '\r');
  return true;
}

long long next_int() {
  std::string token;
  if (!next_token(&token)) {
    std::fprintf(stderr, "fused_share_host: the input ends inside a command\n");
    std::exit(2);
  }
  return std::strtoll(token.c_str(), nullptr, 10);
}

// The matrix words of a table unit: A[v][k], small integers of either sign.
long long matrix_word(unsigned unit, int v, int k) {
  uint32_t x = unit * 2654435761u + (uint32_t)(v * 4 + k) * 40503u + 12345u;
  x ^= x >> 13;
  x *= 2246822519u;
  x ^= x >> 16;
  return (long long)(x % 19u) - 9;
}

void command_items() {
  const int share = (int)next_int();
  const int count = tc::share_item_count(share);
  std::printf("count %d\n", count);
  for (int index = 0; index < count; ++index) {
    const tc::ShareItem item = tc::share_item(share, index);
    std::printf("item %d %d %d %d\n", index, item.tile, item.part, item.select);
  }
}

void command_walk() {
  const int select = (int)next_int(), guard = (int)next_int();
  tc::FusedPart part{};
  part.rb0 = (int)next_int();
  part.cb0 = (int)next_int();
  part.count = (int)next_int();
  part.triangular = (int)next_int();
  part.n_cb = (int)next_int();
  part.unit_base = 0;
  const int n_blocks = (int)next_int();
  if (select < 0 || select > 2 || n_blocks < 1 || n_blocks > tc::kSkipMaxBlocks) {
    std::fprintf(stderr, "fused_share_host: walk: select 0 .. 2, 1 .. %d blocks\n",
                 tc::kSkipMaxBlocks);
    std::exit(2);
  }
  const int rows = 4 * n_blocks;
  std::vector<long long> value((size_t)rows * 32);
  std::vector<double> dens((size_t)rows * tc::kSkipDraws, 0.0);
  for (int row = 0; row < rows; ++row)
    for (int column = 0; column < 32; ++column) {
      const long long v = next_int();
      value[(size_t)row * 32 + (column & 1) * 16 + (column >> 1)] = v;
      dens[(size_t)row * tc::kSkipDraws + column] = (double)v;
    }
  auto at = [&](int row, int g, int c) { return value[(size_t)row * 32 + g * 16 + c]; };
  {
    int rb = part.rb0, cb = part.cb0;
    for (int i = 0; i < part.count; ++i) {
      if (rb >= n_blocks || cb >= n_blocks) {
        std::fprintf(stderr, "fused_share_host: walk: block (%d, %d) beyond the densities\n", rb, cb);
        std::exit(2);
      }
      if (++cb == tc::walk_row_length(part, rb)) { ++rb; cb = 0; }
    }
  }
  const uint64_t leave = tc::share_select_bits(select);
  const uint64_t zero = guard ? tc::skip_tile_mask(dens.data(), 0, n_blocks, 0) : 0;
  const uint64_t mask_b = zero | leave, mask_e = zero | leave;

  const long long kGarbage = 1000003;  // what a sum holds that nobody started
  struct Stage { unsigned unit; int column; } stages[2] = {};
  long long D[2][4][16], F[2][16] = {};
  for (auto& g : D) for (auto& v : g) for (auto& c : v) c = kGarbage;
  unsigned row_bits = 0;
  tc::fused_walk(
      part,
      [&](auto stage, unsigned unit, int column, bool) {
        stages[decltype(stage)::value] = Stage{unit, column};
      },
      [&](int rb) {
        row_bits = tc::skip_bits(mask_e, rb);
        for (auto& g : D) for (auto& v : g) for (auto& c : v) c = kGarbage;
      },
      [&](auto stage, bool first, int rb, int cb) {
        const Stage s = stages[decltype(stage)::value];
        tc::skip_consume(
            first, row_bits, row_bits | tc::skip_bits(mask_b, cb),
            [&](auto group, bool start) {
              constexpr int G = decltype(group)::value;
              std::printf("P %d %d %d\n", rb, cb, G);
              for (int v = 0; v < 4; ++v)
                for (int c = 0; c < 16; ++c) {
                  long long sum = start ? 0 : D[G][v][c];
                  for (int k = 0; k < 4; ++k)
                    sum += matrix_word(s.unit, v, k) * at(4 * s.column + k, G, c);
                  D[G][v][c] = sum;
                }
            },
            [&](auto group) {
              constexpr int G = decltype(group)::value;
              std::printf("C %d %d\n", rb, G);
              for (int v = 0; v < 4; ++v)
                for (int c = 0; c < 16; ++c) D[G][v][c] = 0;
            });
      },
      [&]() { stages[0] = stages[1]; },
      [&](int rb) {
        for (int g = 0; g < 2; ++g) {
          if (row_bits & (1u << g)) continue;
          std::printf("E %d %d\n", rb, g);
          for (int v = 0; v < 4; ++v)
            for (int c = 0; c < 16; ++c) F[g][c] += D[g][v][c] * at(4 * rb + v, g, c);
        }
      });
  for (int g = 0; g < 2; ++g)
    for (int c = 0; c < 16; ++c) std::printf("F %d %d %lld\n", g, c, F[g][c]);

  long long G_[2][16] = {};
  {
    int rb = part.rb0, cb = part.cb0;
    for (int i = 0; i < part.count; ++i) {
      const unsigned unit =
          (unsigned)(part.triangular ? rb * (rb + 1) / 2 + cb : rb * part.n_cb + cb);
      for (int g = 0; g < 2; ++g)
        for (int c = 0; c < 16; ++c)
          for (int v = 0; v < 4; ++v) {
            long long sum = 0;
            for (int k = 0; k < 4; ++k) sum += matrix_word(unit, v, k) * at(4 * cb + k, g, c);
            G_[g][c] += sum * at(4 * rb + v, g, c);
          }
      if (++cb == tc::walk_row_length(part, rb)) { ++rb; cb = 0; }
    }
  }
  for (int g = 0; g < 2; ++g)
    for (int c = 0; c < 16; ++c) std::printf("G %d %d %lld\n", g, c, G_[g][c]);
  std::printf("done\n");
}

}  // namespace

int main() {
  std::string command;
  while (next_token(&command)) {
    if (command == "items") command_items();
    else if (command == "walk") command_walk();
    else {
      std::fprintf(stderr, "fused_share_host: unknown command %s\n", command.c_str());
      return 2;
    }
  }
  return 0;
}
