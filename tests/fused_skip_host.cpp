// Host program of tests/test_fused_skip_cpu.py: steps through csrc/fused_skip.h -- the rank of a
// workgroup's draws, the masks of all-zero density blocks, and which products of a part's walk
// (csrc/fused_walk.h) they leave out -- the way predict_fused_kernel does, in integer arithmetic.
//
//   fused_skip_host < commands
//
// Commands, one after the other until the end of the input (numbers separated by white space;
// doubles as strtod reads them: nan, inf, -inf, -0.0, 1e300):
//   perm  k0 ... k63                        ->  "perm c0 ... c63": the column of every draw
//   mask  rows row0 n_blocks d[rows][64]    ->  "mask m0 m1": the two tiles' masks, hexadecimal
//   walk  rb0 cb0 count triangular n_cb n_blocks d[4 n_blocks][32]
//       one tile's integer densities, rows = columns of the component.  Steps through the part
//       with the masks of these densities and prints
//         "P rb cb g"     a product issued for group g (0: even draws, 1: odd ones)
//         "F g c value"   the sum of group g, draw c, with products left out
//         "G g c value"   the same from every product of the part, nothing left out
//       then "done".
// Stands alone: c++ -std=c++17 -fsanitize=address,undefined -I tabcorr_amd/csrc
// tests/fused_skip_host.cpp
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

double next_double() {
  std::string token;
  if (!next_token(&token)) {
    std::fprintf(stderr, "fused_skip_host: the input ends inside a command\n");
    std::exit(2);
  }
  return std::strtod(token.c_str(), nullptr);
}

long long next_int() {
  std::string token;
  if (!next_token(&token)) {
    std::fprintf(stderr, "fused_skip_host: the input ends inside a command\n");
    std::exit(2);
  }
  return std::strtoll(token.c_str(), nullptr, 10);
}

// The matrix words of a table unit: A[v][k], row v of the block row, column k of the block
// column; small integers of either sign.
long long matrix_word(unsigned unit, int v, int k) {
  uint32_t x = unit * 2654435761u + (uint32_t)(v * 4 + k) * 40503u + 12345u;
  x ^= x >> 13;
  x *= 2246822519u;
  x ^= x >> 16;
  return (long long)(x % 19u) - 9;
}

void command_perm() {
  double keys[tc::kSkipDraws];
  int column[tc::kSkipDraws];
  for (double& key : keys) key = next_double();
  tc::skip_perm(keys, column);
  std::printf("perm");
  for (int c : column) std::printf(" %d", c);
  std::printf("\n");
}

void command_mask() {
  const int rows = (int)next_int(), row0 = (int)next_int(), n_blocks = (int)next_int();
  if (rows < 0 || row0 < 0 || n_blocks < 0 || row0 + 4 * n_blocks > rows) {
    std::fprintf(stderr, "fused_skip_host: mask: blocks beyond the rows\n");
    std::exit(2);
  }
  std::vector<double> dens((size_t)rows * tc::kSkipDraws);
  for (double& value : dens) value = next_double();
  std::printf("mask %llx %llx\n",
              (unsigned long long)tc::skip_tile_mask(dens.data(), row0, n_blocks, 0),
              (unsigned long long)tc::skip_tile_mask(dens.data(), row0, n_blocks, 1));
}

void command_walk() {
  tc::FusedPart part{};
  part.rb0 = (int)next_int();
  part.cb0 = (int)next_int();
  part.count = (int)next_int();
  part.triangular = (int)next_int();
  part.n_cb = (int)next_int();
  part.unit_base = 0;
  const int n_blocks = (int)next_int();
  if (n_blocks < 1 || n_blocks > tc::kSkipMaxBlocks) {
    std::fprintf(stderr, "fused_skip_host: walk: 1 .. %d blocks\n", tc::kSkipMaxBlocks);
    std::exit(2);
  }
  const int rows = 4 * n_blocks;
  // value[row][g][c]: draw c of group g = column 2 c + g of the tile
  std::vector<long long> value((size_t)rows * 32);
  std::vector<double> dens((size_t)rows * tc::kSkipDraws, 0.0);
  for (int row = 0; row < rows; ++row)
    for (int column = 0; column < 32; ++column) {
      const long long v = next_int();
      value[(size_t)row * 32 + (column & 1) * 16 + (column >> 1)] = v;
      dens[(size_t)row * tc::kSkipDraws + column] = (double)v;
    }
  auto at = [&](int row, int g, int c) { return value[(size_t)row * 32 + g * 16 + c]; };
  const uint64_t mask = tc::skip_tile_mask(dens.data(), 0, n_blocks, 0);

  // the part's blocks must lie inside the densities
  {
    int rb = part.rb0, cb = part.cb0;
    for (int i = 0; i < part.count; ++i) {
      if (rb >= n_blocks || cb >= n_blocks) {
        std::fprintf(stderr, "fused_skip_host: walk: block (%d, %d) beyond the densities\n", rb, cb);
        std::exit(2);
      }
      if (++cb == tc::walk_row_length(part, rb)) { ++rb; cb = 0; }
    }
  }

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
        row_bits = tc::skip_bits(mask, rb);
        for (auto& g : D) for (auto& v : g) for (auto& c : v) c = kGarbage;
      },
      [&](auto stage, bool first, int rb, int cb) {
        const Stage s = stages[decltype(stage)::value];
        tc::skip_consume(
            first, row_bits, row_bits | tc::skip_bits(mask, cb),
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
              for (int v = 0; v < 4; ++v)
                for (int c = 0; c < 16; ++c) D[G][v][c] = 0;
            });
      },
      [&]() { stages[0] = stages[1]; },
      [&](int rb) {
        for (int g = 0; g < 2; ++g) {
          if (row_bits & (1u << g)) continue;
          for (int v = 0; v < 4; ++v)
            for (int c = 0; c < 16; ++c) F[g][c] += D[g][v][c] * at(4 * rb + v, g, c);
        }
      });
  for (int g = 0; g < 2; ++g)
    for (int c = 0; c < 16; ++c) std::printf("F %d %d %lld\n", g, c, F[g][c]);

  // every product of the part
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
    if (command == "perm") command_perm();
    else if (command == "mask") command_mask();
    else if (command == "walk") command_walk();
    else {
      std::fprintf(stderr, "fused_skip_host: unknown command %s\n", command.c_str());
      return 2;
    }
  }
  return 0;
}
