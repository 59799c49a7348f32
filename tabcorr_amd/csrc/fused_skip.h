// Which matrix products of predict_fused_kernel's 64-draw, eight-wave deferring instances can be
// left out, and where a workgroup's draws are placed so that many can: for host and device, like
// fused_walk.h.  kernels.hip.h (fused_quad_pass_skip, predict_fused_kernel) takes the rules from
// here; tests/test_fused_skip_cpu.py compiles this header into a host program
// (tests/fused_skip_host.cpp) that steps through them.
//
// A matrix instruction of the kernel serves one block of four density rows (its B operand) and
// one GROUP of 16 draws; a wave's tile of 32 draws is two groups, the even (b.x) and the odd
// (b.y) columns of the tile, so a workgroup has four: group = 2 (column / 32) + column % 2.
// If all 64 densities of (block, group) are zero, every product of a unit in that block COLUMN
// is +-0 for the group, and so is every term fma(D, e, F) of that block ROW: leaving them out
// keeps the bits of the sums, which start at +0 -- as long as no other factor is infinite or NaN
// (the kernel's guard: every matrix entry finite, every draw's pair-weight sum below 1e280).
//
// A Zheng07 satellite bin is exactly zero for every draw whose M0 lies at or above it, so the
// draws of a workgroup are placed in the LDS density array in the order of M0: rank r goes to
// the column of group r / 16.  A draw's values do not depend on its column: same bits.
// (Measured, profiles/skip_notes.md: the skipping alone is level with issuing everything, with
// the order 1.0 us per 10^4 draws ahead, with the parts (0, 1) and (2, 3) on a SIMD 1.6.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TC_SKIP_FN __host__ __device__ __forceinline__
#else
#define TC_SKIP_FN inline
#endif

namespace tc {

constexpr int kSkipDraws = 64;         // draws of a workgroup
constexpr int kSkipGroups = 4;         // groups of 16 draws
constexpr int kSkipMaxBlocks = 32;     // blocks of four density rows a mask word pair can hold

template <int G>
struct SkipGroup {
  static constexpr int value = G;
};

// The order key of a draw: unsigned integers that order like the doubles, NaN below everything.
// (The high dword decides: 20 bits of mantissa are more than the bins' edges need.)
TC_SKIP_FN uint32_t skip_key(double value) {
  if (value != value) return 0u;
  value += 0.0;                          // (-0 as +0: equal keys for equal values)
  uint64_t bits;
  __builtin_memcpy(&bits, &value, sizeof bits);
  const uint32_t hi = (uint32_t)(bits >> 32);
  // (-inf comes out as 0x000fffff: above NaN's 0)
  return (hi & 0x80000000u) ? ~hi : (hi | 0x80000000u);
}

// Ties break by index: the key's six lowest bits make room for the draw's index in the
// workgroup, so that 64 keys are 64 different numbers whatever the input.
TC_SKIP_FN uint32_t skip_unique_key(uint32_t key, int index) {
  return (key & ~(uint32_t)(kSkipDraws - 1)) | (uint32_t)index;
}

// rank (0 .. 63, by unique key) -> column of the LDS density array: ranks 16 g .. 16 g + 15 are
// group g = (tile, parity), the columns 32 tile + 2 c + parity.
TC_SKIP_FN int skip_column(int rank) {
  return 32 * (rank >> 5) + 2 * (rank & 15) + ((rank >> 4) & 1);
}
TC_SKIP_FN int skip_group_of_column(int column) { return 2 * (column >> 5) + (column & 1); }

// Host form of the kernel's rank (the kernel counts with one lane per draw).
inline void skip_perm(const double* keys, int* column) {
  uint32_t unique[kSkipDraws];
  for (int d = 0; d < kSkipDraws; ++d) unique[d] = skip_unique_key(skip_key(keys[d]), d);
  for (int d = 0; d < kSkipDraws; ++d) {
    int rank = 0;
    for (int other = 0; other < kSkipDraws; ++other) rank += unique[other] < unique[d];
    column[d] = skip_column(rank);
  }
}

// A density counts as zero if it compares equal to zero: +0 and -0 do, NaN does not.
TC_SKIP_FN bool skip_is_zero(double value) { return value == 0.0; }

// The masks of a tile's two groups in one word: bit 2 block + parity is set where all 64
// densities of (block, group) are zero.  Host form; dens is (rows, 64), row0 the first row of
// block 0, n_blocks whole blocks (at most kSkipMaxBlocks).
inline uint64_t skip_tile_mask(const double* dens, int row0, int n_blocks, int tile) {
  uint64_t mask = 0;
  for (int block = 0; block < n_blocks && block < kSkipMaxBlocks; ++block)
    for (int parity = 0; parity < 2; ++parity) {
      bool all = true;
      for (int v = 0; v < 4; ++v)
        for (int c = 0; c < 16; ++c)
          all = all && skip_is_zero(dens[(row0 + 4 * block + v) * kSkipDraws + 32 * tile + 2 * c +
                                         parity]);
      if (all) mask |= (uint64_t)1 << (2 * block + parity);
    }
  return mask;
}

// The two groups' bits of block `block`: bit 0 the even columns' group, bit 1 the odd ones'.
TC_SKIP_FN unsigned skip_bits(uint64_t mask, int block) {
  return (unsigned)(mask >> (2 * block)) & 3u;
}

// The products of one unit.  row_bits: the groups whose block row is zero (they take no part in
// the row at all); unit_bits: the groups that leave this unit out (row_bits included).
//   products(SkipGroup<g>, first)   the unit's products for group g
//   clear(SkipGroup<g>)    group g's accumulators = +0: its first unit of the row is left out, a
//                          later one may not be, and then adds to them
// first: the part's first unit of the row (fused_walk.h); with it the products start the sums.
// (One test and one branch per group: the accumulators of a group that is left out stay where
// they are.  A branch to one of four copies of the products made the compiler move all
// accumulators at every unit.)
template <class Products, class Clear>
TC_SKIP_FN void skip_consume(bool first, unsigned row_bits, unsigned unit_bits,
                             Products&& products, Clear&& clear) {
  if (!(unit_bits & 1u)) products(SkipGroup<0>(), first);
  else if (first && !(row_bits & 1u)) clear(SkipGroup<0>());
  if (!(unit_bits & 2u)) products(SkipGroup<1>(), first);
  else if (first && !(row_bits & 2u)) clear(SkipGroup<1>());
}

// ---- sharing the last r pass (option "fused_share", profiles/share_notes.md) ----------------
// Where the last pass of a wave's part covers ONE r sub-tile (U = 3, 5), its sums meet no other
// pass's, and the tile's two groups have accumulators of their own: the chain (tile, part, last
// pass, group) gives the same bits on any wave at any time.  Instead of walking its own part a
// last time every wave takes ITEMS from a counter in LDS until none is left -- nothing is
// estimated, nobody waits: the waves whose parts had many zero blocks take more.
//   share 1   8 items, one per (tile, part), both groups
//   share 2   16 items, one per (tile, part, group)
// The list is fixed, the heaviest expected first: the first part (all centrals: no zero
// blocks) of both tiles, then the parts 3, 2 and 1.
constexpr int kShareParts = 4;                    // parts per tile (eight waves, 64 draws)
constexpr int kShareJobs = 2 * kShareParts;       // (tile, part): the slot 4 tile + part
// LDS of the queue (words of 32 bits): the counter, a word per job that says its masks are
// there, the jobs' masks (two words of 64 bits each)
constexpr int kShareCounterWord = 0;
constexpr int kShareFlagWord = 8;
constexpr int kShareMaskWord = 16;
constexpr int kShareWords = kShareMaskWord + 4 * kShareJobs;

struct ShareItem {
  int tile, part;
  int select;              // 0 both groups, 1 the even columns' alone, 2 the odd ones'
};

TC_SKIP_FN int share_item_count(int share) { return share == 1 ? kShareJobs : share == 2 ? 2 * kShareJobs : 0; }

TC_SKIP_FN ShareItem share_item(int share, int index) {
  const int job = share == 2 ? index >> 1 : index;
  const int turn = job >> 1;                      // 0: part 0; 1, 2, 3: parts 3, 2, 1
  ShareItem item;
  item.tile = job & 1;
  item.part = turn == 0 ? 0 : kShareParts - turn;
  item.select = share == 2 ? 1 + (index & 1) : 0;
  return item;
}

// What an item ORs into a job's mask words: the bit of the OTHER group in every block, so that
// skip_consume and the row ends leave that group out altogether.  Selecting is not skipping: it
// holds where the guard has failed and the zero-block bits are all 0 as well.
TC_SKIP_FN uint64_t share_select_bits(int select) {
  return select == 1 ? 0xAAAAAAAAAAAAAAAAull : select == 2 ? 0x5555555555555555ull : 0ull;
}

}  // namespace tc
