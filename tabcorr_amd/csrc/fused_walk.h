// The walk of one wave over its part of a component's matrix units, for host and device.  Three
// users in kernels.hip.h pass their loads and matrix instructions as callbacks:
//   fused_quad_pass            predict_fused_kernel, 64 and 32 draws per workgroup
//   contract_quad_kernel       the three-kernel path, float64: one walk per run of a wave
//   contract_quad_f32_kernel   the same on float32 tables
// The two contract kernels fence their consume callback (a scheduling barrier as its first and
// as its last statement: requests, barrier, products, barrier, requests, ...); the fused one does
// not, and leaves the interleaving to the compiler (profiles/walk_notes.md).
// (fused_quad_pass40, the latency form of predict_fused_kernel, makes the same requests, products
// and moves in the same order from a loop written out by hand: through this header it measured
// 0.4 us per 10^4 draws behind, profiles/walk_notes.md section 5.)
// tests/test_fused_walk_cpu.py compiles this header into a host program that records the same
// calls.
//
// A part is `count` units of a component from block (rb0, cb0) on, row by row: block row rb of a
// triangular component holds the block columns 0 .. rb, of a rectangular one 0 .. n_cb - 1.  The
// units of a component lie in the table in this order, so the walk's units are consecutive:
// unit_base + rb (rb + 1) / 2 + cb, or unit_base + rb n_cb + cb.
//
// The operands of a unit (the matrix words of its lanes, the densities of its block column) are
// requested one unit ahead into the other of two statically named stages, across row ends; the
// loop of a row's units is unrolled by the two stages and every row begins in stage 0, so a row
// in which the part has an odd number of units (n = 1, 3, 5, ...) ends with a move of the
// requested operands from stage 1 to stage 0.  The request behind the part's last unit has no
// consumer: it asks for the unit behind the part -- the next part's, or the one behind the
// table, which the bounds check of the table's buffer resource answers with zeros -- with block
// column 0.
// (Deeper rings without the move were built on this header and measured: profiles/
// walk_notes.md.)
#pragma once

#if defined(__HIPCC__)
#define TC_WALK_FN __host__ __device__ __forceinline__
#else
#define TC_WALK_FN inline
#endif

namespace tc {

constexpr int kFusedRingDepth = 2;     // units in flight per wave, the consumed one included

struct FusedPart {
  int rb0, cb0;            // first block
  int count;               // units
  int triangular, n_cb;    // block columns 0 .. rb of block row rb, else n_cb in every row
  unsigned unit_base;      // first unit of the component in the table
};

template <int N>
struct WalkStage {
  static constexpr int value = N;
};

TC_WALK_FN int walk_row_length(const FusedPart& p, int rb) { return p.triangular ? rb + 1 : p.n_cb; }

TC_WALK_FN unsigned walk_first_unit(const FusedPart& p) {
  return p.unit_base +
         (unsigned)(p.triangular ? p.rb0 * (p.rb0 + 1) / 2 + p.cb0 : p.rb0 * p.n_cb + p.cb0);
}

// Steps through the part.  The callbacks, in the order of a unit's life:
//   request(WalkStage<s>, unit, column, inside)  load the operands of table unit `unit` (block
//                                                column `column`) into stage s; !inside: nobody
//                                                will consume them
//   row_begin(rb)                                the part enters block row rb
//   consume(WalkStage<s>, first, rb, cb)         the matrix instructions of block (rb, cb) from
//                                                stage s; first: the part's first unit of the row
//   move()                                       stage 1's operands into stage 0
//   row_end(rb)                                  the part leaves block row rb
template <class Request, class RowBegin, class Consume, class Move, class RowEnd>
TC_WALK_FN void fused_walk(const FusedPart& p, Request&& request, RowBegin&& row_begin,
                           Consume&& consume, Move&& move, RowEnd&& row_end) {
  int rb = p.rb0, cb = p.cb0, left = p.count;
  if (left <= 0) return;
  unsigned next_unit = walk_first_unit(p);
  const WalkStage<0> stage0;
  const WalkStage<1> stage1;
  auto ask = [&](auto stage, int column, bool inside) {
    request(stage, next_unit, column, inside);
    ++next_unit;
  };
  ask(stage0, cb, true);
  while (left > 0) {
    const int row_length = walk_row_length(p, rb);
    const int n = row_length - cb < left ? row_length - cb : left;
    left -= n;
    row_begin(rb);
    ask(stage1, n > 1 ? cb + 1 : 0, n > 1 || left > 0);
    consume(stage0, true, rb, cb);
    int t = 1;
    for (; t + 1 < n; t += 2) {
      ask(stage0, cb + t + 1, true);
      consume(stage1, false, rb, cb + t);
      ask(stage1, t + 2 < n ? cb + t + 2 : 0, t + 2 < n || left > 0);
      consume(stage0, false, rb, cb + t + 1);
    }
    if (t < n) {
      ask(stage0, 0, left > 0);
      consume(stage1, false, rb, cb + t);
    } else {
      move();
    }
    row_end(rb);
    ++rb;
    cb = 0;
  }
}

}  // namespace tc
