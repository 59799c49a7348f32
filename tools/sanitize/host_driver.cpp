// Host-only exerciser of the library's planning / layout code for the sanitizer build
// (SURVEY.md section 5): g++ -fsanitize=address,undefined on hostmath.cpp + this file, no
// HIP.  Walks the same entry points the C ABI uses (bin permutation and segmentation,
// chunking, the quadratic-form layout / schedule / table fill / emulation, spline
// matrices, quadrature nodes, the fast-math tables, the pair counter's cell sort and label-block
// plan, the choice of the one-launch form, the slabs of a derivative call, the chunk plan and the
// chunks of a forward call, the LDS budgets and the node matching of a joint of interpolators)
// over a sweep of shapes
// and checks the results against direct evaluations.  Exit status 0 = all
// checks passed and no sanitizer report (-fno-sanitize-recover aborts on the first).
//
//   make -C tools/sanitize && tools/sanitize/host_driver
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <numeric>
#include <vector>

#include "../../tabcorr_amd/csrc/fastmath.h"
#include "../../tabcorr_amd/csrc/grad_call.h"
#include "../../tabcorr_amd/csrc/hostmath.h"
#include "../../tabcorr_amd/csrc/joint_interp.h"
#include "../../tabcorr_amd/csrc/kernel_args.h"
#include "../../tabcorr_amd/csrc/predict_call.h"

static int g_failures = 0;
#define EXPECT(condition, ...)                 \
  do {                                         \
    if (!(condition)) {                        \
      ++g_failures;                            \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

static void check_quadrature() {
  for (int n = 1; n <= 64; ++n) {
    std::vector<double> x, w;
    tc::gauss_legendre(n, x, w);
    double sum = 0.0, moment = 0.0;
    for (int k = 0; k < n; ++k) {
      sum += w[k];
      moment += w[k] * x[k];
      EXPECT(x[k] > 0.0 && x[k] < 1.0, "node outside (0, 1) for n = %d", n);
    }
    // numpy's leggauss weights (sum 2) with the nodes mapped to (0, 1): tabcorr.py:543-546
    EXPECT(std::fabs(sum - 2.0) < 1e-13, "weights of n = %d sum to %.17g", n, sum);
    EXPECT(std::fabs(moment - 1.0) < 1e-13, "first moment of n = %d", n);
  }
}

static void check_splines() {
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> uniform(0.1, 1.0);
  for (int n = 4; n <= 14; ++n) {
    std::vector<double> xp(n), y(n), a;
    xp[0] = -1.0;
    for (int i = 1; i < n; ++i) xp[i] = xp[i - 1] + uniform(rng);
    for (double& v : y) v = uniform(rng);
    EXPECT(tc::spline_interpolation_matrix(n, xp.data(), a), "singular spline system n = %d", n);
    EXPECT((int)a.size() == (n - 1) * 4 * n, "spline matrix size n = %d", n);
    // the spline passes through the nodes: segment s at xp[s] and xp[s + 1]
    for (int s = 0; s + 1 < n; ++s)
      for (int end = 0; end < 2; ++end) {
        const double x = xp[s + end];
        double value = 0.0;
        for (int p = 0; p < 4; ++p)
          for (int j = 0; j < n; ++j)
            value += a[((size_t)s * 4 + p) * n + j] * y[j] * std::pow(x, p);
        EXPECT(std::fabs(value - y[s + end]) < 1e-8, "spline n = %d segment %d: %g vs %g", n, s,
               value, y[s + end]);
      }
  }
  std::vector<double> a, three = {0.0, 1.0, 2.0};
  (void)tc::spline_interpolation_matrix(3, three.data(), a);   // too few nodes: must not crash
}

static void check_plans() {
  std::mt19937_64 rng(2);
  for (int mode = 0; mode < 2; ++mode)
    for (int n_bins : {1, 2, 3, 7, 16, 60, 100, 137, 200, 440}) {
      std::vector<uint8_t> central(n_bins);
      for (int g = 0; g < n_bins; ++g) central[g] = (rng() % 3) != 0;
      if (n_bins > 5) std::shuffle(central.begin(), central.end(), rng);
      for (int block : {tc::kF64Block, tc::kF32Block})
        for (int budget : {56, 128}) {
          tc::Plan plan;
          tc::build_plan(mode, n_bins, central.data(), block, budget, plan);
          const int64_t expect = mode == 0 ? (int64_t)n_bins * (n_bins + 1) / 2 : n_bins;
          EXPECT(plan.n_entries == expect, "plan entries %lld vs %lld", (long long)plan.n_entries,
                 (long long)expect);
          std::vector<int> seen((size_t)expect, 0);
          for (int64_t q = 0; q < plan.n_positions; ++q)
            if (plan.column[q] >= 0) {
              EXPECT(plan.column[q] < expect, "column out of range");
              ++seen[plan.column[q]];
            }
          for (int64_t p = 0; p < expect; ++p)
            EXPECT(seen[p] == 1, "mode %d bins %d: column %lld covered %d times", mode, n_bins,
                   (long long)p, seen[p]);
          for (int n_chunks : {1, 4, 13, 32, 100, 256}) {
            for (int waves : {4, 8}) {
              tc::Chunking chunking;
              tc::build_chunking(plan, n_chunks, waves, chunking);
              int64_t covered = 0;
              for (const tc::Chunk& chunk : chunking.chunks) {
                EXPECT(chunk.q_begin % block == 0, "chunk not block aligned");
                covered += chunk.q_end - chunk.q_begin;
              }
              EXPECT(covered == plan.n_positions, "chunks cover %lld of %lld positions",
                     (long long)covered, (long long)plan.n_positions);
            }
          }
        }
    }
}

static void check_quad() {
  std::mt19937_64 rng(3);
  std::normal_distribution<double> normal(0.0, 1.0);
  for (int n_bins : {1, 3, 4, 8, 13, 30, 100})
    for (int n_r : {1, 4, 19, 23, 45})
      for (int separate = 0; separate < 2; ++separate) {
        const int64_t n_pairs = (int64_t)n_bins * (n_bins + 1) / 2;
        std::vector<double> matrix((size_t)n_r * n_pairs);
        for (double& v : matrix) v = (float)std::exp(normal(rng));
        std::vector<uint8_t> central(n_bins);
        for (int g = 0; g < n_bins; ++g) central[g] = g % 3 != 1;
        tc::Plan plan;
        tc::build_plan(0, n_bins, central.data(), tc::kF64Block, 56, plan);
        const bool by_type = separate || plan.n_central % 4 == 0 || plan.n_central == n_bins;
        tc::QuadLayout layout;
        tc::build_quad_layout(n_bins, plan.n_central, by_type, layout);
        const tc::QuadTiling tiling = tc::quad_tiling(n_r);
        std::vector<double> table;
        tc::fill_quad_table(layout, plan.perm, n_r, n_pairs, matrix.data(), false, tiling, table);
        const int64_t n_draws = 70, ldb = 128;
        std::vector<double> densities((size_t)n_bins * ldb, 0.0);   // library bin order
        for (int g = 0; g < n_bins; ++g)
          for (int64_t b = 0; b < n_draws; ++b) densities[(size_t)g * ldb + b] = std::exp(normal(rng));
        for (int max_waves : {1, 7, 64, 2048}) {
          tc::QuadSchedule schedule;
          tc::build_quad_schedule(layout, (int)(ldb / 32), tiling.n_rtiles, 1, separate != 0,
                                  max_waves, 8, schedule);
          const int n_comp = separate ? 3 : 1;
          std::vector<double> out((size_t)n_draws * n_comp * n_r, 0.0);
          // with and without the workgroup-level merge of the slabs
          tc::QuadMergePlan merge;
          if (max_waves != 7)
            tc::merge_quad_schedule(layout, tiling.n_rtiles, separate != 0, tc::kQuadWavesPerBlock,
                                    max_waves == 64 ? 3 : 12, schedule, merge);
          tc::quad_emulate(layout, schedule, tiling, table, densities.data(), ldb, n_draws, n_r,
                           separate != 0, out.data(), max_waves != 7 ? &merge : nullptr);
          EXPECT(schedule.group_begin.back() == schedule.n_slabs, "slab count after the merge");
          // direct evaluation: sum_p c_p T[r][p] n_i n_j over the packed columns
          for (int64_t b = 0; b < n_draws; b += 23)
            for (int r = 0; r < n_r; ++r) {
              double expect[3] = {0.0, 0.0, 0.0};
              for (int i = 0; i < n_bins; ++i)
                for (int j = 0; j <= i; ++j) {
                  const int ri = plan.perm[i], rj = plan.perm[j];
                  const int hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
                  const double t = matrix[(size_t)r * n_pairs + tc::packed_index(hi, lo)];
                  const double w = (i == j ? 1.0 : 2.0) * densities[(size_t)i * ldb + b] *
                                   densities[(size_t)j * ldb + b];
                  const int ci = i < plan.n_central ? 0 : 1, cj = j < plan.n_central ? 0 : 1;
                  expect[separate ? ci + cj : 0] += t * w;
                }
              for (int c = 0; c < n_comp; ++c) {
                const double got = out[((size_t)b * n_comp + c) * n_r + r];
                EXPECT(std::fabs(got - expect[c]) <= 1e-11 * std::fabs(expect[c]) + 1e-300,
                       "quad emulate bins %d r %d sep %d waves %d: %g vs %g", n_bins, n_r, separate,
                       max_waves, got, expect[c]);
              }
            }
        }
      }
}

static void check_fastmath() {
  std::vector<double> table(tc::fm::kTableDoubles);
  tc::fm::build_tables(table.data());
  const tc::fm::Consts k = tc::fm::make_consts();
  double worst = 0.0;
  for (int i = -80000; i <= 80000; ++i) {
    const double x = i * 1e-4;
    worst = std::max(worst, std::fabs(tc::fm::erf_fast(table.data(), k, x) - std::erf(x)));
  }
  EXPECT(worst < 1e-15, "erf_fast deviates by %g", worst);
  for (int i = -3000; i <= 3000; ++i) {
    const double z = i * 0.1;
    const double got = tc::fm::exp2_fast(table.data(), k, z), expect = std::exp2(z);
    EXPECT(std::fabs(got / expect - 1.0) < 1e-15, "exp2_fast(%g)", z);
  }
  for (double y = 1e-300; y < 1e300; y *= 1.7) {
    const double got = tc::fm::log2_fast(table.data(), k, y), expect = std::log2(y);
    EXPECT(std::fabs(got - expect) <= 1e-15 * std::max(1.0, std::fabs(expect)), "log2_fast(%g)", y);
  }
  // out-of-range and non-finite arguments must stay inside the tables
  for (double x : {1e308, -1e308, HUGE_VAL, -HUGE_VAL, std::nan(""), 0.0, -0.0, 5e-324}) {
    (void)tc::fm::erf_fast(table.data(), k, x);
    (void)tc::fm::exp2_fast(table.data(), k, x);
    (void)tc::fm::exp10_fast(table.data(), k, x);
  }
}

static void check_cells() {
  std::mt19937_64 rng(4);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  // (250 000 points: the sorts run on several host threads)
  for (int64_t n : {0, 1, 17, 5000, 250000})
    for (int shape = 0; shape < 3; ++shape) {
      const double box[3] = {100.0, shape == 1 ? 45.0 : 100.0, shape == 2 ? 70.0 : 130.0};
      std::vector<double> pos((size_t)n * 3);
      std::vector<int32_t> label((size_t)n);
      for (int64_t p = 0; p < n; ++p) {
        for (int d = 0; d < 3; ++d) pos[3 * p + d] = uniform(rng) * box[d];
        label[p] = (int32_t)(rng() % 7);
      }
      if (n > 3) {
        pos[0] = 0.0;
        pos[4] = box[1];      // exactly on the upper face
        pos[8] = box[2];
      }
      const tc::CellGrid grid = tc::make_cell_grid(box, 20.0, 40.0, n);
      EXPECT(grid.nx >= 1 && grid.ny >= 1 && grid.nz >= 1, "empty grid");
      EXPECT((grid.ny == 1) == (grid.reach_y == 0), "reach does not match the cell count");
      // neighbour cells to each side are distinct cells and cover the reach
      EXPECT(grid.nx >= 2 * grid.reach_x + 1 && grid.ny >= 2 * grid.reach_y + 1 &&
                 grid.nz >= 2 * grid.reach_z + 1, "neighbour cells alias");
      EXPECT(grid.reach_x == 0 || grid.lx / grid.nx * grid.reach_x >= 20.0, "x cells too narrow");
      EXPECT(grid.reach_z == 0 || grid.lz / grid.nz * grid.reach_z >= 40.0, "z cells too narrow");
      tc::CellSort sorted;
      EXPECT(tc::sort_into_cells(grid, pos.data(), label.data(), n, sorted) == -1,
             "points reported outside the box");
      EXPECT((int64_t)sorted.x.size() == n && sorted.cell_start.back() == n, "cell sort lost points");
      for (int c = 0; c < grid.n_cells(); ++c)
        for (int32_t s = sorted.cell_start[c]; s < sorted.cell_start[c + 1]; ++s) {
          const int cx = std::min(grid.nx - 1, (int)(sorted.x[s] / grid.lx * grid.nx));
          EXPECT(cx == c / (grid.ny * grid.nz), "point in the wrong cell");
        }
      {
        // stable: with the input index as label, the points of a cell keep their input order
        // (whatever the number of threads), and sorting by that label changes nothing
        std::vector<int32_t> index((size_t)n);
        std::iota(index.begin(), index.end(), 0);
        tc::CellSort by_index;
        EXPECT(tc::sort_into_cells(grid, pos.data(), index.data(), n, by_index) == -1,
               "points reported outside the box");
        EXPECT(by_index.cell_start == sorted.cell_start && by_index.x == sorted.x,
               "cell sort depends on the labels");
        for (int c = 0; c < grid.n_cells(); ++c)
          for (int32_t s = by_index.cell_start[c] + 1; s < by_index.cell_start[c + 1]; ++s)
            EXPECT(by_index.label[s - 1] < by_index.label[s], "cell sort is not stable");
        const std::vector<double> before = by_index.z;
        tc::sort_cells_by_label(by_index);
        EXPECT(by_index.z == before, "label sort moved points that were in order");
      }
      // labelled work items: sorted by label inside the cells, bounded points and labels
      const tc::CellSort unsorted = sorted;
      tc::sort_cells_by_label(sorted);
      for (int c = 0; c < grid.n_cells(); ++c) {
        // (stable inside a label: equal labels keep the order they had in the cell)
        std::vector<int32_t> order((size_t)(sorted.cell_start[c + 1] - sorted.cell_start[c]));
        std::iota(order.begin(), order.end(), sorted.cell_start[c]);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
          return unsorted.label[a] < unsorted.label[b];
        });
        for (size_t k = 0; k < order.size(); ++k)
          EXPECT(sorted.x[sorted.cell_start[c] + k] == unsorted.x[order[k]] &&
                     sorted.label[sorted.cell_start[c] + k] == unsorted.label[order[k]],
                 "label sort differs from a stable sort");
      }
      for (int c = 0; c < grid.n_cells(); ++c)
        for (int32_t s = sorted.cell_start[c] + 1; s < sorted.cell_start[c + 1]; ++s)
          EXPECT(sorted.label[s - 1] <= sorted.label[s], "labels not sorted inside a cell");
      for (int block : {1, 3, 8}) {
        tc::LabelBlocks blocks;
        tc::build_label_blocks(sorted, 7, block, blocks);
        EXPECT(blocks.n_blocks == (7 + block - 1) / block, "number of label blocks");
        const size_t stride = (size_t)blocks.n_blocks + 1;
        int64_t covered = 0;
        for (int c = 0; c < grid.n_cells(); ++c) {
          EXPECT(blocks.start[c * stride] == sorted.cell_start[c] &&
                     blocks.start[c * stride + blocks.n_blocks] == sorted.cell_start[c + 1],
                 "label blocks do not span the cell");
          for (int k = 0; k < blocks.n_blocks; ++k) {
            EXPECT(blocks.start[c * stride + k] <= blocks.start[c * stride + k + 1],
                   "label block offsets decrease");
            for (int32_t p = blocks.start[c * stride + k]; p < blocks.start[c * stride + k + 1];
                 ++p) {
              EXPECT(sorted.label[p] / block == k, "point in the wrong label block");
              ++covered;
            }
          }
        }
        EXPECT(covered == n, "label blocks cover %lld of %lld points", (long long)covered,
               (long long)n);
        // work units: every (block, block, cell) exactly once
        for (int target : {1, 40, 4096}) {
          tc::PairUnits units;
          tc::build_pair_units(grid, sorted, sorted, blocks.n_blocks, blocks.n_blocks, target,
                               units);
          std::vector<int> seen((size_t)blocks.n_blocks * blocks.n_blocks * grid.n_cells(), 0);
          for (size_t u = 0; u < units.block1.size(); ++u) {
            EXPECT(units.cell_begin[u] < units.cell_end[u] && units.cell_end[u] <= grid.n_cells(),
                   "unit cell range");
            for (int c = units.cell_begin[u]; c < units.cell_end[u]; ++c)
              ++seen[((size_t)units.block1[u] * blocks.n_blocks + units.block2[u]) *
                         grid.n_cells() + c];
          }
          for (int v : seen) EXPECT(v == 1, "a (block, block, cell) is covered %d times", v);
        }
      }
      if (n > 0) {
        pos[2] = -1.0;
        EXPECT(tc::sort_into_cells(grid, pos.data(), nullptr, n, sorted) == 0,
               "point outside the box not reported");
      }
    }
}

// hostmath.h: plan_label_blocks over bins up to the limit and labels up to the C ABI's 4096:
// blocks that cover the labels, counters within the limit always and within the budget until
// nothing is left to shrink, and a cell sort cut by the planned blocks.
static void check_label_block_plan() {
  const int limit = tc::kPairLdsLimit;
  std::vector<int> bins;
  for (double b = 1.0; b < limit; b *= 1.37) bins.push_back((int)b);
  for (int b : {19, 64, 80, 3840, 6782, 6783, 7200, 7680, 7681, 7744, 13564, 13565, 15359, 15360})
    bins.push_back(b);
  for (int budget_kb : {30, 8, 60})
    for (int n_bin : bins)
      for (int n_labels : {1, 2, 3, 7, 8, 9, 50, 51, 70, 71, 100, 4096}) {
        const int budget = budget_kb * 1024 / 4;
        const tc::LabelBlockPlan plan = tc::plan_label_blocks(n_bin, n_labels, budget, limit);
        const int64_t counters = (int64_t)n_bin * plan.block1 * plan.block2;
        EXPECT(plan.block1 >= 1 && plan.block1 <= n_labels && plan.block2 >= 1 &&
                   plan.block2 <= std::min(n_labels, 8),
               "%d bins, %d labels: blocks of %d and %d labels", n_bin, n_labels, plan.block1,
               plan.block2);
        EXPECT(counters <= limit, "%d bins, %d labels: %lld counters", n_bin, n_labels,
               (long long)counters);
        EXPECT(counters <= budget || (plan.block1 == 1 && plan.block2 <= 2),
               "%d bins, %d labels: %lld counters over the budget with blocks of %d and %d", n_bin,
               n_labels, (long long)counters, plan.block1, plan.block2);
      }
  // the planned blocks cut a sorted point set: every label in exactly one block per side
  std::mt19937_64 rng(6);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  const double box[3] = {100.0, 100.0, 100.0};
  for (int n_labels : {3, 51, 71}) {
    const int64_t n = 2000;
    std::vector<double> pos((size_t)n * 3);
    std::vector<int32_t> label((size_t)n);
    for (int64_t p = 0; p < n; ++p) {
      for (int d = 0; d < 3; ++d) pos[3 * p + d] = uniform(rng) * box[d];
      label[p] = (int32_t)(rng() % n_labels);
    }
    const tc::CellGrid grid = tc::make_cell_grid(box, 20.0, 20.0, n);
    tc::CellSort sorted;
    EXPECT(tc::sort_into_cells(grid, pos.data(), label.data(), n, sorted) == -1, "outside");
    tc::sort_cells_by_label(sorted);
    for (int n_bin : {64, 80, 7200, 7744}) {
      const tc::LabelBlockPlan plan =
          tc::plan_label_blocks(n_bin, n_labels, tc::kPairLdsBudgetKB * 1024 / 4, limit);
      for (int block : {plan.block1, plan.block2}) {
        tc::LabelBlocks blocks;
        tc::build_label_blocks(sorted, n_labels, block, blocks);
        EXPECT(blocks.n_blocks * block >= n_labels && (blocks.n_blocks - 1) * block < n_labels,
               "%d blocks of %d labels for %d labels", blocks.n_blocks, block, n_labels);
        const size_t stride = (size_t)blocks.n_blocks + 1;
        for (int c = 0; c < grid.n_cells(); ++c)
          for (int k = 0; k < blocks.n_blocks; ++k)
            for (int32_t p = blocks.start[c * stride + k]; p < blocks.start[c * stride + k + 1]; ++p)
              EXPECT(sorted.label[p] / block == k, "point in the wrong label block");
      }
    }
  }
}

// hostmath.h: choose_fused_form over a few thousand queries, degenerate ones included (zero
// draws, no nodes, tables without centrals or satellites, no layouts at all): a form the
// instances exist for, an LDS footprint within the CU's, and the same answer twice.
static void check_fused_form() {
  std::mt19937_64 rng(5);
  auto pick = [&](std::initializer_list<int> values) {
    return *(values.begin() + rng() % values.size());
  };
  tc::AutoChoice choice;
  for (int i = 0; i < tc::AutoChoice::kSizes; ++i) {
    choice.form[i] = pick({0, 32, 64});
    for (int k = 0; k < 3; ++k) choice.us[i][k] = (float)(rng() % 4) * 7.5f;
  }
  int one_launch = 0;
  for (int n = 0; n < 6000; ++n) {
    const int n_bins = pick({1, 3, 8, 60, 100, 104, 108, 208, 212, 248, 252, 440});
    const int n_central = pick({0, n_bins / 2, n_bins / 2, n_bins / 2 + 1, n_bins});
    const int n_r = pick({1, 3, 19, 20, 21, 45});
    const tc::QuadTiling tiling = tc::quad_tiling(n_r);
    tc::QuadLayout total, by_type;
    tc::FusedQuery q;
    if (n % 17 != 0) {                  // (else: a handle without the quadratic-form layouts)
      tc::build_quad_layout(n_bins, std::min(n_central, n_bins), true, by_type);
      tc::build_quad_layout(n_bins, std::min(n_central, n_bins), false, total);
      q.servable = tiling.n_rtiles == 1 && n_r <= 20;
    }
    q.n_bins = n_bins;
    q.n_u = tiling.n_u;
    q.n_cus = pick({256, 64, 1});
    q.grouped = rng() % 4 == 0;
    q.units_total = total.n_units;
    q.units_by_type = by_type.n_units;
    q.rows_total = tc::fused_dens_rows(total);
    q.rows_by_type = tc::fused_dens_rows(by_type);
    q.by_type_complete = by_type.comps.size() == 3;
    for (const tc::QuadComp& comp : by_type.comps) q.by_type_complete &= comp.n_units > 0;
    q.n_draws = pick({0, 1, 255, 2048, 8192, 10000, 16384, 30721, 1 << 30});
    q.n_gauss = pick({0, 1, 10, 10, 10, 12});
    q.flags = (unsigned)pick({0, 0, 1, 2, 4, 16, 18, 23, 31});
    q.alone = rng() % 2;
    q.async = rng() % 3 == 0;
    q.sync_spread = rng() % 4 == 0;
    q.chain = rng() % 16 == 0;
    q.trace = rng() % 16 == 0;
    q.likelihood = rng() % 4 == 0;
    q.fused = pick({0, 1, 1, 2});
    q.fused_min_draws = pick({0, 0, 1, 5000});
    q.fused_max_draws = pick({30720, 0, 1 << 30});
    q.fused_waves = pick({0, 0, 8, 16});
    q.fused_draws = pick({0, 0, 32, 40, 64});
    q.fused_spread = rng() % 4 != 0;
    q.fused_spread_min = pick({8192, 0, 1});
    q.fused_spread_rounds = pick({1, 2, 0, -1});
    q.deterministic = pick({0, 0, 1, 2});
    q.measured = rng() % 3 == 0 ? &choice : nullptr;
    const tc::FusedForm form = tc::choose_fused_form(q);
    const tc::FusedForm again = tc::choose_fused_form(q);
    EXPECT(form.waves == again.waves && form.draws == again.draws, "the decision is not a function");
    if (form.waves == 0) {
      EXPECT(form.draws == 0, "three kernels with %d draws per workgroup", form.draws);
      continue;
    }
    ++one_launch;
    EXPECT(q.servable && q.fused != 0 && q.n_gauss >= 1, "one launch for a table it cannot serve");
    EXPECT((form.waves == 8 && (form.draws == 64 || form.draws == 32 || form.draws == 40)) ||
               (form.waves == 16 && form.draws == 64),
           "no instance of %d waves x %d draws", form.waves, form.draws);
    const int rows = (q.flags & tc::kFlagSeparate) ? q.rows_by_type : q.rows_total;
    const int lds = tc::fused_lds_bytes(rows, form.waves, form.draws);
    EXPECT(rows >= n_bins && lds <= 160 * 1024, "%d bins: %d rows, %d bytes of LDS", n_bins, rows, lds);
  }
  EXPECT(one_launch > 300, "only %d queries took a one-launch form", one_launch);
}

// The slab arithmetic of the derivative entry points (grad_call.h: GradRequest::slab) against the
// closed forms, up to products far beyond 2^31 elements: every one of them in 64 bits.
static void check_grad_slabs() {
  const int64_t begins[] = {0, 1, 1 << 18, (1 << 18) + 17, ((int64_t)1 << 31) - 1,
                            (int64_t)1 << 31, ((int64_t)1 << 31) + 5, ((int64_t)1 << 33) + 3};
  for (int n_params : {tc::kGradParams, tc::kGradParamsAssembias, tc::kGradParamsLeauthaud11})
    for (int n_extra : {0, 1, 3})
      for (int n_r : {1, 2, 19, 38, 1000})
        for (int likelihood = 0; likelihood < 2; ++likelihood)
          for (int64_t begin : begins) {
            int64_t at[7];
            tc::host::grad_slab_offsets(n_params, n_extra, n_r, likelihood != 0, begin, at);
            const int64_t cols = n_params + n_extra, wide = likelihood ? 1 : n_r;
            EXPECT(at[0] == begin * tc::grad_theta_columns(n_params) &&
                       at[1] == (n_extra ? begin * n_extra : -1) && at[2] == begin &&
                       at[3] == begin * cols && at[4] == begin * wide &&
                       at[5] == begin * cols * wide &&
                       at[6] == (likelihood ? begin * cols * cols : -1),
                   "slab offsets of %d + %d columns, %d rows, likelihood %d at draw %lld", n_params,
                   n_extra, n_r, likelihood, (long long)begin);
          }
}

// The completeness rules of the occupation seam (grad_call.h: vjp_incomplete) on listed cases per
// handle kind, written out from the entries' documentation and not from the function: the arrays
// that are there by letter -- o occupation, n ngal, v xi, c chi2, x x, g g_xi, G g_occupation
// (dchi2_docc), X g_x (dchi2_dx), D dngal_dx -- and what the call is told: nothing (complete), a
// NULL pointer, or the kind's words for adjoint arrays that go together.
static void check_vjp_rules() {
  using tc::host::VjpRequest;
  using tc::host::VjpRule;
  static double anchor[1];
  enum { kTable, kJoint, kInterp };
  const VjpRule rules[3] = {{false, false, {nullptr, nullptr}},
                            {false, true, {"pair", nullptr}},
                            {true, true, {"triple", "chi2 triple"}}};
  const char* const null = "NULL pointer";
  const struct Case { int kind; bool likelihood, operands; const char* there; const char* told; }
  cases[] = {
      // a table: every adjoint array of the form is required
      {kTable, false, true, "onvgG", nullptr}, {kTable, false, true, "onvG", null},
      {kTable, false, true, "onvg", null},     {kTable, false, true, "onv", null},
      {kTable, false, true, "nvgG", null},     {kTable, false, true, "ovgG", null},
      {kTable, false, true, "ongG", null},     {kTable, false, true, "oncgG", null},
      {kTable, true, true, "oncG", nullptr},   {kTable, true, true, "onc", null},
      {kTable, true, false, "oncG", null},     {kTable, true, true, "onvG", null},
      // a joint: g_xi and g_occupation together, both NULL the forward-only form; the likelihood
      // form has dchi2_docc alone, there or not
      {kJoint, false, true, "onvgG", nullptr}, {kJoint, false, true, "onv", nullptr},
      {kJoint, false, true, "onvg", "pair"},   {kJoint, false, true, "onvG", "pair"},
      {kJoint, false, true, "ovgG", null},     {kJoint, false, true, "ong", null},
      {kJoint, true, true, "oncG", nullptr},   {kJoint, true, true, "onc", nullptr},
      {kJoint, true, false, "onc", null},      {kJoint, true, true, "ncG", null},
      // an interpolator: x required; the triples together
      {kInterp, false, true, "onvxgGX", nullptr},    {kInterp, false, true, "onvx", nullptr},
      {kInterp, false, true, "onvxgG", "triple"},    {kInterp, false, true, "onvxX", "triple"},
      {kInterp, false, true, "onvxgX", "triple"},    {kInterp, false, true, "onvxGXD", "triple"},
      {kInterp, false, true, "onvgGX", null},        {kInterp, false, true, "onxgGX", null},
      {kInterp, true, true, "oncxGXD", nullptr},     {kInterp, true, true, "oncx", nullptr},
      {kInterp, true, true, "oncxGX", "chi2 triple"}, {kInterp, true, true, "oncxD", "chi2 triple"},
      {kInterp, true, true, "oncxgG", "chi2 triple"}, {kInterp, true, true, "oncGXD", null},
      {kInterp, true, false, "oncxGXD", null},       {kInterp, true, true, "onvxGXD", null},
  };
  for (const Case& c : cases) {
    const auto at = [&](char letter) { return std::strchr(c.there, letter) ? anchor : nullptr; };
    VjpRequest r{};
    r.occupation = at('o'), r.ngal = at('n'), r.xi = at('v'), r.chi2 = at('c'), r.x = at('x');
    r.g_xi = at('g'), r.g_occupation = at('G'), r.g_x = at('X'), r.dngal_dx = at('D');
    const char* got = tc::host::vjp_incomplete(rules[c.kind], r, c.likelihood, c.operands);
    EXPECT((got == nullptr) == (c.told == nullptr) &&
               (got == nullptr || std::strcmp(got, c.told) == 0),
           "seam rule of kind %d, likelihood %d, arrays %s: %s", c.kind, c.likelihood, c.there,
           got ? got : "complete");
  }
}

// hostmath.h: plan_sync_chunks over the sweep of tests/test_predict_call_cpu.py: boundaries from 0
// to n_draws, strictly increasing, inner ones multiples of 64, at most 64 chunks, never staggered
// for an interpolator or a likelihood; and the chunk arithmetic of the forward entry points
// (predict_call.h: PredictRequest::chunk) against the closed forms beyond 2^31 elements.
static void check_forward_calls() {
  int planned = 0, staggered = 0;
  for (int64_t n_draws : {0, 1, 63, 64, 65, 100, 2047, 2048, 4096, 5013, 9037, 10000, 400000})
    for (int sync_chunks : {-1, 0, 1, 2, 3, 7, 8, 64})
      for (int sync_stagger : {0, 1, 10, 50, 100})
        for (int doubles : {8, 20, 257, 761})
          for (int bits = 0; bits < 32; ++bits) {
            tc::SyncChunkQuery q;
            q.n_draws = n_draws;
            q.out_bytes_per_draw = 8 * doubles;
            q.likelihood = bits & 1;
            q.second_cols = q.likelihood ? 1 : doubles - 1;
            q.sync_chunks = sync_chunks;
            q.sync_stagger = sync_stagger;
            q.n_lanes = bits & 2 ? 4 : 1;
            q.float32 = bits & 4;
            q.interpolator = bits & 8;
            q.cross = bits & 16;
            const tc::SyncChunkPlan plan = tc::plan_sync_chunks(q);
            EXPECT(plan.n_chunks >= 0 && plan.n_chunks <= 64, "%d chunks", plan.n_chunks);
            if (plan.n_chunks == 0) {
              EXPECT(!plan.staggered, "a staggered serial call");
              continue;
            }
            ++planned;
            staggered += plan.staggered;
            EXPECT(q.n_lanes >= 2 && sync_chunks >= 0, "chunks on the serial path");
            EXPECT(!plan.staggered || (!q.interpolator && !q.likelihood && q.float32),
                   "a staggered plan where none belongs");
            EXPECT(plan.begins[0] == 0 && plan.begins[plan.n_chunks] == n_draws,
                   "%lld draws: chunks from %lld to %lld", (long long)n_draws,
                   (long long)plan.begins[0], (long long)plan.begins[plan.n_chunks]);
            for (int k = 1; k <= plan.n_chunks; ++k) {
              EXPECT(plan.begins[k] > plan.begins[k - 1], "%lld draws: chunk %d is empty",
                     (long long)n_draws, k - 1);
              EXPECT(k == plan.n_chunks || plan.begins[k] % 64 == 0, "boundary %lld",
                     (long long)plan.begins[k]);
            }
          }
  EXPECT(planned > 5000 && staggered > 50, "%d plans, %d staggered", planned, staggered);

  // (chunk() on arrays that exist, so that every chunk lies inside them; the byte counts, which
  // are plain integers, up to 2^33 draws: every product in 64 bits)
  const int64_t n_whole = 4096;
  for (int n_extra : {0, 2})
    for (int form = 0; form < 3; ++form)          // total, separated by galaxy type, likelihood
      for (int n_r : {1, 19, 256}) {
        const int n_theta = 5, n_comp = 3;
        const int64_t ngal_cols = form == 1 ? 2 : 1;
        const int64_t second_cols = form == 2 ? 1 : (int64_t)(form == 1 ? n_comp : 1) * n_r;
        std::vector<double> theta(n_whole * n_theta), x(n_whole * n_extra + 1),
            ngal(n_whole * ngal_cols), second(n_whole * second_cols);
        const tc::host::PredictRequest whole{
            n_theta, n_extra, 10, form == 1 ? (unsigned)TC_FLAG_SEPARATE_GAL_TYPE : 0u, n_whole, n_r,
            n_comp, theta.data(), n_extra ? x.data() : nullptr, ngal.data(), second.data(),
            form == 2};
        EXPECT((int64_t)whole.in_bytes() == n_whole * (n_theta + n_extra) * 8 &&
                   (int64_t)whole.out_bytes() == n_whole * (ngal_cols + second_cols) * 8,
               "bytes of form %d", form);
        for (int64_t begin : {(int64_t)0, (int64_t)1, (int64_t)64, (int64_t)1409, n_whole - 81}) {
          const tc::host::PredictRequest part = whole.chunk(begin, 81);
          EXPECT(part.n_draws == 81 && part.theta - whole.theta == begin * n_theta &&
                     (n_extra ? part.x - whole.x == begin * n_extra : part.x == nullptr) &&
                     part.ngal - whole.ngal == begin * ngal_cols &&
                     part.second - whole.second == begin * second_cols &&
                     (int64_t)part.ngal_count() == 81 * ngal_cols &&
                     (int64_t)part.second_count() == 81 * second_cols,
                 "chunk of form %d, %d extra columns, %d rows at draw %lld", form, n_extra, n_r,
                 (long long)begin);
        }
        tc::host::PredictRequest huge = whole;
        huge.n_draws = ((int64_t)1 << 33) + 3;
        EXPECT(huge.theta_bytes() == (size_t)huge.n_draws * n_theta * 8 &&
                   huge.x_bytes() == (size_t)huge.n_draws * n_extra * 8 &&
                   huge.second_count() == (size_t)huge.n_draws * second_cols &&
                   huge.out_bytes() == (size_t)huge.n_draws * (ngal_cols + second_cols) * 8,
               "64-bit sizes of form %d", form);
      }
}

// joint_interp.h: the LDS budgets of both forms against the interpolator kernels' own with N rows,
// and joint_interp_permutation on shuffled grids of one to three axes: every walk position finds
// the member's table at its node, and a member with a node twice (another one missing) is refused.
static void check_joint_interp() {
  for (int n_params : {tc::kGradParams, tc::kGradParamsAssembias})
    for (int n_dim : {1, 2, tc::kGradMaxDim})
      for (int n_bins : {1, 18, 100, 1104})
        for (int n_r_total : {1, 8, 26, 38}) {
          const int n_central = n_bins / 2;
          const size_t row = (size_t)tc::kGradDraws * sizeof(double);
          EXPECT(tc::joint_interp_lds_bytes(tc::kJointInterpSlabs, n_bins, n_central, n_r_total,
                                            n_r_total, n_dim, n_params) ==
                     tc::grad_interp_cross_lds_bytes(n_r_total, n_dim, false, n_params),
                 "slab budget of %d rows", n_r_total);
          for (int n_r_cross : {0, 1, n_r_total - 1}) {
            if (n_r_cross < 0 || n_r_cross >= n_r_total) continue;
            EXPECT(tc::joint_interp_lds_bytes(tc::kJointInterpRows, n_bins, n_central, n_r_total,
                                              n_r_cross, n_dim, n_params) ==
                       tc::grad_interp_auto_lds_bytes(n_bins, n_central, n_r_total, n_dim, false,
                                                      n_params) +
                           (size_t)(n_params + 1 + n_dim) * n_r_cross * row,
                   "rows budget of %d bins, %d rows, %d cross", n_bins, n_r_total, n_r_cross);
          }
        }
  const int modes[3] = {TC_MODE_CROSS, TC_MODE_AUTO, TC_MODE_CROSS};
  EXPECT(tc::joint_interp_form(modes, 3) == tc::kJointInterpRows &&
             tc::joint_interp_form(modes, 1) == tc::kJointInterpSlabs &&
             tc::joint_interp_form(modes + 2, 1) == tc::kJointInterpSlabs,
         "form by the members' modes");
  std::mt19937_64 rng(8);
  const int axis[3] = {4, 5, 3};
  for (int n_dim = 1; n_dim <= 3; ++n_dim) {
    int n_tables = 1;
    for (int d = 0; d < n_dim; ++d) n_tables *= axis[d];
    std::vector<int32_t> node0((size_t)n_tables * n_dim);
    for (int k = 0; k < n_tables; ++k) {
      int rest = k;
      for (int d = 0; d < n_dim; ++d) {
        node0[(size_t)k * n_dim + d] = rest % axis[d];
        rest /= axis[d];
      }
    }
    std::vector<int32_t> walk0(n_tables), order(n_tables), found(n_tables);
    std::iota(walk0.begin(), walk0.end(), 0);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(walk0.begin(), walk0.end(), rng);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<int32_t> node((size_t)n_tables * n_dim);
    for (int k = 0; k < n_tables; ++k)
      for (int d = 0; d < n_dim; ++d)
        node[(size_t)k * n_dim + d] = node0[(size_t)order[k] * n_dim + d];
    EXPECT(tc::joint_interp_permutation(n_tables, n_dim, walk0.data(), node0.data(), node.data(),
                                        found.data()),
           "a shuffled member of %d axes is refused", n_dim);
    for (int s = 0; s < n_tables; ++s)
      EXPECT(order[found[s]] == walk0[s], "walk position %d finds table %d", s, found[s]);
    for (int d = 0; d < n_dim; ++d) node[d] = node[n_dim + d];
    EXPECT(!tc::joint_interp_permutation(n_tables, n_dim, walk0.data(), node0.data(), node.data(),
                                         found.data()),
           "a member with a node twice is accepted");
  }
}

int main() {
  check_joint_interp();
  check_forward_calls();
  check_grad_slabs();
  check_vjp_rules();
  check_quadrature();
  check_splines();
  check_plans();
  check_quad();
  check_fastmath();
  check_cells();
  check_label_block_plan();
  check_fused_form();
  if (g_failures != 0) {
    printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  printf("host sanitizer driver: all checks passed\n");
  return 0;
}
