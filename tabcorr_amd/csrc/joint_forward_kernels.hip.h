// Joint forward kernel: (ngal, xi) or (ngal, chi2) of a batch of draws for SEVERAL tables that
// share one halo table, in one launch (joint.h: the argument block and the LDS budget; joint.cpp
// fills it in).  The forward counterpart of grad_joint_kernel, composed of the pieces of
// predict_fused_kernel (kernels.hip.h): a workgroup of kJointForwardWaves waves carries
// kJointForwardDraws = 64 draws, two tiles of 32, from theta to the results.
//   1  once per workgroup: the occupations of every bin (lane = draw, the bins strided over the
//      waves: draw_params, occ_bin_zheng07) into the LDS density array dens[bin][64], and ngal;
//   2  per table in list order, into its rows r_offset[t] .. of the N concatenated ones:
//      mode auto   the table's own unit layout of the packed triangle on v_mfma_f64_16x16x4_f64
//                  (fused_quad_pass over fused_walk.h).  A PASS is (table, pair of r sub-tiles,
//                  part of the triangle, tile of 32 draws); the passes of ALL auto tables are
//                  numbered through the list and dealt to the waves (wave, wave + 8, ...), so
//                  that a table of 3 r bins leaves no wave idle.  A pass leaves its sums in its
//                  part's slab of `sums`;
//      mode cross  xi_r = T_r . dens / ngal: ONE fma chain per (r, draw) over the bins in
//                  library order; the rows of all cross tables are numbered through the list and
//                  dealt to the waves behind the last pass.  A row's sum goes to part 0;
//   3  per row the parts in part order, normalised (auto by ngal^2, cross by ngal, by division)
//      into the results tile (N, 65), then tile_write_xi, or chi2 = delta^T P delta: wave w sums
//      the rows i = w, w + 8, ... of delta_i (P delta)_i, wave 0 adds the waves' sums in wave
//      order -- every thread of the workgroup works, the order of addition is fixed.
// Order guarantees: ONE form; a draw's results depend on the draw alone (the occupations' per-lane
// rules, a matrix product whose columns do not mix, per-lane chains); the arithmetic of a row
// does not depend on the wave that runs it; ngal does not depend on the tables at all.
#pragma once

#include "joint.h"
#include "kernels.hip.h"

namespace tc {

// The end of step 3, behind the barrier that follows the results tile (N, 65) -- shared with
// joint_interp_forward_kernel: tile_write_xi of the workgroup's valid draws, or (chi2 != NULL)
// chi2 = delta^T P delta for the lane's draw (as predict_fused_kernel) against `operands` in
// LDS, data (N) then the precision matrix (N, N): wave w sums the rows i = w, w + 8, ... into
// red[w], wave 0 adds the waves' sums in wave order.
__device__ __forceinline__ void joint_forward_results(
    const double (*tile)[kLanes + 1], const double* operands,
    double (*red)[kLanes], int n_total, int64_t col, int64_t n_draws, double* xi, double* chi2) {
  constexpr int W = kJointForwardWaves, DL = kJointForwardDraws;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_valid = n_draws - col < DL ? n_draws - col : DL;
  if (chi2 != nullptr) {
    const double* data = operands;
    const double* matrix = operands + n_total;
    double part = 0.0;
    for (int i = wave; i < n_total; i += W) {
      double inner = 0.0;
      for (int j = 0; j < n_total; ++j)
        inner = fma(matrix[i * n_total + j], tile[j][lane] - data[j], inner);
      part = fma(tile[i][lane] - data[i], inner, part);
    }
    red[wave][lane] = part;
    __syncthreads();
    if (wave == 0 && lane < n_valid) {
      double total = 0.0;
      for (int w = 0; w < W; ++w) total += red[w][lane];
      chi2[col + lane] = total;
    }
    return;
  }
  tile_write_xi(&tile[0][0], n_total, DL, n_valid, xi + col * (int64_t)n_total, n_total, 0);
}

template <int NGAUSS, bool ASSEMBIAS, bool MODULATE>
__global__ __launch_bounds__(64 * kJointForwardWaves) void joint_forward_kernel(
    const JointForwardArgs a) {
  constexpr int W = kJointForwardWaves, DL = kJointForwardDraws;
  constexpr int PARTS = joint_forward_parts(W);
  extern __shared__ __attribute__((aligned(16))) double joint_forward_lds[];
  const int n_total = a.n_r;
  const int tile_doubles = (n_total * (kLanes + 1) + 1) / 2 * 2;
  const int region_b = a.dens_rows * DL > tile_doubles ? a.dens_rows * DL : tile_doubles;
  const int operand_doubles = n_total * (n_total + 1);
  const int region_a = fm::kTableDoubles > operand_doubles ? fm::kTableDoubles : operand_doubles;
  double* dens = joint_forward_lds;                       // later the results tile
  double* table = dens + region_b;                        // later data | precision
  double(*red)[W][kLanes] = (double(*)[W][kLanes])(table + region_a);
  double* sums = table + region_a + 2 * W * kLanes;       // (PARTS, N, 64)
  const fm::Consts kc = fm::make_consts();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_gauss = NGAUSS > 0 ? NGAUSS : a.n_gauss;

  stage_math_table(table, a.math_table);
  for (int idx = a.n_bins * DL + threadIdx.x; idx < a.dens_rows * DL; idx += blockDim.x)
    dens[idx] = 0.0;
  __syncthreads();

  // ---- 1. occupations (as predict_fused_kernel, 64 draws, per bin, no expansions) ----
  const int64_t col = (int64_t)blockIdx.x * DL;
  const int64_t b0 = col + lane;
  const int64_t b = b0 < a.n_draws ? b0 : a.n_draws - 1;
  double ngal;
  {
    DrawParams dp = draw_params<ASSEMBIAS>(table, kc, a.theta + b * a.n_theta);
    series_setup<MODULATE>(dp, false, false);
    sc_f64 log_m = (sc_f64)a.log_m;
    sc_f64 mass = (sc_f64)a.m;
    sc_f64 weight = (sc_f64)a.weight;
    sc_f64 weight_sum = weight + a.n_bins * n_gauss;   // (get_quadrature: the bins' sums)
    sc_f64 n_h = (sc_f64)a.n_h;
    sc_f64 percentile = (sc_f64)a.percentile;
    const double f1 = (1.0 - a.split) / a.split, f2 = a.split / (1.0 - a.split);
    double sum_cen = 0.0, sum_sat = 0.0;
    for (int g = wave; g < a.n_bins; g += W) {
      const bool central = g < a.n_central;
      const bool above = ASSEMBIAS ? percentile[g] > a.split : false;
      const double acc = occ_bin_zheng07<NGAUSS, ASSEMBIAS, MODULATE>(
          table, kc, g, n_gauss, central, above, log_m, mass, weight, weight_sum, dp, f1, f2);
      const double value = acc * n_h[g];
      dens[g * DL + lane] = value;
      if (central) sum_cen += value; else sum_sat += value;
    }
    red[0][wave][lane] = sum_cen;
    red[1][wave][lane] = sum_sat;
    __syncthreads();
    double n_cen = 0.0, n_sat = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      n_cen += red[0][w][lane];
      n_sat += red[1][w][lane];
    }
    ngal = n_cen + n_sat;
    if (wave == 0 && b0 < a.n_draws) a.ngal[b0] = ngal;
  }
  // (the math table is dead: the likelihood's operands take its place)
  if (a.chi2 != nullptr)
    for (int idx = threadIdx.x; idx < operand_doubles; idx += blockDim.x)
      table[idx] = a.chi2_data[idx];

  // ---- 2. the tables ----
  const int c = lane & 15, kq = lane >> 4;
  const int n_jobs = a.job_begin[a.n_tables];
  for (int job = wave; job < n_jobs; job += W) {
    int t = 0;
    while (job >= a.job_begin[t + 1]) ++t;
    // pass (pair p, part, tile) of table t: the pairs outermost, so that eight consecutive passes
    // -- one per wave -- are the (part, tile) combinations of one pair
    const int local = job - a.job_begin[t];
    const int p = local / (2 * PARTS), part = local / 2 % PARTS, sub = local % 2;
    const int n_u = a.n_u[t], up = (n_u + 1) / 2;
    const __amdgpu_buffer_rsrc_t rs_t =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.matrix[t], 0, a.table_bytes[t], kBufferFlags);
    const double* dens_b = dens + (a.j_row0 + kq) * DL + sub * kQuadTile + 2 * c;
    const double* dens_e = dens + a.i_row0 * DL + sub * kQuadTile + 2 * c;
    const FusedPart walk = {a.part_rb0[part], a.part_cb0[part], a.part_count[part], 1, a.n_cb,
                            (unsigned)a.unit_base};
    double F[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    const unsigned off_a = lane * 16 + p * 1024;
    if (2 * p + 1 < n_u)
      fused_quad_pass<2, DL>(rs_t, off_a, up * 1024u, dens_b, dens_e, walk, F);
    else
      fused_quad_pass<1, DL>(rs_t, off_a, up * 1024u, dens_b, dens_e, walk, F);
    // r = 4 (2 p + u) + l / 16, draws 2 c and 2 c + 1 of the tile
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = 4 * (2 * p + u) + kq;
      if (r < a.n_rows[t]) {
        const f64x2 value = {F[u][0], F[u][1]};
        *(f64x2*)(sums + ((size_t)part * n_total + a.r_offset[t] + r) * kLanes + sub * kQuadTile +
                  2 * c) = value;
      }
    }
  }
  {
    // mode cross: row g of the cross tables' rows, numbered through the list
    int n_cross = 0;
    for (int t = 0; t < a.n_tables; ++t)
      if (a.mode[t] == TC_MODE_CROSS) n_cross += a.n_rows[t];
    for (int g = (wave + W - n_jobs % W) % W; g < n_cross; g += W) {
      int t = 0, r = g;
      for (;; ++t) {
        if (a.mode[t] != TC_MODE_CROSS) continue;
        if (r < a.n_rows[t]) break;
        r -= a.n_rows[t];
      }
      sc_f64 matrix = (sc_f64)a.matrix[t];
      const int n_r = a.n_rows[t];
      double sum = 0.0;
      for (int i = 0; i < a.n_bins; ++i) sum = fma(matrix[i * n_r + r], dens[i * DL + lane], sum);
      sums[(size_t)(a.r_offset[t] + r) * kLanes + lane] = sum;
    }
  }
  __syncthreads();       // the densities are dead: their place takes the results tile

  // ---- 3. the parts of every row, normalisation, results ----
  double(*tile)[kLanes + 1] = (double(*)[kLanes + 1])dens;
  const double ngal2 = ngal * ngal;
  for (int t = 0; t < a.n_tables; ++t) {
    const bool is_auto = a.mode[t] == TC_MODE_AUTO;
    for (int rr = wave; rr < a.n_rows[t]; rr += W) {
      const int row = a.r_offset[t] + rr;
      const double* first = sums + (size_t)row * kLanes + lane;
      double sum = first[0];
      if (is_auto) {
#pragma unroll
        for (int part = 1; part < PARTS; ++part) sum += first[(size_t)part * n_total * kLanes];
      }
      tile[row][lane] = sum / (is_auto ? ngal2 : ngal);
    }
  }
  __syncthreads();
  joint_forward_results(tile, table, red[0], n_total, col, a.n_draws, a.xi, a.chi2);
}

}  // namespace tc
