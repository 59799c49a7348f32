// Occupation seam of a joint: predict(occupation) of SEVERAL tables that share one halo table,
// its vector-Jacobian product with respect to the occupation array, and chi2 of the concatenated
// data vector with or without its gradient, one launch per batch (joint.h: the argument block
// and the LDS budget; joint.cpp fills it in).  Geometry and pieces are those of
// vjp_kernels.hip.h: kGradDraws = 16 draws per workgroup of kGradWaves = 4 waves, one per LDS
// column; table t owns the rows r_offset[t] .. of the N concatenated ones.
//   1  once per workgroup: w = n . n_h of every bin (through perm, LDS in library order) and one
//      row of zeros; ngal = sum_i w_i in bin order;
//   2  mode-auto tables: wave v owns the row tiles v, v + 4, ...; inside a tile the auto tables
//      in list order, r ascending inside a table (vjp::auto_pass) -- the tile's four rows of
//      sum_t sum_r g_r (S_tr w)_i stay in registers across the tables, the tile's share of q_tr =
//      w . S_tr w goes to the wave's partial; the four partials are added in wave order;
//   3  mode-cross tables: one fma chain per (row, draw) over the bins in library order, read from
//      the LDS rows of w (no slabs: a joint keeps every bin in LDS);
//   4  xi_r = q_r / ngal^2 (auto) or y_r / ngal (cross), stored where asked for;
//   5  likelihood form: g = 2 P_sym (xi - data) and P e over all N rows (vjp::chi2_cotangent: the
//      off-diagonal blocks of the precision matrix couple the tables), chi2 = e . (P e), and the
//      auto pass a SECOND time with its cotangent (U_r for all r does not fit the LDS);
//   6  the chain rule of joint.h per (bin, draw), stored in reference row order; the cross sum
//      is read from the tables' (n_bins, n_r) matrices in global memory.
// Forward only (g_occupation == NULL): no cotangent pass and no phase 6 -- (ngal, xi), or
// (ngal, chi2) with ONE product per auto table.
// Order guarantees:
//   - ONE form: a draw's results depend on its own LDS column alone -- not on the batch, its place
//     in it or the entry point; a draw without galaxies keeps its NaN to itself;
//   - a row's arithmetic does not depend on the wave or thread that runs it;
//   - the pieces are those of the table kernels, and an absent term of the chain rule is an exact
//     zero that is added: a joint of ONE table returns the values of vjp_auto_kernel /
//     vjp_cross_kernel on that table bit for bit (the slabs of vjp_cross_kernel amount to the one
//     fma chain in bin order), and the forward-only form those of the gradient form.
#pragma once

#include "joint.h"
#include "vjp_device.hip.h"

namespace tc {

namespace vjp {

// The tables of a joint as auto_pass and finish_draws walk them.
struct JointTables {
  const JointVjpArgs& j;
  __device__ __forceinline__ int count() const { return j.n_tables; }
  __device__ __forceinline__ bool is_auto(int k) const { return j.mode[k] == TC_MODE_AUTO; }
  __device__ __forceinline__ int n_r(int k) const { return j.n_r[k]; }
  __device__ __forceinline__ int row0(int k) const { return j.r_offset[k]; }
  __device__ __forceinline__ const double* matrix(int k) const { return j.matrix[k]; }
};

// T_r . w of one draw: one fma chain over the bins in library order.
__device__ __forceinline__ double cross_row_product(const double* matrix, int n_r, int r,
                                                    const double* w, int col, int n_bins) {
  double sum = 0.0;
  for (int i = 0; i < n_bins; ++i)
    sum = fma(matrix[(size_t)i * n_r + r], w[i * kGradDraws + col], sum);
  return sum;
}

}  // namespace vjp

__global__ __launch_bounds__(kGradThreads) void vjp_joint_kernel(const JointVjpArgs j) {
  extern __shared__ __attribute__((aligned(16))) double vjp_joint_lds[];
  const VjpArgs& a = j.vjp;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int64_t draw = draw0 + col;
  const int64_t source = grad::clamp_draw(draw, a.n_draws);
  const int n_bins = a.n_bins, n_all = a.n_r, n_auto = j.n_r_auto;
  const bool likelihood = a.chi2_data != nullptr;
  const bool backward = a.g_occupation != nullptr;
  const int zero_row = n_bins;
  const int part_rows = kGradWaves * n_auto > n_all ? kGradWaves * n_auto : n_all;
  double* w = vjp_joint_lds;                                        // (n_bins + 1, 16)
  double* gsum = w + (size_t)(n_bins + 1) * kGradDraws;             // (n_bins, 16)
  double* part = gsum + (size_t)n_bins * kGradDraws;                // (n_auto, 4, 16); (N, 16)
  double* gbar = part + (size_t)part_rows * kGradDraws;             // (N, 16)
  double* xis = gbar + (size_t)n_all * kGradDraws;                  // (N, 16)
  double* total = xis + (size_t)n_all * kGradDraws;                 // ngal, the two sums g_r xi_r
  const vjp::JointTables tables{j};

  // phase 1: thread = (bin i % 16, draw)
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
    const int i = item / kGradDraws;
    w[item] = a.occupation[source * n_bins + a.perm[i]] * a.n_h[i];
  }
  if (t < kGradDraws) w[zero_row * kGradDraws + t] = 0.0;
  for (int item = t; item < kGradWaves * n_auto * kGradDraws; item += kGradThreads)
    part[item] = 0.0;
  if (backward && !likelihood)
    for (int item = t; item < n_all * kGradDraws; item += kGradThreads)
      gbar[item] = a.g_xi[source * n_all + item / kGradDraws];
  __syncthreads();
  if (t < kGradDraws) {
    double sum = 0.0;
    for (int i = 0; i < n_bins; ++i) sum += w[i * kGradDraws + t];
    total[t] = sum;
    if (draw < a.n_draws) a.ngal[draw] = sum;
  }

  // phase 2: the auto products (the likelihood form: for q_r alone)
  vjp::auto_pass(a, tables, w, gbar, gsum, part, zero_row, true, backward && !likelihood);
  __syncthreads();
  const double ngal = total[col];
  const double inv_ngal = 1.0 / ngal;
  const double inv_ngal2 = 1.0 / (ngal * ngal);
  // phases 3 and 4: items (row, draw) of every table  (item % 16 == col: 256 is a multiple of 16)
  int q_row0 = 0;
  for (int k = 0; k < j.n_tables; ++k) {
    const int n_r = j.n_r[k], row0 = j.r_offset[k];
    const bool is_auto = j.mode[k] == TC_MODE_AUTO;
    const double* matrix = j.matrix[k];
    for (int item = t; item < n_r * kGradDraws; item += kGradThreads) {
      const int r = item / kGradDraws;
      double xi;
      if (is_auto) {
        const double* mine = part + (size_t)(q_row0 + r) * kGradWaves * kGradDraws + col;
        double q = mine[0];
#pragma unroll
        for (int v = 1; v < kGradWaves; ++v) q += mine[v * kGradDraws];
        xi = q * inv_ngal2;
      } else {
        xi = vjp::cross_row_product(matrix, n_r, r, w, col, n_bins) * inv_ngal;
      }
      xis[(row0 + r) * kGradDraws + col] = xi;
      if (a.xi != nullptr && draw < a.n_draws) a.xi[draw * n_all + row0 + r] = xi;
    }
    if (is_auto) q_row0 += n_r;
  }
  if (!likelihood && !backward) return;
  __syncthreads();

  // phase 5
  if (likelihood) {
    vjp::chi2_cotangent(a, xis, gbar, part);
    __syncthreads();
    // the auto products once more, now with their cotangent
    if (backward) vjp::auto_pass(a, tables, w, gbar, gsum, part, zero_row, false, true);
  }
  vjp::finish_draws(a, tables, xis, gbar, part, total + kGradDraws, total + 2 * kGradDraws, draw0);
  if (!backward) return;
  __syncthreads();

  // phase 6
  const double g_ngal = likelihood || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source];
  const double auto_dot = total[kGradDraws + col];
  const double cross_dot = total[2 * kGradDraws + col];
  if (draw >= a.n_draws) return;
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
    const int i = item / kGradDraws;
    double cross_sum = 0.0;
    for (int k = 0; k < j.n_tables; ++k) {
      if (j.mode[k] == TC_MODE_AUTO) continue;
      const int n_r = j.n_r[k];
      const double* row = j.matrix[k] + (size_t)i * n_r;
      const double* g = gbar + (size_t)j.r_offset[k] * kGradDraws + col;
      for (int r = 0; r < n_r; ++r) cross_sum = fma(g[r * kGradDraws], row[r], cross_sum);
    }
    const double auto_sum = n_auto > 0 ? gsum[item] : 0.0;
    a.g_occupation[draw * n_bins + a.perm[i]] = vjp::chain_rule(
        a.n_h[i], g_ngal, inv_ngal, inv_ngal2, auto_sum, auto_dot, cross_sum, cross_dot);
  }
}

}  // namespace tc
