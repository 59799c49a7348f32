// Device code that the occupation-seam kernels share (vjp_kernels.hip.h: one table;
// joint_vjp_kernels.hip.h: the tables of a joint): the pass over a wave's row tiles of the
// mode-auto tables, the likelihood's cotangent, the sums that close a draw and the chain rule of
// vjp.h.  Sharing them is what makes a joint of one table return the table's own bits.
#pragma once

#include <hip/hip_runtime.h>

#include "grad_device.hip.h"
#include "vjp.h"

namespace tc {

namespace vjp {

// The tables of a pass as the pieces below walk them: count() tables in list order, table k of
// mode auto or not, with n_r(k) result rows from row row0(k) on and its matrix(k).  A table
// kernel has the one table of its arguments; joint_vjp_kernels.hip.h has several.
struct OneTable {
  const VjpArgs& a;
  bool mode_auto;
  __device__ __forceinline__ int count() const { return 1; }
  __device__ __forceinline__ bool is_auto(int) const { return mode_auto; }
  __device__ __forceinline__ int n_r(int) const { return a.n_r; }
  __device__ __forceinline__ int row0(int) const { return 0; }
  __device__ __forceinline__ const double* matrix(int) const { return a.matrix; }
};

// One pass of mode auto over the row tiles of this wave: inside a tile the mode-auto tables in
// list order, r ascending inside a table; their rows are numbered consecutively for qpart.
// with_q: qpart[(row 4 + wave), col] += the tiles' share of w . U_r (qpart starts at zero);
// with_g: gsum[i, col] = sum_tables sum_r g_r U_ri for the rows i of the tiles, g_r at row
// row0(k) + r of gbar.  lane = (row group l / 16, draw l % 16); D[row = l / 16 + 4 v][draw] in
// register v.
template <typename Tables>
__device__ __forceinline__ void auto_pass(const VjpArgs& a, const Tables& tables, const double* w,
                                          const double* gbar, double* gsum, double* qpart,
                                          int zero_row, bool with_q, bool with_g) {
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const int group = lane / kGradDraws, col = lane % kGradDraws;
  const int n_bins = a.n_bins;
  const int tiles = a.row_tiles, steps = a.k_steps;
  using grad::f64x4;
  for (int tile = wave; tile < tiles; tile += kGradWaves) {
    double w_row[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = 16 * tile + group + 4 * v;
      w_row[v] = w[(i < n_bins ? i : zero_row) * kGradDraws + col];
    }
    f64x4 g = {0.0, 0.0, 0.0, 0.0};
    int q_row0 = 0;
    for (int k = 0; k < tables.count(); ++k) {
      if (!tables.is_auto(k)) continue;
      const int n_r = tables.n_r(k), g_row0 = tables.row0(k);
      const double* matrix = tables.matrix(k);
      for (int r = 0; r < n_r; ++r) {
        const double* a_lane = matrix + ((size_t)r * tiles + tile) * steps * 64 + lane;
        const f64x4 u = grad::dense_tile_product(a_lane, steps, w, group, col, [=](int j) {
          return j < n_bins ? j : zero_row;
        });
        if (with_q) {
          double q = 0.0;
#pragma unroll
          for (int v = 0; v < 4; ++v) q = fma(w_row[v], u[v], q);
          q = grad::sum_row_groups(q);
          if (group == 0) qpart[((q_row0 + r) * kGradWaves + wave) * kGradDraws + col] += q;
        }
        if (with_g) {
          const double g_r = gbar[(g_row0 + r) * kGradDraws + col];
#pragma unroll
          for (int v = 0; v < 4; ++v) g[v] = fma(g_r, u[v], g[v]);
        }
      }
      q_row0 += n_r;
    }
    if (with_g) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 16 * tile + group + 4 * v;
        if (i < n_bins) gsum[i * kGradDraws + col] = g[v];
      }
    }
  }
}

// Likelihood form, items (r, draw): gbar_r = sum_s (P_rs + P_sr) e_s = (2 P_sym e)_r and pe_r =
// (P e)_r with e = xi - data, in s order.
__device__ __forceinline__ void chi2_cotangent(const VjpArgs& a, const double* xis, double* gbar,
                                               double* pe) {
  const int n_r = a.n_r;
  const double* data = a.chi2_data;
  const double* precision = a.chi2_data + n_r;
  for (int item = threadIdx.x; item < n_r * kGradDraws; item += kGradThreads) {
    const int r = item / kGradDraws, col = item % kGradDraws;
    double both = 0.0, row = 0.0;
    for (int s = 0; s < n_r; ++s) {
      const double e = xis[s * kGradDraws + col] - data[s];
      const double p_rs = precision[(size_t)r * n_r + s];
      both = fma(p_rs + precision[(size_t)s * n_r + r], e, both);
      row = fma(p_rs, e, row);
    }
    gbar[item] = both;
    pe[item] = row;
  }
}

// Threads 0 .. 15 = draw: c = sum_r g_r xi_r, one chain over the rows of the mode-auto tables
// into dot_auto and one over the rows of the others into dot_cross (either may be NULL), in row
// order; and, likelihood form (chi2_data), chi2 = e . (P e) over all a.n_r rows.
template <typename Tables>
__device__ __forceinline__ void finish_draws(const VjpArgs& a, const Tables& tables,
                                             const double* xis, const double* gbar,
                                             const double* pe, double* dot_auto,
                                             double* dot_cross, int64_t draw0) {
  const int t = threadIdx.x;
  if (t >= kGradDraws) return;
  double c_auto = 0.0, c_cross = 0.0, chi2 = 0.0;
  for (int k = 0; k < tables.count(); ++k) {
    const int begin = tables.row0(k), end = begin + tables.n_r(k);
    if (tables.is_auto(k)) {
      for (int r = begin; r < end; ++r)
        c_auto = fma(gbar[r * kGradDraws + t], xis[r * kGradDraws + t], c_auto);
    } else {
      for (int r = begin; r < end; ++r)
        c_cross = fma(gbar[r * kGradDraws + t], xis[r * kGradDraws + t], c_cross);
    }
  }
  if (dot_auto != nullptr) dot_auto[t] = c_auto;
  if (dot_cross != nullptr) dot_cross[t] = c_cross;
  if (a.chi2_data == nullptr) return;
  const int n_r = a.n_r;
  for (int r = 0; r < n_r; ++r)
    chi2 = fma(xis[r * kGradDraws + t] - a.chi2_data[r], pe[r * kGradDraws + t], chi2);
  if (draw0 + t < a.n_draws) a.chi2[draw0 + t] = chi2;
}

// The chain rule of vjp.h for one (bin, draw): auto_sum = sum_r g_r U_ri and auto_dot = sum_r g_r
// xi_r over the rows of the mode-auto tables, cross_sum = sum_r g_r T_ri and cross_dot likewise
// over the others.  An absent term is an exact zero: adding it leaves the sum as it is.
__device__ __forceinline__ double chain_rule(double n_h, double g_ngal, double inv_ngal,
                                             double inv_ngal2, double auto_sum, double auto_dot,
                                             double cross_sum, double cross_dot) {
  return n_h * (g_ngal + 2.0 * inv_ngal2 * auto_sum + cross_sum * inv_ngal -
                2.0 * inv_ngal * auto_dot - cross_dot * inv_ngal);
}

}  // namespace vjp

}  // namespace tc
