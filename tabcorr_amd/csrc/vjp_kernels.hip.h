// Vector-Jacobian product of predict(occupation) with respect to the occupation array, one launch
// per batch (vjp.h: the formulas, the argument block and the LDS budget; launch.hip: run_vjp;
// vjp_device.hip.h: the pieces these kernels share with the joint's, joint_vjp_kernels.hip.h).
//
// A workgroup of four waves carries kGradDraws = 16 draws, one per LDS column:
//   1  w = n . n_h of every bin from the caller's array (reference row order, through perm) into
//      LDS in library order; ngal = sum_i w_i in bin order;
//   2  mode auto: U_r = S_r W on the FP64 matrix pipe (v_mfma_f64_16x16x4_f64 against the dense
//      operand of grad.h, as grad::auto_products).  Wave v owns the row tiles v, v + 4, ... and
//      loops over r inside a tile: the tile's four rows of sum_r g_r U_ri stay in registers, the
//      tile's share of q_r = w . U_r is added to the wave's partial q_r in LDS; the four partials
//      are added in wave order.  Mode cross: vector FMAs; pass 1 over the bins in slabs gives
//      T_r . w, pass 2 sum_r g_r T_ri bin by bin (it needs no w);
//   3  the chain rule of vjp.h and the stores, in reference row order.
// Likelihood form (g_xi == NULL): the cotangent 2 P_sym (xi - data) needs xi first, so mode auto
// runs the product TWICE in the launch -- once for q_r alone, once for sum_r g_r U_ri (U_r for all
// r does not fit the LDS) -- and mode cross simply forms it between its two passes.  Nothing
// leaves the device in between.
// There is ONE form per mode: the sums over bins in bin order, the matrix products in column
// order, the rows of a tile by the fixed tree over its four row groups, the tiles of a wave in
// tile order, the waves in wave order -- a draw's results depend on its own LDS column alone,
// never on the batch or on its neighbours (a draw without galaxies keeps its NaN to itself).
// Where ngal = 0 the results are what IEEE arithmetic gives.
#pragma once

#include <hip/hip_runtime.h>

#include "vjp_device.hip.h"

namespace tc {

// ---- mode auto ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void vjp_auto_kernel(const VjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double vjp_lds[];
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int64_t draw = draw0 + col;
  const int64_t source = grad::clamp_draw(draw, a.n_draws);
  const int n_bins = a.n_bins, n_r = a.n_r;
  const bool likelihood = a.g_xi == nullptr;
  const int zero_row = n_bins;
  double* w = vjp_lds;                                              // (n_bins + 1, 16)
  double* gsum = w + (size_t)(n_bins + 1) * kGradDraws;             // (n_bins, 16)
  double* qpart = gsum + (size_t)n_bins * kGradDraws;               // (n_r, 4, 16)
  double* gbar = qpart + (size_t)kGradWaves * n_r * kGradDraws;     // (n_r, 16)
  double* xis = gbar + (size_t)n_r * kGradDraws;                    // (n_r, 16)
  double* total = xis + (size_t)n_r * kGradDraws;                   // ngal (16), sum_r g_r xi_r (16)

  // phase 1: thread = (bin i % 16, draw)
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
    const int i = item / kGradDraws;
    w[item] = a.occupation[source * n_bins + a.perm[i]] * a.n_h[i];
  }
  if (t < kGradDraws) w[zero_row * kGradDraws + t] = 0.0;
  for (int item = t; item < kGradWaves * n_r * kGradDraws; item += kGradThreads) qpart[item] = 0.0;
  if (!likelihood)
    for (int item = t; item < n_r * kGradDraws; item += kGradThreads)
      gbar[item] = a.g_xi[source * n_r + item / kGradDraws];
  __syncthreads();
  if (t < kGradDraws) {
    double sum = 0.0;
    for (int i = 0; i < n_bins; ++i) sum += w[i * kGradDraws + t];
    total[t] = sum;
    if (draw < a.n_draws) a.ngal[draw] = sum;
  }

  // phase 2: the product (the likelihood form: for q_r alone)
  const vjp::OneTable table{a, true};
  vjp::auto_pass(a, table, w, gbar, gsum, qpart, zero_row, true, !likelihood);
  __syncthreads();
  const double ngal = total[col];
  const double inv_ngal = 1.0 / ngal;
  const double inv_ngal2 = 1.0 / (ngal * ngal);
  for (int item = t; item < n_r * kGradDraws; item += kGradThreads) {
    const int r = item / kGradDraws;           // (item % 16 == col: 256 is a multiple of 16)
    const double* part = qpart + (size_t)r * kGradWaves * kGradDraws + col;
    double q = part[0];
#pragma unroll
    for (int v = 1; v < kGradWaves; ++v) q += part[v * kGradDraws];
    const double xi = q * inv_ngal2;
    xis[item] = xi;
    if (!likelihood && draw < a.n_draws) a.xi[draw * n_r + r] = xi;
  }
  __syncthreads();
  if (likelihood) {
    vjp::chi2_cotangent(a, xis, gbar, qpart);
    __syncthreads();
    // the product once more, now with its cotangent
    vjp::auto_pass(a, table, w, gbar, gsum, qpart, zero_row, false, true);
  }
  vjp::finish_draws(a, table, xis, gbar, qpart, total + kGradDraws, nullptr, draw0);
  __syncthreads();

  // phase 3
  const double g_ngal = likelihood || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source];
  const double c = total[kGradDraws + col];
  if (draw >= a.n_draws) return;
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
    const int i = item / kGradDraws;
    a.g_occupation[draw * n_bins + a.perm[i]] =
        vjp::chain_rule(a.n_h[i], g_ngal, inv_ngal, inv_ngal2, gsum[item], c, 0.0, 0.0);
  }
}

// ---- mode cross ---------------------------------------------------------------------------------
// xi_r = T_r . w / ngal (tabcorr.py:646-649) on the (n_bins, n_r) matrix of grad_cross_kernel:
// the bins in slabs of kGradCrossSlab, any number of them; vector FMAs, thread = (r, draw) items
// in pass 1 and (bin, draw) items in pass 2.
__global__ __launch_bounds__(kGradThreads) void vjp_cross_kernel(const VjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double vjp_lds[];
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int64_t draw = draw0 + col;
  const int64_t source = grad::clamp_draw(draw, a.n_draws);
  const int n_bins = a.n_bins, n_r = a.n_r;
  const bool likelihood = a.g_xi == nullptr;
  double* w = vjp_lds;                                              // (slab, 16)
  double* y = w + (size_t)kGradCrossSlab * kGradDraws;              // (n_r, 16)
  double* gbar = y + (size_t)n_r * kGradDraws;                      // (n_r, 16)
  double* xis = gbar + (size_t)n_r * kGradDraws;                    // (n_r, 16)
  double* total = xis + (size_t)n_r * kGradDraws;                   // ngal (16), sum_r g_r xi_r (16)
  const int n_items = n_r * kGradDraws;
  for (int item = t; item < n_items; item += kGradThreads) {
    y[item] = 0.0;
    if (!likelihood) gbar[item] = a.g_xi[source * n_r + item / kGradDraws];
  }

  // pass 1
  double my_total = 0.0;
  for (int slab0 = 0; slab0 < n_bins; slab0 += kGradCrossSlab) {
    const int count = min(kGradCrossSlab, n_bins - slab0);
    __syncthreads();
    for (int item = t; item < count * kGradDraws; item += kGradThreads) {
      const int i = slab0 + item / kGradDraws;
      w[item] = a.occupation[source * n_bins + a.perm[i]] * a.n_h[i];
    }
    __syncthreads();
    if (t < kGradDraws)
      for (int li = 0; li < count; ++li) my_total += w[li * kGradDraws + t];
    for (int item = t; item < n_items; item += kGradThreads) {
      y[item] = grad::cross_slab_product(a.matrix, n_r, item / kGradDraws, slab0, count, w, 0, col,
                                         y[item]);
    }
  }
  if (t < kGradDraws) {
    total[t] = my_total;
    if (draw < a.n_draws) a.ngal[draw] = my_total;
  }
  __syncthreads();
  const double inv_ngal = 1.0 / total[col];
  for (int item = t; item < n_items; item += kGradThreads) {
    const double xi = y[item] * inv_ngal;       // (item % 16 == col)
    xis[item] = xi;
    if (!likelihood && draw < a.n_draws) a.xi[draw * n_r + item / kGradDraws] = xi;
  }
  __syncthreads();
  if (likelihood) {
    vjp::chi2_cotangent(a, xis, gbar, y);
    __syncthreads();
  }
  const vjp::OneTable table{a, false};
  vjp::finish_draws(a, table, xis, gbar, y, nullptr, total + kGradDraws, draw0);
  __syncthreads();

  // pass 2
  const double g_ngal = likelihood || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source];
  const double c = total[kGradDraws + col];
  if (draw >= a.n_draws) return;
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
    const int i = item / kGradDraws;
    const double* row = a.matrix + (size_t)i * n_r;
    double sum = 0.0;
    for (int r = 0; r < n_r; ++r) sum = fma(gbar[r * kGradDraws + col], row[r], sum);
    a.g_occupation[draw * n_bins + a.perm[i]] =
        vjp::chain_rule(a.n_h[i], g_ngal, inv_ngal, 0.0, 0.0, 0.0, sum, c);
  }
}

}  // namespace tc
