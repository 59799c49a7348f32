// Gradient kernels of an interpolator: (ngal, xi[, chi2]) of a batch of draws (theta, x) over a
// grid of tables together with their exact derivatives with respect to the five Zheng07
// parameters AND the n_dim extra parameters, one launch per batch (grad.h: GradInterpArgs and the
// LDS budget; interp.cpp fills the arguments).
//
// The interpolated result is linear in the per-table results: with c_t(x) the tensor-product
// spline weight of table t,
//   ngal = sum_t c_t ngal_t, xi_r = sum_t c_t xi_{t,r},
//   d/dtheta_k = sum_t c_t d(ngal_t, xi_t)/dtheta_k,  d/dx_d = sum_t (dc_t/dx_d) (ngal_t, xi_t).
// A workgroup of four waves carries kGradDraws = 16 draws:
//   1  the weights and derivative weights of every axis (grad.h: spline_weights, the text the
//      host helper tc_spline_weights runs) into LDS;
//   2  the tables class by class, inside a class in list order: the node loops of
//      grad_kernels.hip.h once per CLASS, the matrix products once per TABLE, every table's
//      results added with c_t (value, five theta derivatives) and dc_t/dx_d (n_dim more) into
//      6 + n_dim accumulators per (r, draw) in LDS;
//   3  the stores or, with a data vector, chi2, its 5 + n_dim derivatives and, where asked for,
//      the Fisher matrix over the same 5 + n_dim quantities.
// The order of every sum -- tables, rows, slabs -- is fixed by the interpolator: a draw's results
// do not depend on the batch or on the draw's neighbours.
// NP as in grad_kernels.hip.h: 5, or 7 for the decorated model, where "6" reads 8 and "5" 7, or
// 11 for the Leauthaud11 family (theta then has 14 columns), where they read 12 and 11.
#pragma once

#include "grad_kernels.hip.h"

namespace tc {

namespace grad {

// Weights (n_dim, kGradMaxAxis, 16) and, behind them, derivative weights of the workgroup's
// draws: thread = (node j % 16, draw).
__device__ __forceinline__ void interp_weights(const GradInterpArgs& ia, int64_t draw0,
                                               double* weights) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw = clamp_draw(draw0 + col, ia.table.n_draws);
  double* dweights = weights + (size_t)ia.n_dim * kGradMaxAxis * kGradDraws;
  for (int d = 0; d < ia.n_dim; ++d)
    spline_weights(ia.n_axis[d], ia.xp + ia.axis_offset[d], ia.a + ia.a_offset[d],
                   ia.x[draw * ia.n_dim + d], t / kGradDraws, kGradThreads / kGradDraws,
                   kGradDraws, weights + (size_t)d * kGradMaxAxis * kGradDraws + col,
                   dweights + (size_t)d * kGradMaxAxis * kGradDraws + col);
}

// Coefficient of the table at grid node `node` for one draw: which = 0 its weight c_t, which =
// 1 + d the derivative dc_t/dx_d (the derivative of the one factor of axis d times the others).
__device__ __forceinline__ double interp_coef(const GradInterpArgs& ia, const double* weights,
                                              const int32_t* node, int which, int col) {
  const double* dweights = weights + (size_t)ia.n_dim * kGradMaxAxis * kGradDraws;
  double c = 1.0;
  for (int e = 0; e < ia.n_dim; ++e) {
    const double* from = e == which - 1 ? dweights : weights;
    c *= from[((size_t)e * kGradMaxAxis + node[e]) * kGradDraws + col];
  }
  return c;
}

// Accumulator q = 0 .. 5 takes c_t times quantity q of the table, q = 6 + d takes dc_t/dx_d times
// its value (quantity 0).
template <int NP>
__device__ __forceinline__ int interp_which(int q) { return q < NP + 1 ? 0 : q - NP; }
template <int NP>
__device__ __forceinline__ int interp_quantity(int q) { return q < NP + 1 ? q : 0; }

__device__ __forceinline__ void set_class(GradArgs& a, const GradInterpArgs& ia, int v) {
  a.log_m = ia.class_log_m[v];
  a.m = ia.class_m[v];
  a.weight = ia.class_weight[v];
  a.n_h = ia.class_n_h[v];
  a.percentile = ia.class_percentile != nullptr ? ia.class_percentile[v] : nullptr;
}

// ngal and its 5 + n_dim derivatives (thread = (q, draw)), then xi and its derivatives from the
// accumulators (n_q, n_r, 16) -- or chi2, its derivatives and, where asked for, the Fisher matrix.
__device__ __forceinline__ void interp_finish(const GradArgs& a, int n_q, double my_ngal,
                                              double* sums, int64_t draw0) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int n_r = a.n_r;
  const int64_t draw = draw0 + col;
  if (t < n_q * kGradDraws && draw < a.n_draws) {
    const int q = t / kGradDraws;
    if (q == 0)
      a.ngal[draw] = my_ngal;
    else
      a.dngal[draw * (n_q - 1) + (q - 1)] = my_ngal;
  }
  if (a.xi != nullptr) {
    if (draw >= a.n_draws) return;
    for (int item = t; item < n_q * n_r * kGradDraws; item += kGradThreads) {
      const int q = item / (n_r * kGradDraws), r = item / kGradDraws % n_r;
      if (q == 0)
        a.xi[draw * n_r + r] = sums[item];
      else
        a.dxi[(draw * (n_q - 1) + (q - 1)) * n_r + r] = sums[item];
    }
    return;
  }
  for (int item = t; item < n_r * kGradDraws; item += kGradThreads)
    sums[item] -= a.chi2_data[item / kGradDraws];
  __syncthreads();
  finish_chi2(a, sums, draw0, n_q);
  finish_fisher(a, sums, draw0, n_q);
}

}  // namespace grad

// ---- mode auto ----------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(kGradThreads) void grad_interp_auto_kernel(const GradInterpArgs ia) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  GradArgs a = ia.table;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central, n_r = a.n_r, n_dim = ia.n_dim;
  const int n_q = NQ + n_dim;
  const int zero_row = grad_auto_rows(n_bins, n_central, NP) - 1;
  double* w = grad_lds;                                               // (rows, 16), one class
  double* total = w + (size_t)(zero_row + 1) * kGradDraws;            // (6, 16), one class
  double* weights = total + NQ * kGradDraws;                           // (2, n_dim, 32, 16)
  double* sums = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;   // (n_q, n_r, 16)
  const fm::Consts k = fm::make_consts();
  grad::interp_weights(ia, draw0, weights);
  for (int item = t; item < n_q * n_r * kGradDraws; item += kGradThreads) sums[item] = 0.0;
  double my_ngal = 0.0;                                               // thread = (q, draw)
  const int wave = t / 64, group = t % 64 / kGradDraws;
  for (int v = 0; v < ia.n_classes; ++v) {
    grad::set_class(a, ia, v);
    __syncthreads();
    {
      const typename grad::DrawOf<NP>::type d = grad::load_draw<NP>(a, k, draw0 + col);
      grad::auto_node_loops<NP>(a, k, d, w, zero_row);
    }
    __syncthreads();
    if (t < NQ * kGradDraws)
      total[t] = grad::auto_total<NP>(w, t / kGradDraws, col, n_bins, n_central, zero_row);
    __syncthreads();
    const double ngal = total[col];
    const double inv_ngal = 1.0 / ngal;
    const double inv_ngal2 = 1.0 / (ngal * ngal);
    for (int s = ia.class_begin[v]; s < ia.class_begin[v + 1]; ++s) {
      const int32_t* node = ia.walk_node + (size_t)s * n_dim;
      if (t < n_q * kGradDraws) {
        const int q = t / kGradDraws;
        my_ngal = fma(grad::interp_coef(ia, weights, node, grad::interp_which<NP>(q), col),
                      total[grad::interp_quantity<NP>(q) * kGradDraws + col], my_ngal);
      }
      a.matrix = ia.matrices[s];
      const double c = grad::interp_coef(ia, weights, node, 0, col);
      for (int r = wave; r < n_r; r += kGradWaves) {
        double acc[NQ];
        grad::auto_products<NP>(a, w, r, zero_row, acc);
        const double xi = grad::auto_xi(acc, inv_ngal2);
        if (group == 0) {
          double* slot = sums + (size_t)r * kGradDraws + col;
          const size_t stride = (size_t)n_r * kGradDraws;
          slot[0] = fma(c, xi, slot[0]);
#pragma unroll
          for (int p = 1; p < NQ; ++p)
            slot[p * stride] = fma(c, grad::auto_dxi(acc, p, xi, total, col, inv_ngal, inv_ngal2),
                                   slot[p * stride]);
          for (int d = 0; d < n_dim; ++d)
            slot[(NQ + d) * stride] = fma(grad::interp_coef(ia, weights, node, 1 + d, col), xi,
                                         slot[(NQ + d) * stride]);
        }
      }
    }
  }
  __syncthreads();
  grad::interp_finish(a, n_q, my_ngal, sums, draw0);
}

// ---- mode cross ---------------------------------------------------------------------------------
// Inside a class xi_t = T_t . w / ngal shares w and ngal, so the class is linear in the slab
// products: Y_q = sum_t coef_{t,q} T_t . (w or dw_q) accumulates over slabs and tables, the chain
// rule of grad_cross_kernel is applied once per class and the class added to the accumulators.
// The slab holds grad_interp_cross_slab(NP) bins (grad.h).
template <int NP>
__global__ __launch_bounds__(kGradThreads) void grad_interp_cross_kernel(const GradInterpArgs ia) {
  constexpr int NQ = NP + 1;
  constexpr int kSlab = grad_interp_cross_slab(NP);
  extern __shared__ double grad_lds[];
  GradArgs a = ia.table;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_r = a.n_r, n_dim = ia.n_dim;
  const int n_q = NQ + n_dim;
  const int n_items = n_q * n_r * kGradDraws;
  double* w = grad_lds;                                               // (6, slab, 16)
  double* total = w + NQ * kSlab * kGradDraws;                         // (6, 16), one class
  double* weights = total + NQ * kGradDraws;                           // (2, n_dim, 32, 16)
  double* y = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;      // (n_q, n_r, 16), one class
  double* sums = y + n_items;                                         // (n_q, n_r, 16)
  const fm::Consts k = fm::make_consts();
  const typename grad::DrawOf<NP>::type d = grad::load_draw<NP>(a, k, draw0 + col);
  grad::interp_weights(ia, draw0, weights);
  for (int item = t; item < n_items; item += kGradThreads) sums[item] = 0.0;
  double my_ngal = 0.0;                                               // thread = (q, draw)
  for (int v = 0; v < ia.n_classes; ++v) {
    grad::set_class(a, ia, v);
    const int s_begin = ia.class_begin[v], s_end = ia.class_begin[v + 1];
    __syncthreads();
    for (int item = t; item < n_items; item += kGradThreads) y[item] = 0.0;
    double my_total = 0.0;
    for (int slab0 = 0; slab0 < n_bins; slab0 += kSlab) {
      const int count = min(kSlab, n_bins - slab0);
      __syncthreads();
      grad::cross_node_loops<NP, kSlab>(a, k, d, slab0, count, w);
      __syncthreads();
      if (t < NQ * kGradDraws) {
        const int p = t / kGradDraws;
        for (int li = 0; li < count; ++li) my_total += w[(p * kSlab + li) * kGradDraws + col];
      }
      for (int s = s_begin; s < s_end; ++s) {
        const int32_t* node = ia.walk_node + (size_t)s * n_dim;
        const double* matrix = ia.matrices[s];
        // item = (r, quantity p, draw) as in grad_cross_kernel: one product each; the value's
        // product (p = 0) also feeds the n_dim accumulators of d/dx
        for (int item = t; item < NQ * n_r * kGradDraws; item += kGradThreads) {
          const int r = item / (NQ * kGradDraws), p = item / kGradDraws % NQ;
          const double product =
              grad::cross_slab_product<kSlab>(matrix, n_r, r, slab0, count, w, p, col, 0.0);
          const size_t stride = (size_t)n_r * kGradDraws;
          double* slot = y + (size_t)r * kGradDraws + col;
          slot[p * stride] = fma(grad::interp_coef(ia, weights, node, 0, col), product,
                                 slot[p * stride]);
          if (p == 0)
            for (int e = 0; e < n_dim; ++e)
              slot[(NQ + e) * stride] = fma(grad::interp_coef(ia, weights, node, 1 + e, col),
                                           product, slot[(NQ + e) * stride]);
        }
      }
    }
    if (t < NQ * kGradDraws) total[t] = my_total;
    __syncthreads();
    if (t < n_q * kGradDraws) {
      const int q = t / kGradDraws;
      for (int s = s_begin; s < s_end; ++s)
        my_ngal = fma(grad::interp_coef(ia, weights, ia.walk_node + (size_t)s * n_dim,
                                        grad::interp_which<NP>(q), col),
                      total[grad::interp_quantity<NP>(q) * kGradDraws + col], my_ngal);
    }
    // xi = Y_0 / ngal, dxi_k = (Y_k - xi dngal_k) / ngal, d/dx_d = Y_(6 + d) / ngal
    const double inv_ngal = 1.0 / total[col];
    for (int item = t; item < n_items; item += kGradThreads) {
      const int r = item / (n_q * kGradDraws), q = item / kGradDraws % n_q;
      const size_t slot = ((size_t)q * n_r + r) * kGradDraws + col;
      const double xi = y[(size_t)r * kGradDraws + col] * inv_ngal;
      double value = xi;
      if (q >= NQ)
        value = y[slot] * inv_ngal;
      else if (q > 0)
        value = (y[slot] - xi * total[q * kGradDraws + col]) * inv_ngal;
      sums[slot] += value;
    }
  }
  __syncthreads();
  grad::interp_finish(a, n_q, my_ngal, sums, draw0);
}

}  // namespace tc
