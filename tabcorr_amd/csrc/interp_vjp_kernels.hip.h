// Occupation seam of an interpolator: predict(occupation, x) over a grid of tables, its
// vector-Jacobian product with respect to the occupation array (n_classes, n_bins) AND the grid
// parameters x, and chi2 of the interpolated prediction with or without its gradient, one launch
// per batch (vjp.h: the formulas, InterpVjpArgs and the LDS budget; interp.cpp fills the
// arguments).  Geometry and pieces are those of vjp_kernels.hip.h and grad_interp_kernels.hip.h:
// kGradDraws = 16 draws per workgroup of kGradWaves = 4 waves, one per LDS column.
//   1  the weights and derivative weights of every axis into LDS (grad::interp_weights);
//   2  the walk: the tables class by class, inside a class in list order.  Per class w = n_v .
//      n_h,v and ngal_v = sum_i w_i in bin order.  Mode auto, per table: U_r = S_t,r w on the FP64
//      matrix pipe (vjp::auto_pass on the dense operand of grad.h), the per-wave partials of q_r
//      added in wave order, xi_t,r = q_r / ngal_v^2 added with c_t to the class's share of xi and
//      with dc_t/dx_d to the accumulators of dxi_r/dx_d; with a cotangent the table's sum_r g_r
//      U_ri added with c_t to the class accumulator of g_n, which is stored when the walk leaves
//      the class.  Mode cross: the class is linear in the slab products, Y_q = sum_{t in v}
//      coef_t,q T_t . w over slabs of kGradCrossSlab bins and tables (q = 0: c_t, 1 + d:
//      dc_t/dx_d), divided by ngal_v once per class; with a cotangent a second pass over the
//      bins of the class gives sum_t c_t sum_r g_r T_t,ri;
//   3  g_x[d] = g_ngal dngal/dx_d + sum_r g_r dxi_r/dx_d from the accumulators, and the stores.
// Likelihood form (chi2_data): the cotangent 2 P_sym (xi - data) needs the interpolated xi, so
// the kernel walks the tables TWICE -- a forward walk, then the adjoint walk, which forms the
// tables' products again; nothing leaves the device in between.  The prediction form with its
// cotangents given needs one walk.  Forward only (g_occupation == NULL): the forward walk alone --
// no cotangent work, no row of g_n; its (ngal, xi) or (ngal, chi2) are the bits of the full form.
// The order of every sum -- tables, rows, slabs, waves -- is fixed by the interpolator: a draw's
// results depend on its own LDS column alone, never on the batch or on its place in it.  An x
// outside the grid takes the outermost polynomial (spline.h).
#pragma once

#include <hip/hip_runtime.h>

#include "grad_interp_kernels.hip.h"
#include "vjp_device.hip.h"

namespace tc {

namespace vjp {

// What both kernels do once the forward walk is complete, between two barriers of the caller:
// the stores of the prediction form, or the likelihood's cotangent and chi2 (pe: n_r rows of
// scratch).  Ends behind a barrier.
__device__ __forceinline__ void interp_after_forward(const VjpArgs& a, const double* xis,
                                                     double* gbar, double* pe, double* scratch,
                                                     int64_t draw0) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw = draw0 + col;
  const int n_r = a.n_r;
  if (a.chi2_data == nullptr) {
    if (draw < a.n_draws)
      for (int item = t; item < n_r * kGradDraws; item += kGradThreads)
        a.xi[draw * n_r + item / kGradDraws] = xis[item];
    return;
  }
  chi2_cotangent(a, xis, gbar, pe);
  __syncthreads();
  const OneTable table{a, true};
  finish_draws(a, table, xis, gbar, pe, scratch, nullptr, draw0);
  __syncthreads();
}

// Threads (q, draw), q <= n_dim: q = 0 stores ngal; q = 1 + d stores g_x[d] = g_ngal dngal/dx_d
// + sum_r g_r dxi_r/dx_d (backward) and, likelihood form, dngal/dx_d.
__device__ __forceinline__ void interp_finish_x(const InterpVjpArgs& ia, const VjpArgs& a,
                                                const double* gbar, const double* dxi,
                                                double mine, int64_t draw0, int64_t source) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws, q = t / kGradDraws;
  const int n_r = a.n_r, n_dim = ia.interp.n_dim;
  const int64_t draw = draw0 + col;
  if (q > n_dim || draw >= a.n_draws) return;
  const bool likelihood = a.chi2_data != nullptr;
  if (q == 0) {
    a.ngal[draw] = mine;
    return;
  }
  if (likelihood && ia.dngal_dx != nullptr) ia.dngal_dx[draw * n_dim + (q - 1)] = mine;
  if (a.g_occupation == nullptr) return;
  double sum = likelihood || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source] * mine;
  const double* rows = dxi + (size_t)(q - 1) * n_r * kGradDraws + col;
  for (int r = 0; r < n_r; ++r) sum = fma(gbar[r * kGradDraws + col], rows[r * kGradDraws], sum);
  ia.g_x[draw * n_dim + (q - 1)] = sum;
}

}  // namespace vjp

// ---- mode auto ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void vjp_interp_auto_kernel(const InterpVjpArgs ia) {
  extern __shared__ __attribute__((aligned(16))) double vjp_interp_lds[];
  VjpArgs a = ia.vjp;
  const GradInterpArgs& grid = ia.interp;
  const int t = threadIdx.x;
  const int col = t % kGradDraws, q_mine = t / kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int64_t draw = draw0 + col;
  const int64_t source = grad::clamp_draw(draw, a.n_draws);
  const int n_bins = a.n_bins, n_r = a.n_r, n_dim = grid.n_dim, n_classes = grid.n_classes;
  const bool likelihood = a.chi2_data != nullptr;
  const bool backward = a.g_occupation != nullptr;
  const int zero_row = n_bins;
  const int n_items = n_r * kGradDraws;
  double* weights = vjp_interp_lds;                                  // (2, n_dim, 32, 16)
  double* w = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;   // (n_bins + 1, 16)
  double* gsum = w + (size_t)(n_bins + 1) * kGradDraws;              // (n_bins, 16), one table
  double* gacc = gsum + (size_t)n_bins * kGradDraws;                 // (n_bins, 16), one class
  double* qpart = gacc + (size_t)n_bins * kGradDraws;                // (n_r, 4, 16)
  double* xv = qpart + (size_t)kGradWaves * n_items;                 // (n_r, 16), one class
  double* gbar = xv + n_items;                                       // (n_r, 16)
  double* xis = gbar + n_items;                                      // (n_r, 16)
  double* dxi = xis + n_items;                                       // (n_dim, n_r, 16)
  double* total = dxi + (size_t)n_dim * n_items;                     // ngal_v, sum c, dot, scratch

  grad::interp_weights(grid, draw0, weights);
  for (int item = t; item < n_items; item += kGradThreads) xis[item] = 0.0;
  for (int item = t; item < n_dim * n_items; item += kGradThreads) dxi[item] = 0.0;
  for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) gacc[item] = 0.0;
  if (backward && !likelihood)
    for (int item = t; item < n_items; item += kGradThreads)
      gbar[item] = a.g_xi[source * n_r + item / kGradDraws];
  const double g_ngal = likelihood || !backward || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source];
  double mine = 0.0;                 // thread (q, draw): ngal (q = 0), dngal/dx_d (q = 1 + d)

  // walk 0: the forward walk (and, prediction form, the adjoint with it); walk 1: the adjoint
  // walk of the likelihood form
  for (int walk = 0; walk < 2; ++walk) {
    const bool accumulate = walk == 0;
    const bool with_g = backward && (likelihood ? walk == 1 : true);
    for (int v = 0; v < n_classes; ++v) {
      a.n_h = grid.class_n_h[v];
      const double* occupation = a.occupation + (source * n_classes + v) * n_bins;
      __syncthreads();
      for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
        const int i = item / kGradDraws;
        w[item] = occupation[a.perm[i]] * a.n_h[i];
      }
      if (t < kGradDraws) w[zero_row * kGradDraws + t] = 0.0;
      for (int item = t; item < n_items; item += kGradThreads) xv[item] = 0.0;
      __syncthreads();
      if (t < kGradDraws) {
        double sum = 0.0;
        for (int i = 0; i < n_bins; ++i) sum += w[i * kGradDraws + t];
        total[t] = sum;
      }
      double c_sum = 0.0;            // thread (0, draw): sum of c_t over the class
      for (int s = grid.class_begin[v]; s < grid.class_begin[v + 1]; ++s) {
        const int32_t* node = grid.walk_node + (size_t)s * n_dim;
        a.matrix = grid.matrices[s];
        const double c = grad::interp_coef(grid, weights, node, 0, col);
        __syncthreads();
        for (int item = t; item < kGradWaves * n_items; item += kGradThreads) qpart[item] = 0.0;
        __syncthreads();
        const vjp::OneTable table{a, true};
        vjp::auto_pass(a, table, w, gbar, gsum, qpart, zero_row, true, with_g);
        if (with_g) {
          // (the rows of a wave's tiles: written above by this very lane)
          const int wave = t / 64, group = t % 64 / kGradDraws;
          for (int tile = wave; tile < a.row_tiles; tile += kGradWaves) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int i = 16 * tile + group + 4 * k;
              if (i < n_bins)
                gacc[i * kGradDraws + col] =
                    fma(c, gsum[i * kGradDraws + col], gacc[i * kGradDraws + col]);
            }
          }
        }
        __syncthreads();
        const double ngal_v = total[col];
        const double inv_ngal2 = 1.0 / (ngal_v * ngal_v);
        for (int item = t; item < n_items; item += kGradThreads) {
          const int r = item / kGradDraws;         // (item % 16 == col: 256 is a multiple of 16)
          const double* part = qpart + (size_t)r * kGradWaves * kGradDraws + col;
          double q = part[0];
#pragma unroll
          for (int k = 1; k < kGradWaves; ++k) q += part[k * kGradDraws];
          const double xi = q * inv_ngal2;
          xv[item] = fma(c, xi, xv[item]);
          if (accumulate)
            for (int d = 0; d < n_dim; ++d)
              dxi[d * n_items + item] =
                  fma(grad::interp_coef(grid, weights, node, 1 + d, col), xi, dxi[d * n_items + item]);
        }
        if (q_mine == 0) c_sum += c;
        if (accumulate && q_mine <= n_dim)
          mine = fma(grad::interp_coef(grid, weights, node, q_mine, col), ngal_v, mine);
      }
      __syncthreads();
      if (accumulate)
        for (int item = t; item < n_items; item += kGradThreads) xis[item] += xv[item];
      if (with_g) {
        if (t < kGradDraws) {
          double dot = 0.0;
          for (int r = 0; r < n_r; ++r) dot = fma(gbar[r * kGradDraws + t], xv[r * kGradDraws + t], dot);
          total[kGradDraws + t] = c_sum;
          total[2 * kGradDraws + t] = dot;
        }
        __syncthreads();
        const double ngal_v = total[col];
        const double inv_ngal = 1.0 / ngal_v;
        const double inv_ngal2 = 1.0 / (ngal_v * ngal_v);
        const double class_g_ngal = g_ngal * total[kGradDraws + col];
        const double class_dot = total[2 * kGradDraws + col];
        double* g_occupation = a.g_occupation + (draw * n_classes + v) * n_bins;
        for (int item = t; item < n_bins * kGradDraws; item += kGradThreads) {
          const int i = item / kGradDraws;
          if (draw < a.n_draws)
            g_occupation[a.perm[i]] = vjp::chain_rule(a.n_h[i], class_g_ngal, inv_ngal, inv_ngal2,
                                                      gacc[item], class_dot, 0.0, 0.0);
          gacc[item] = 0.0;
        }
      }
    }
    __syncthreads();
    if (accumulate) {
      if (!likelihood || !backward) vjp::interp_finish_x(ia, a, gbar, dxi, mine, draw0, source);
      vjp::interp_after_forward(a, xis, gbar, qpart, total + 3 * kGradDraws, draw0);
      if (!likelihood || !backward) return;
    }
  }
  vjp::interp_finish_x(ia, a, gbar, dxi, mine, draw0, source);
}

// ---- mode cross ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void vjp_interp_cross_kernel(const InterpVjpArgs ia) {
  extern __shared__ __attribute__((aligned(16))) double vjp_interp_lds[];
  VjpArgs a = ia.vjp;
  const GradInterpArgs& grid = ia.interp;
  const int t = threadIdx.x;
  const int col = t % kGradDraws, q_mine = t / kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int64_t draw = draw0 + col;
  const int64_t source = grad::clamp_draw(draw, a.n_draws);
  const int n_bins = a.n_bins, n_r = a.n_r, n_dim = grid.n_dim, n_classes = grid.n_classes;
  const bool likelihood = a.chi2_data != nullptr;
  const bool backward = a.g_occupation != nullptr;
  const int n_items = n_r * kGradDraws;
  double* weights = vjp_interp_lds;                                  // (2, n_dim, 32, 16)
  double* w = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;   // (slab, 16)
  double* y = w + (size_t)kGradCrossSlab * kGradDraws;               // (1 + n_dim, n_r, 16), one class
  double* gbar = y + (size_t)(1 + n_dim) * n_items;                  // (n_r, 16)
  double* xis = gbar + n_items;                                      // (n_r, 16)
  double* dxi = xis + n_items;                                       // (n_dim, n_r, 16)
  double* total = dxi + (size_t)n_dim * n_items;                     // ngal_v, sum c, dot, scratch

  grad::interp_weights(grid, draw0, weights);
  for (int item = t; item < n_items; item += kGradThreads) xis[item] = 0.0;
  for (int item = t; item < n_dim * n_items; item += kGradThreads) dxi[item] = 0.0;
  if (backward && !likelihood)
    for (int item = t; item < n_items; item += kGradThreads)
      gbar[item] = a.g_xi[source * n_r + item / kGradDraws];
  const double g_ngal = likelihood || !backward || a.g_ngal == nullptr ? 0.0 : a.g_ngal[source];
  double mine = 0.0;                 // thread (q, draw): ngal (q = 0), dngal/dx_d (q = 1 + d)

  for (int walk = 0; walk < 2; ++walk) {
    const bool accumulate = walk == 0;
    const bool with_g = backward && (likelihood ? walk == 1 : true);
    const int n_q = accumulate ? 1 + n_dim : 1;      // (the adjoint walk needs Y_0 alone)
    for (int v = 0; v < n_classes; ++v) {
      a.n_h = grid.class_n_h[v];
      const double* occupation = a.occupation + (source * n_classes + v) * n_bins;
      const int s_begin = grid.class_begin[v], s_end = grid.class_begin[v + 1];
      __syncthreads();
      for (int item = t; item < n_q * n_items; item += kGradThreads) y[item] = 0.0;
      double my_total = 0.0;
      for (int slab0 = 0; slab0 < n_bins; slab0 += kGradCrossSlab) {
        const int count = min(kGradCrossSlab, n_bins - slab0);
        __syncthreads();
        for (int item = t; item < count * kGradDraws; item += kGradThreads) {
          const int i = slab0 + item / kGradDraws;
          w[item] = occupation[a.perm[i]] * a.n_h[i];
        }
        __syncthreads();
        if (t < kGradDraws)
          for (int li = 0; li < count; ++li) my_total += w[li * kGradDraws + t];
        for (int s = s_begin; s < s_end; ++s) {
          const int32_t* node = grid.walk_node + (size_t)s * n_dim;
          const double* matrix = grid.matrices[s];
          for (int item = t; item < n_items; item += kGradThreads) {
            const double product = grad::cross_slab_product(matrix, n_r, item / kGradDraws, slab0,
                                                            count, w, 0, col, 0.0);
            for (int q = 0; q < n_q; ++q)
              y[q * n_items + item] =
                  fma(grad::interp_coef(grid, weights, node, q, col), product, y[q * n_items + item]);
          }
        }
      }
      if (t < kGradDraws) total[t] = my_total;
      __syncthreads();
      const double ngal_v = total[col];
      const double inv_ngal = 1.0 / ngal_v;
      if (accumulate) {
        if (q_mine <= n_dim)
          for (int s = s_begin; s < s_end; ++s)
            mine = fma(grad::interp_coef(grid, weights, grid.walk_node + (size_t)s * n_dim, q_mine,
                                         col),
                       ngal_v, mine);
        for (int item = t; item < n_items; item += kGradThreads) {
          xis[item] += y[item] * inv_ngal;
          for (int d = 0; d < n_dim; ++d)
            dxi[d * n_items + item] += y[(1 + d) * n_items + item] * inv_ngal;
        }
      }
      if (!with_g) continue;
      if (t < kGradDraws) {
        double c_sum = 0.0, dot = 0.0;
        for (int s = s_begin; s < s_end; ++s)
          c_sum += grad::interp_coef(grid, weights, grid.walk_node + (size_t)s * n_dim, 0, t);
        for (int r = 0; r < n_r; ++r)
          dot = fma(gbar[r * kGradDraws + t], y[r * kGradDraws + t] * inv_ngal, dot);
        total[kGradDraws + t] = c_sum;
        total[2 * kGradDraws + t] = dot;
      }
      __syncthreads();
      const double class_g_ngal = g_ngal * total[kGradDraws + col];
      const double class_dot = total[2 * kGradDraws + col];
      // (a column beyond the batch stores nothing, and keeps to the barriers of the walk)
      double* g_occupation = a.g_occupation + (draw * n_classes + v) * n_bins;
      const int n_stores = draw < a.n_draws ? n_bins * kGradDraws : 0;
      for (int item = t; item < n_stores; item += kGradThreads) {
        const int i = item / kGradDraws;
        double sum = 0.0;
        for (int s = s_begin; s < s_end; ++s) {
          const double* row = grid.matrices[s] + (size_t)i * n_r;
          double mine_s = 0.0;
          for (int r = 0; r < n_r; ++r) mine_s = fma(gbar[r * kGradDraws + col], row[r], mine_s);
          sum = fma(grad::interp_coef(grid, weights, grid.walk_node + (size_t)s * n_dim, 0, col),
                    mine_s, sum);
        }
        g_occupation[a.perm[i]] =
            vjp::chain_rule(a.n_h[i], class_g_ngal, inv_ngal, 0.0, 0.0, 0.0, sum, class_dot);
      }
    }
    __syncthreads();
    if (accumulate) {
      if (!likelihood || !backward) vjp::interp_finish_x(ia, a, gbar, dxi, mine, draw0, source);
      vjp::interp_after_forward(a, xis, gbar, y, total + 3 * kGradDraws, draw0);
      if (!likelihood || !backward) return;
    }
  }
  vjp::interp_finish_x(ia, a, gbar, dxi, mine, draw0, source);
}

}  // namespace tc
