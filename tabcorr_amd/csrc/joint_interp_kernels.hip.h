// Joint gradient kernel of several interpolators over one grid: (ngal, xi[, chi2, fisher]) of a
// batch of draws (theta, x) and their derivatives with respect to the model's parameters AND the
// grid's n_dim extra parameters, for ALL members in one launch (joint_interp.h: the argument block
// and the LDS budgets; joint_interp.cpp fills it in).  Geometry and pieces are those of the
// derivative kernels: kGradDraws = 16 draws per workgroup of kGradWaves = 4 waves, clamp_draw for
// the partial last workgroup.
//   1  interp_weights once; the accumulators sums (n_q, N, 16) start at zero, n_q = 6 + n_dim;
//   2  the classes in member 0's walk order, the occupations of a class ONCE for all members:
//      rows form (a member is mode auto): auto_node_loops and auto_total into the LDS rows of
//        grad_auto_kernel; per grid node s the r rows of ALL auto members, numbered consecutively
//        through the list, are dealt to the waves (wave, wave + 4, ...): auto_products against the
//        member's operand at that node, added with c_t / dc_t/dx_d into the member's rows as
//        grad_interp_auto_kernel adds them.  A cross member reads the same LDS rows: ONE fma chain
//        per (r, quantity, draw) over the bins in library order (cross_row_product), Y_q =
//        sum_t coef_{t,q} T_t . (w | dw_q) over the class's nodes, the chain rule of
//        grad_interp_cross_kernel once per class;
//      slab form (every member mode cross): the loops of grad_interp_cross_kernel -- slabs of
//        kGradCrossSlab bins outermost, cross_node_loops once per slab, then member, node s, items
//        (r, quantity, draw) into the class's y (n_q, N, 16) --, the totals, ngal and the chain
//        rule once per class;
//   3  interp_finish with N for n_r: the stores, or sums -= data, finish_chi2 and finish_fisher
//      over the n_q quantities against the (N, N) precision matrix.
// Order guarantees:
//   - ONE form per joint, chosen from the members' modes alone; a draw's results depend on the
//     draw alone (batch-invariant by construction);
//   - the order of every sum -- classes, nodes, bins, slabs, rows -- is fixed by member 0's walk
//     and does not depend on the wave or thread that runs it;
//   - prediction form: the rows of a mode-auto member (in any joint) and of every member of an
//     all-cross joint carry the bits of that member's own grad_interp_auto_kernel /
//     grad_interp_cross_kernel, provided the member's list agrees node for node with member 0's
//     (then its own walk is this one); ngal and dngal carry member 0's bits;
//   - a joint of ONE member returns that member's bits in every form: prediction, chi2, Fisher.
#pragma once

#include "grad_interp_kernels.hip.h"
#include "joint_interp.h"
#include "joint_kernels.hip.h"

namespace tc {

namespace grad {

// A workgroup of this kernel is alone on its CU where N is large (the LDS), and one chain of
// dependent fmas behind global loads per thread leaves the CU waiting: a thread runs up to
// kJointInterpChains of its items (r, quantity p, draw) at once.  Every chain is the one of
// cross_slab_product / cross_row_product, fma for fma: the sums are those of the members' own
// kernels, bit for bit.
constexpr int kJointInterpChains = 4;

// What the items of one member at one grid node are made of and where they go.
struct CrossItems {
  const double* matrix;      // (n_bins in library order, n_r)
  int n_r;
  // slab form: the slab (6, kGradCrossSlab, 16) and its bins; rows form: the rows of every bin
  const double* w;
  int slab0, count;
  int n_bins, n_central, zero_row;
  double* y;                 // row 0 of the member in the class's products, at the draw's column
  size_t stride;             // between the quantities of y
};

// The items base + t, base + t + 256, ... (C of them, those below n_items) of a thread: C
// products, then c_t times each into y -- and the value's product (p = 0) with dc_t/dx_d into
// the n_dim accumulators of d/dx.
template <int NP, int C, bool ROWS>
__device__ __forceinline__ void cross_items(const GradInterpArgs& ia, const double* weights,
                                            const int32_t* node, const CrossItems& it, int base,
                                            int n_items) {
  constexpr int NQ = NP + 1;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  if (base + t >= n_items) return;
  int r[C], p[C];
  double sum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    // (a chain beyond the last item repeats the first one and stores nothing)
    const int item = base + t + c * kGradThreads < n_items ? base + t + c * kGradThreads : base + t;
    r[c] = item / (NQ * kGradDraws);
    p[c] = item / kGradDraws % NQ;
    sum[c] = 0.0;
  }
  if (ROWS) {
    for (int i = 0; i < it.n_bins; ++i) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        sum[c] = fma(it.matrix[(size_t)i * it.n_r + r[c]],
                     it.w[auto_row<NP>(i, p[c], it.n_bins, it.n_central, it.zero_row) *
                              kGradDraws + col],
                     sum[c]);
    }
  } else {
    const double* column = it.matrix + (size_t)it.slab0 * it.n_r;
    for (int li = 0; li < it.count; ++li) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        sum[c] = fma(column[(size_t)li * it.n_r + r[c]],
                     it.w[((size_t)p[c] * kGradCrossSlab + li) * kGradDraws + col], sum[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (base + t + c * kGradThreads >= n_items) break;
    double* slot = it.y + (size_t)r[c] * kGradDraws;
    const int q = p[c];
    slot[q * it.stride] = fma(interp_coef(ia, weights, node, 0, col), sum[c], slot[q * it.stride]);
    if (q == 0)
      for (int e = 0; e < ia.n_dim; ++e)
        slot[(NQ + e) * it.stride] = fma(interp_coef(ia, weights, node, 1 + e, col), sum[c],
                                         slot[(NQ + e) * it.stride]);
  }
}

// All NQ n_r 16 items of a member at a node, walked by the workgroup in rounds of up to
// kJointInterpChains x 256 items -- as many chains as there are items left for, so that no
// round repeats work.
template <int NP, bool ROWS>
__device__ __forceinline__ void cross_member(const GradInterpArgs& ia, const double* weights,
                                             const int32_t* node, const CrossItems& it) {
  const int n_items = (NP + 1) * it.n_r * kGradDraws;
  int base = 0;
  while (base < n_items) {
    const int rounds = (n_items - base + kGradThreads - 1) / kGradThreads;
    if (rounds >= 4) {
      cross_items<NP, 4, ROWS>(ia, weights, node, it, base, n_items);
      base += 4 * kGradThreads;
    } else if (rounds == 3) {
      cross_items<NP, 3, ROWS>(ia, weights, node, it, base, n_items);
      base += 3 * kGradThreads;
    } else if (rounds == 2) {
      cross_items<NP, 2, ROWS>(ia, weights, node, it, base, n_items);
      base += 2 * kGradThreads;
    } else {
      cross_items<NP, 1, ROWS>(ia, weights, node, it, base, n_items);
      base += kGradThreads;
    }
  }
}

// ---- rows form ------------------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void joint_interp_rows(const JointInterpArgs& j) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  const GradInterpArgs& ia = j.interp;
  GradArgs a = ia.table;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central, n_total = a.n_r, n_dim = ia.n_dim;
  const int n_cross = j.n_r_cross;
  const int n_q = NQ + n_dim;
  const int zero_row = grad_auto_rows(n_bins, n_central, NP) - 1;
  double* w = grad_lds;                                               // (rows, 16), one class
  double* total = w + (size_t)(zero_row + 1) * kGradDraws;            // (6, 16), one class
  double* weights = total + NQ * kGradDraws;                           // (2, n_dim, 32, 16)
  double* sums = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;   // (n_q, N, 16)
  double* y = sums + (size_t)n_q * n_total * kGradDraws;              // (n_q, n_cross, 16), one class
  const fm::Consts k = fm::make_consts();
  interp_weights(ia, draw0, weights);
  for (int item = t; item < n_q * n_total * kGradDraws; item += kGradThreads) sums[item] = 0.0;
  double my_ngal = 0.0;                                               // thread = (q, draw)
  const int wave = t / 64, group = t % 64 / kGradDraws;
  int n_auto = 0;
  for (int m = 0; m < j.n_members; ++m)
    if (j.mode[m] == TC_MODE_AUTO) n_auto += j.n_r[m];
  const size_t stride = (size_t)n_total * kGradDraws;
  const size_t y_stride = (size_t)n_cross * kGradDraws;
  for (int v = 0; v < ia.n_classes; ++v) {
    set_class(a, ia, v);
    __syncthreads();
    {
      const Draw d = load_draw<NP>(a, k, draw0 + col);
      auto_node_loops<NP>(a, k, d, w, zero_row);
    }
    for (int item = t; item < n_q * n_cross * kGradDraws; item += kGradThreads) y[item] = 0.0;
    __syncthreads();
    if (t < NQ * kGradDraws)
      total[t] = auto_total<NP>(w, t / kGradDraws, col, n_bins, n_central, zero_row);
    __syncthreads();
    const double ngal = total[col];
    const double inv_ngal = 1.0 / ngal;
    const double inv_ngal2 = 1.0 / (ngal * ngal);
    for (int s = ia.class_begin[v]; s < ia.class_begin[v + 1]; ++s) {
      const int32_t* node = ia.walk_node + (size_t)s * n_dim;
      if (t < n_q * kGradDraws) {
        const int q = t / kGradDraws;
        my_ngal = fma(interp_coef(ia, weights, node, interp_which<NP>(q), col),
                      total[interp_quantity<NP>(q) * kGradDraws + col], my_ngal);
      }
      const double c = interp_coef(ia, weights, node, 0, col);
      // mode auto: row g of the auto members' rows, numbered through the list
      for (int g = wave; g < n_auto; g += kGradWaves) {
        int m = 0, r = g;
        for (;; ++m) {
          if (j.mode[m] != TC_MODE_AUTO) continue;
          if (r < j.n_r[m]) break;
          r -= j.n_r[m];
        }
        a.matrix = j.matrices[m][s];
        double acc[NQ];
        auto_products<NP>(a, w, r, zero_row, acc);
        const double xi = auto_xi(acc, inv_ngal2);
        if (group == 0) {
          double* slot = sums + (size_t)(j.r_offset[m] + r) * kGradDraws + col;
          slot[0] = fma(c, xi, slot[0]);
#pragma unroll
          for (int p = 1; p < NQ; ++p)
            slot[p * stride] = fma(c, auto_dxi(acc, p, xi, total, col, inv_ngal, inv_ngal2),
                                   slot[p * stride]);
          for (int d = 0; d < n_dim; ++d)
            slot[(NQ + d) * stride] = fma(interp_coef(ia, weights, node, 1 + d, col), xi,
                                         slot[(NQ + d) * stride]);
        }
      }
      // mode cross: items (r, quantity p, draw) of every cross member, one chain over the bins
      // each; the value's product (p = 0) also feeds the n_dim accumulators of d/dx
      if (n_cross == 0) continue;
      for (int m = 0; m < j.n_members; ++m) {
        if (j.mode[m] != TC_MODE_CROSS) continue;
        const double* matrix = j.matrices[m][s];
        const int n_r = j.n_r[m];
        const CrossItems items{matrix, n_r, w, 0, 0, n_bins, n_central, zero_row,
                               y + (size_t)j.cross_offset[m] * kGradDraws + col, y_stride};
        cross_member<NP, true>(ia, weights, node, items);
      }
    }
    if (n_cross == 0) continue;
    __syncthreads();
    // xi = Y_0 / ngal, dxi_k = (Y_k - xi dngal_k) / ngal, d/dx_d = Y_(6 + d) / ngal
    for (int m = 0; m < j.n_members; ++m) {
      if (j.mode[m] != TC_MODE_CROSS) continue;
      const int n_r = j.n_r[m];
      for (int item = t; item < n_q * n_r * kGradDraws; item += kGradThreads) {
        const int r = item / (n_q * kGradDraws), q = item / kGradDraws % n_q;
        const double* from = y + (size_t)(j.cross_offset[m] + r) * kGradDraws + col;
        const double xi = from[0] * inv_ngal;
        double value = xi;
        if (q >= NQ)
          value = from[q * y_stride] * inv_ngal;
        else if (q > 0)
          value = (from[q * y_stride] - xi * total[q * kGradDraws + col]) * inv_ngal;
        sums[q * stride + (size_t)(j.r_offset[m] + r) * kGradDraws + col] += value;
      }
    }
  }
  __syncthreads();
  interp_finish(a, n_q, my_ngal, sums, draw0);
}

// ---- slab form ------------------------------------------------------------------------------------
template <int NP>
__device__ __forceinline__ void joint_interp_slabs(const JointInterpArgs& j) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  const GradInterpArgs& ia = j.interp;
  GradArgs a = ia.table;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_total = a.n_r, n_dim = ia.n_dim;
  const int n_q = NQ + n_dim;
  const int n_items = n_q * n_total * kGradDraws;
  double* w = grad_lds;                                               // (6, slab, 16)
  double* total = w + NQ * kGradCrossSlab * kGradDraws;                // (6, 16), one class
  double* weights = total + NQ * kGradDraws;                           // (2, n_dim, 32, 16)
  double* y = weights + (size_t)2 * n_dim * kGradMaxAxis * kGradDraws;      // (n_q, N, 16), one class
  double* sums = y + n_items;                                         // (n_q, N, 16)
  const fm::Consts k = fm::make_consts();
  const Draw d = load_draw<NP>(a, k, draw0 + col);
  interp_weights(ia, draw0, weights);
  for (int item = t; item < n_items; item += kGradThreads) sums[item] = 0.0;
  double my_ngal = 0.0;                                               // thread = (q, draw)
  const size_t stride = (size_t)n_total * kGradDraws;
  for (int v = 0; v < ia.n_classes; ++v) {
    set_class(a, ia, v);
    const int s_begin = ia.class_begin[v], s_end = ia.class_begin[v + 1];
    __syncthreads();
    for (int item = t; item < n_items; item += kGradThreads) y[item] = 0.0;
    double my_total = 0.0;
    for (int slab0 = 0; slab0 < n_bins; slab0 += kGradCrossSlab) {
      const int count = min(kGradCrossSlab, n_bins - slab0);
      __syncthreads();
      cross_node_loops<NP>(a, k, d, slab0, count, w);
      __syncthreads();
      if (t < NQ * kGradDraws) {
        const int p = t / kGradDraws;
        for (int li = 0; li < count; ++li) my_total += w[(p * kGradCrossSlab + li) * kGradDraws + col];
      }
      for (int m = 0; m < j.n_members; ++m) {
        const int n_r = j.n_r[m];
        for (int s = s_begin; s < s_end; ++s) {
          const int32_t* node = ia.walk_node + (size_t)s * n_dim;
          const double* matrix = j.matrices[m][s];
          // item = (r, quantity p, draw) as in grad_interp_cross_kernel, the rows the member's
          const CrossItems items{matrix, n_r, w, slab0, count, n_bins, 0, 0,
                                 y + (size_t)j.r_offset[m] * kGradDraws + col, stride};
          cross_member<NP, false>(ia, weights, node, items);
        }
      }
    }
    if (t < NQ * kGradDraws) total[t] = my_total;
    __syncthreads();
    if (t < n_q * kGradDraws) {
      const int q = t / kGradDraws;
      for (int s = s_begin; s < s_end; ++s)
        my_ngal = fma(interp_coef(ia, weights, ia.walk_node + (size_t)s * n_dim,
                                  interp_which<NP>(q), col),
                      total[interp_quantity<NP>(q) * kGradDraws + col], my_ngal);
    }
    // xi = Y_0 / ngal, dxi_k = (Y_k - xi dngal_k) / ngal, d/dx_d = Y_(6 + d) / ngal
    const double inv_ngal = 1.0 / total[col];
    for (int item = t; item < n_items; item += kGradThreads) {
      const int r = item / (n_q * kGradDraws), q = item / kGradDraws % n_q;
      const size_t slot = ((size_t)q * n_total + r) * kGradDraws + col;
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
  interp_finish(a, n_q, my_ngal, sums, draw0);
}

}  // namespace grad

template <int NP, int FORM>
__global__ __launch_bounds__(kGradThreads) void grad_joint_interp_kernel(const JointInterpArgs j) {
  if (FORM == kJointInterpRows)
    grad::joint_interp_rows<NP>(j);
  else
    grad::joint_interp_slabs<NP>(j);
}

}  // namespace tc
