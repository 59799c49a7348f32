// Joint gradient kernel: (ngal, xi[, chi2, fisher]) of a batch of draws and their derivatives
// for SEVERAL tables that share one halo table, in one launch (joint.h: the argument block and the
// LDS budget; joint.cpp fills it in).  Geometry and pieces are those of grad_kernels.hip.h:
// kGradDraws = 16 draws per workgroup of kGradWaves = 4 waves.
//   1  once per workgroup: the node loops of every bin and the totals (auto_occupations) -- w,
//      dw, ngal and dngal do not depend on the table;
//   2  per table in list order, into its rows r_offset[t] .. of the N concatenated ones:
//      mode auto   auto_products against the table's dense operand, then auto_xi / auto_dxi; the
//                  r rows of ALL auto tables are numbered consecutively and dealt to the waves
//                  (wave, wave + 4, ...), so that a table of 3 r bins leaves no wave idle;
//      mode cross  xi_r = T_r . w / ngal: ONE fma chain per (r, quantity, draw) over the bins in
//                  library order, read from the LDS rows (a row a bin does not keep is the row of
//                  zeros); the items (r, quantity, draw) are walked by the workgroup.  An item of a
//                  derivative runs the value's chain too rather than wait for it at a barrier;
//   3  the prediction's arrays, or finish_chi2 / finish_fisher against the (N, N) precision.
// Order guarantees:
//   - ONE form: a draw's results depend on the draw alone (batch-invariant by construction);
//   - the arithmetic of a result row does not depend on the wave or thread that runs it;
//   - the pieces and their order are those of the table kernels: a joint of one mode-auto table
//     returns the bits of grad_auto_kernel on that table, and a joint of one mode-cross table those
//     of grad_cross_kernel, whose slabs amount to the one fma chain in bin order (adding the
//     product with the row of zeros leaves a sum as it is).
#pragma once

#include "grad_kernels.hip.h"
#include "joint.h"

namespace tc {

namespace grad {

// T_r . (quantity p of the bins) of one draw: one fma chain over the bins in library order.
template <int NP>
__device__ __forceinline__ double cross_row_product(const double* matrix, int n_r, int r,
                                                    const double* w, int p, int col, int n_bins,
                                                    int n_central, int zero_row) {
  double sum = 0.0;
  for (int i = 0; i < n_bins; ++i)
    sum = fma(matrix[(size_t)i * n_r + r],
              w[auto_row<NP>(i, p, n_bins, n_central, zero_row) * kGradDraws + col], sum);
  return sum;
}

}  // namespace grad

template <int NP>
__global__ __launch_bounds__(kGradThreads) void grad_joint_kernel(const JointArgs j) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  const GradArgs& a = j.grad;
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central;
  const int zero_row = grad_auto_rows(n_bins, n_central, NP) - 1;
  double* w = grad_lds;                                       // (rows, 16)
  double* total = w + (size_t)(zero_row + 1) * kGradDraws;    // (6, 16)
  double* stash = total + NQ * kGradDraws;                     // (6, N, 16), likelihood only
  const fm::Consts k = fm::make_consts();

  // phase 1, once for all tables
  grad::auto_occupations<NP>(a, k, w, total, draw0, zero_row);

  const int wave = t / 64;
  const double ngal = total[col];
  const double inv_ngal = 1.0 / ngal;
  const double inv_ngal2 = 1.0 / (ngal * ngal);
  const int64_t draw = draw0 + col;

  // phase 2, mode auto: row g of the auto tables' rows, numbered through the list
  int n_auto = 0;
  for (int table = 0; table < j.n_tables; ++table)
    if (j.mode[table] == TC_MODE_AUTO) n_auto += j.n_r[table];
  for (int g = wave; g < n_auto; g += kGradWaves) {
    int table = 0, r = g;
    for (;; ++table) {
      if (j.mode[table] != TC_MODE_AUTO) continue;
      if (r < j.n_r[table]) break;
      r -= j.n_r[table];
    }
    GradArgs of_table = a;
    of_table.matrix = j.matrix[table];
    double acc[NQ];
    grad::auto_products<NP>(of_table, w, r, zero_row, acc);
    grad::auto_store_row<NP>(a, acc, total, stash, draw, j.r_offset[table] + r, inv_ngal,
                             inv_ngal2);
  }

  // phase 2, mode cross: items (r, quantity, draw) of every cross table
  for (int table = 0; table < j.n_tables; ++table) {
    if (j.mode[table] != TC_MODE_CROSS) continue;
    const double* matrix = j.matrix[table];
    const int n_r = j.n_r[table];
    const int n_items = NQ * n_r * kGradDraws;
    for (int item = t; item < n_items; item += kGradThreads) {
      // (item % 16 == col: 256 is a multiple of 16)
      const int r = item / (NQ * kGradDraws), p = item / kGradDraws % NQ;
      const double y0 =
          grad::cross_row_product<NP>(matrix, n_r, r, w, 0, col, n_bins, n_central, zero_row);
      const double xi = grad::cross_xi(y0, inv_ngal);
      double value = xi;
      if (p != 0) {
        const double y =
            grad::cross_row_product<NP>(matrix, n_r, r, w, p, col, n_bins, n_central, zero_row);
        value = grad::cross_dxi(y, xi, total[p * kGradDraws + col], inv_ngal);
      }
      grad::store_result<NP>(a, stash, draw, col, j.r_offset[table] + r, p, value);
    }
  }

  // phase 3: a.n_r = N is the stride of the stash and the dimension of the precision matrix
  if (a.xi == nullptr) {
    __syncthreads();
    grad::finish_chi2(a, stash, draw0, NQ);
    grad::finish_fisher(a, stash, draw0, NQ);
  }
}

}  // namespace tc
