// Reverse-mode derivative of predict(occupation) (tabcorr.py:616-650): the vector-Jacobian
// product with respect to the occupation array, for every occupation model at once.  The argument
// block of the two kernels (vjp_kernels.hip.h) and their LDS budget; plain C++ for the host-only
// units that fill these in.
//
// With n one draw's occupation, w = n . n_h, ngal = sum_i w_i and the cotangents g_ngal (scalar),
// g_r (n_r):
//   mode auto   q_r = w^T S_r w, xi_r = q_r / ngal^2, U_r = S_r w (the dense operand of grad.h)
//     g_n,i = n_h,i [ g_ngal + (2 / ngal^2) sum_r g_r U_ri - (2 / ngal) sum_r g_r xi_r ]
//   mode cross  xi_r = T_r . w / ngal
//     g_n,i = n_h,i [ g_ngal + (1 / ngal) sum_r g_r T_ri - (1 / ngal) sum_r g_r xi_r ]
// Likelihood form: g = 2 P_sym (xi - data) with P_sym = (P + P^T) / 2 and g_ngal = 0, formed in
// the launch from its own xi; the results are chi2 and dchi2 / dn.
#pragma once

#include <cstddef>
#include <cstdint>

#include "grad.h"

namespace tc {

struct VjpArgs {
  const double* occupation;  // (n_draws, n_bins), rows in the reference's gal_type order
  int64_t n_draws;
  int n_bins;
  int n_r;
  const int32_t* perm;       // (n_bins) reference row of library bin i
  const double* n_h;         // (n_bins) library order
  // mode auto: the dense operand layout of grad.h; mode cross: (n_bins in library order, n_r)
  const double* matrix;
  int row_tiles;             // blocks of 16 matrix rows
  int k_steps;               // steps of 4 matrix columns
  const double* g_ngal;      // (n_draws), or NULL = 0
  const double* g_xi;        // (n_draws, n_r); NULL: the likelihood form
  const double* chi2_data;   // likelihood form: data (n_r), then the precision matrix (n_r, n_r)
  double* ngal;              // (n_draws)
  double* xi;                // (n_draws, n_r); not written by the likelihood form
  double* chi2;              // (n_draws), likelihood form
  double* g_occupation;      // (n_draws, n_bins), reference row order
};

// ---- LDS, in rows of kGradDraws doubles ---------------------------------------------------------
// Both kernels keep per r bin: the cotangent g_r, xi_r (the likelihood form: the residual) and the
// products that become xi -- in mode auto one partial q_r per wave, added in wave order; and two
// rows for ngal and sum_r g_r xi_r.  The same for both forms of a call.
// vjp_auto_kernel: w of every bin and one row of zeros (the padding of the matrix up to whole
// tiles), and sum_r g_r U_ri of every bin.
constexpr int vjp_auto_rows(int n_bins, int n_r) {
  return 2 * n_bins + 1 + (kGradWaves + 2) * n_r + 2;
}
constexpr size_t vjp_auto_lds_bytes(int n_bins, int n_r) {
  return (size_t)vjp_auto_rows(n_bins, n_r) * kGradDraws * sizeof(double);
}
// vjp_cross_kernel: one slab of w (kGradCrossSlab bins), any number of bins.
constexpr size_t vjp_cross_lds_bytes(int n_r) {
  return ((size_t)kGradCrossSlab + 3 * (size_t)n_r + 2) * kGradDraws * sizeof(double);
}

// ---- the occupation seam of an interpolator (interp_vjp_kernels.hip.h) ---------------------------
// Tables t on a grid with the tensor-product spline weights c_t(x), classes v of tables with one
// halo table; a draw's occupation is (n_classes, n_bins), class v's row in the gal_type order of
// that class's tables.  With w = n_v . n_h,v and ngal_t = sum w (the class's):
//   ngal = sum_t c_t ngal_t, xi_r = sum_t c_t xi_t,r
//   g_n[v,i] = n_h,v,i sum_{t in v} c_t [ the bracket of the table formulas above ]
//   g_x[d] = sum_t (dc_t/dx_d) [ g_ngal ngal_t + sum_r g_r xi_t,r ]
// Likelihood form: g = 2 P_sym (xi - data) of the INTERPOLATED xi, g_ngal = 0; it also returns
// dngal_dx[d] = sum_t (dc_t/dx_d) ngal_t.
struct InterpVjpArgs {
  // the grid, the walk (class_begin, walk_node, matrices) and class_n_h as for the gradient
  // kernels; of `table` only n_draws is read (grad::interp_weights)
  GradInterpArgs interp;
  // occupation and g_occupation (n_draws, n_classes, n_bins); n_h and matrix are set per class
  // and per table by the kernel.  g_occupation NULL: the forward-only form
  VjpArgs vjp;
  double* g_x;               // (n_draws, n_dim): the likelihood form's dchi2 / dx
  double* dngal_dx;          // (n_draws, n_dim), likelihood form only
};

// LDS rows of kGradDraws doubles that both kernels keep: the weights and derivative weights of
// every axis; per r bin the cotangent, the interpolated xi (the likelihood form: then the
// residual) and the n_dim accumulators of dxi_r / dx_d; four rows of per-draw sums.
constexpr int interp_vjp_common_rows(int n_r, int n_dim) {
  return 2 * n_dim * kGradMaxAxis + (2 + n_dim) * n_r + 4;
}
// vjp_interp_auto_kernel: w of every bin of the class in flight and one row of zeros, per bin
// the table's sum_r g_r U_ri and the class accumulator of g_n, one partial q_r per wave and the
// class's share of xi.
constexpr int interp_vjp_auto_rows(int n_bins, int n_r, int n_dim) {
  return 3 * n_bins + 1 + (kGradWaves + 1) * n_r + interp_vjp_common_rows(n_r, n_dim);
}
constexpr size_t interp_vjp_auto_lds_bytes(int n_bins, int n_r, int n_dim) {
  return (size_t)interp_vjp_auto_rows(n_bins, n_r, n_dim) * kGradDraws * sizeof(double);
}
// vjp_interp_cross_kernel: one slab of w, and the class's weighted products (1 + n_dim, n_r);
// any number of bins.
constexpr int interp_vjp_cross_rows(int n_r, int n_dim) {
  return kGradCrossSlab + (1 + n_dim) * n_r + interp_vjp_common_rows(n_r, n_dim);
}
constexpr size_t interp_vjp_cross_lds_bytes(int n_r, int n_dim) {
  return (size_t)interp_vjp_cross_rows(n_r, n_dim) * kGradDraws * sizeof(double);
}

}  // namespace tc
