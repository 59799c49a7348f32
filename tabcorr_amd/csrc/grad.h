// Analytic gradients of (ngal, xi, chi2) with respect to the five Zheng07 parameters -- or, for
// the model decorated with Heaviside assembly bias at the median split, those and the two
// strengths, or the eleven parameters of the Leauthaud11 family (`n_params` = 5, 7 or 11 below, a
// template parameter of the kernels) --: the
// argument block of the gradient kernels (grad_kernels.hip.h), their LDS budget and the dense
// matrix-operand layout of a mode-auto table.  Plain C++ for the host-only units that fill these
// in (spline.h, which it includes, is compiled for the device too).
//
// With w = n_h <N> and S_r the symmetric matrix of one r bin, q_r = w^T S_r w and
// dq_r / dtheta_k = 2 (dw / dtheta_k)^T (S_r w): ONE dense product U_r = S_r W per tile of draws
// gives the value and all five derivatives by dot products.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "kernel_args.h"
#include "spline.h"

namespace tc {

constexpr int kGradParams = 5;        // logMmin, sigma_logM, logM0, logM1, alpha
// ... and the strengths of the centrals' and the satellites' assembly bias (the decorated model):
// N_cen' = N + s_b c(A_cen) min(N, 1 - N) per node and N_sat' = (1 + s_b c(A_sat)) N with c the
// clip to [-1, 1] and s_b = +1 for a bin whose secondary percentile lies above 0.5, else -1
constexpr int kGradParamsAssembias = 7;
// The Leauthaud11 family (grad_leauthaud11.h): logm0, logm1, beta, delta, gamma, scatter,
// alphasat, bsat, betasat, bcut, betacut -- the first eleven of the fourteen theta columns of the
// forward kernels; threshold, h and h_s behind them are inputs and are not differentiated.
constexpr int kGradParamsLeauthaud11 = 11;
constexpr int kGradThetaLeauthaud11 = 14;
// theta columns of a draw: the differentiated parameters, and for Leauthaud11 the three inputs
constexpr int grad_theta_columns(int n_params) {
  return n_params == kGradParamsLeauthaud11 ? kGradThetaLeauthaud11 : n_params;
}
constexpr int kGradDraws = 16;        // draws per workgroup: the N of one v_mfma_f64_16x16x4_f64
constexpr int kGradWaves = 4;
constexpr int kGradThreads = 64 * kGradWaves;
constexpr int kGradCrossSlab = 64;    // mode cross: bins whose w and dw one LDS slab holds
// ... of the INTERPOLATOR's cross kernel, a trait of the family: its LDS also keeps the products
// of the class in flight and the accumulators, (2 (n_params + 1 + n_dim), n_r) rows, and with the
// twelve quantities of the Leauthaud11 family a slab of 64 bins (98 KB) would leave no room for the
// 14 r bins of a grid of three dimensions.  Half the slab does (126 KB).
constexpr int grad_interp_cross_slab(int n_params) {
  return n_params == kGradParamsLeauthaud11 ? 32 : kGradCrossSlab;
}

struct GradArgs {
  // (n_draws, 5) -- 7 wherever 5 stands below, decorated; Leauthaud11: (n_draws, 14), and 11
  // wherever 5 stands below
  const double* theta;
  int64_t n_draws;
  int n_bins;
  int n_central;
  int n_gauss;
  int n_r;
  int modulate;              // modulate_with_cenocc
  const double* log_m;       // quadrature constants as in OccArgs (library bin order)
  const double* m;
  const double* weight;
  const double* n_h;
  const double* math_table;  // fastmath.h tables, read from global memory
  // mode auto: the dense operand layout below; mode cross: (n_bins in library order, n_r)
  const double* matrix;
  int row_tiles;             // blocks of 16 matrix rows
  int k_steps;               // steps of 4 matrix columns
  double* ngal;              // (n_draws)
  double* dngal;             // (n_draws, 5)
  double* xi;                // (n_draws, n_r); NULL: the likelihood is finished in the launch
  double* dxi;               // (n_draws, 5, n_r)
  const double* chi2_data;   // data (n_r), then the precision matrix (n_r, n_r)
  double* chi2;              // (n_draws)
  double* dchi2;             // (n_draws, 5)
  // Fisher matrix of the likelihood, fisher[k][l] = dxi_k^T P_sym dxi_l over the differentiated
  // quantities (n_draws, 5, 5) -- (n_draws, 5 + n_dim, 5 + n_dim) for an interpolator; NULL: not
  // asked for.  Only with the likelihood (xi NULL): grad_kernels.hip.h: finish_fisher
  double* fisher;
  const double* percentile;  // (n_bins) sec_haloprop_percentile, library bin order; decorated only
};

// ---- LDS of grad_auto_kernel ------------------------------------------------------------------
// Rows of kGradDraws doubles.  A central bin keeps (w, dw/dlogMmin, dw/dsigma), a satellite bin
// w and all five derivatives (three of them zero unless modulate_with_cenocc); one shared row of
// zeros stands for everything else: the derivatives a central bin does not have and the padding
// of the matrix up to whole tiles.  Decorated (n_params = 7): a central bin keeps a fourth row,
// dw/dA_cen, a satellite bin a seventh, dw/dA_sat.
// Leauthaud11 (n_params = 11): a central bin keeps w and its six non-zero derivatives (the five
// relation parameters and scatter), a satellite bin w and all eleven.
//
// The family trait: the rows a central and a satellite bin keep, and the row (within its bin's)
// of quantity p = 0 (w), 1 + k (dw/dtheta_k); -1: the bin does not keep it, it is the row of zeros.
constexpr int grad_central_rows(int n_params) {
  return n_params == kGradParams ? 3 : n_params == kGradParamsAssembias ? 4 : 7;
}
constexpr int grad_satellite_rows(int n_params) {
  return n_params == kGradParams ? 6 : n_params == kGradParamsAssembias ? 7 : 12;
}
constexpr int grad_central_row(int n_params, int p) {
  if (n_params == kGradParamsLeauthaud11) return p < 7 ? p : -1;
  if (p < 3) return p;
  return n_params == kGradParamsAssembias && p == n_params - 1 ? 3 : -1;      // A_cen
}
constexpr int grad_satellite_row(int n_params, int p) {
  if (n_params != kGradParamsAssembias) return p;
  if (p == n_params - 1) return -1;                                            // A_cen
  return p == n_params ? n_params - 1 : p;                                     // A_sat
}
// Whether a bin's rows are simply its first quantities, in order (plain, Leauthaud11), so that they
// are written as one run; the decorated rows skip a quantity.
constexpr bool grad_rows_in_order(int n_params) { return n_params != kGradParamsAssembias; }
constexpr int grad_auto_rows(int n_bins, int n_central, int n_params = kGradParams) {
  return grad_central_rows(n_params) * n_central +
         grad_satellite_rows(n_params) * (n_bins - n_central) + 1;
}
// ... then the totals (6, kGradDraws) and, for the likelihood, (6, n_r, kGradDraws) residuals
// and derivatives -- 8 for 6 where decorated, 12 for the Leauthaud11 family, here and below
constexpr size_t grad_auto_lds_bytes(int n_bins, int n_central, int n_r, bool chi2,
                                     int n_params = kGradParams) {
  return ((size_t)grad_auto_rows(n_bins, n_central, n_params) + (n_params + 1) +
          (chi2 ? (n_params + 1) * (size_t)n_r : 0)) *
         kGradDraws * sizeof(double);
}
// grad_cross_kernel: one slab (6, kGradCrossSlab, kGradDraws), the products (6, n_r, kGradDraws)
// and the totals
constexpr size_t grad_cross_lds_bytes(int n_r, int n_params = kGradParams) {
  return (size_t)(n_params + 1) * ((size_t)kGradCrossSlab + (size_t)n_r + 1) * kGradDraws *
         sizeof(double);
}

// ---- dense operand layout of a mode-auto table ------------------------------------------------
// Per r bin, block of 16 rows and step of 4 columns 64 doubles: [l] = S_r[16 block + l % 16]
// [4 step + l / 16], the A operand of v_mfma_f64_16x16x4_f64 in lane order (one coalesced
// 512-byte load per instruction); zeros beyond the last bin.
inline int grad_row_tiles(int n_bins) { return (n_bins + 15) / 16; }
inline int grad_k_steps(int n_bins) { return (n_bins + 3) / 4; }
inline size_t grad_operand_doubles(int n_bins, int n_r) {
  return (size_t)n_r * grad_row_tiles(n_bins) * grad_k_steps(n_bins) * 64;
}
inline size_t grad_operand_index(int n_bins, int r, int i, int j) {
  return (((size_t)r * grad_row_tiles(n_bins) + i / 16) * grad_k_steps(n_bins) + j / 4) * 64 +
         (size_t)(j % 4) * 16 + i % 16;
}
// `packed`: (n_r, n_bins (n_bins + 1) / 2) lower triangles, p = i (i + 1) / 2 + j with j <= i
// (tabcorr.py:770-806), WITHOUT the pair prefactor.
inline void build_grad_operand(int n_bins, int n_r, const double* packed,
                               std::vector<double>& out) {
  const size_t n_pairs = (size_t)n_bins * (n_bins + 1) / 2;
  out.assign(grad_operand_doubles(n_bins, n_r), 0.0);
  for (int r = 0; r < n_r; ++r)
    for (int i = 0; i < n_bins; ++i)
      for (int j = 0; j <= i; ++j) {
        const double value = packed[(size_t)r * n_pairs + (size_t)i * (i + 1) / 2 + j];
        out[grad_operand_index(n_bins, r, i, j)] = value;
        out[grad_operand_index(n_bins, r, j, i)] = value;
      }
}

// ---- gradients of an interpolator (grad_interp_kernels.hip.h) -----------------------------------
// The interpolated result is linear in the per-table results: with c_t(x) the tensor-product
// spline weight of table t, d/dtheta_k = sum_t c_t d(ngal_t, xi_t)/dtheta_k and d/dx_d =
// sum_t (dc_t/dx_d) (ngal_t, xi_t).  One launch per batch walks the tables class by class.

// (the spline weights c_t and dc_t/dx_d of an axis: spline.h: spline_weights)

// what tc_interp_create admits (kernel_args.h) sizes the argument arrays and the weight rows
constexpr int kGradMaxDim = kMaxInterpDim;
constexpr int kGradMaxAxis = kMaxInterpAxis;

struct GradInterpArgs {
  // theta, the sizes, the flags, math_table, row_tiles / k_steps and the result arrays as for one
  // table: dngal (n_draws, 5 + n_dim), dxi (n_draws, 5 + n_dim, n_r), dchi2 (n_draws, 5 + n_dim),
  // the five Zheng07 parameters first (7 decorated, 11 of the Leauthaud11 family for 5).  log_m,
  // m, weight, n_h and matrix are set per class and per table by the kernel.
  GradArgs table;
  const double* x;                    // (n_draws, n_dim)
  int n_dim;
  int n_classes;
  int n_axis[kGradMaxDim];
  int axis_offset[kGradMaxDim];       // offset of xp_d in xp
  int a_offset[kGradMaxDim];          // offset of a_d in a
  const double* xp;
  const double* a;
  // the walk: the tables class by class, inside a class in list order -- fixed by the
  // interpolator; class v is walk[class_begin[v] .. class_begin[v + 1])
  const int32_t* class_begin;         // (n_classes + 1)
  const int32_t* walk_node;           // (K, n_dim) grid node of every table, in walk order
  const double* const* matrices;      // (K) GradArgs::matrix of every table, in walk order
  const double* const* class_log_m;   // (n_classes) quadrature constants and n_h of every class
  const double* const* class_m;
  const double* const* class_weight;
  const double* const* class_n_h;
  const double* const* class_percentile;   // decorated only; else NULL
};

// The axes an interpolator may have for the family: both kernels finish ngal, chi2 and their
// derivatives with one thread per (quantity, draw), kGradThreads / kGradDraws = 16 quantities at
// the most, of which the family takes n_params + 1 -- every grid tc_interp_create admits for 5 and
// 7 parameters, four axes for the eleven of the Leauthaud11 family.
constexpr int grad_interp_max_dim(int n_params) {
  return kGradThreads / kGradDraws - (n_params + 1) < kGradMaxDim
             ? kGradThreads / kGradDraws - (n_params + 1)
             : kGradMaxDim;
}

// LDS rows of kGradDraws doubles that both interpolator kernels keep: the weights and derivative
// weights of every axis, and the (6 + n_dim) accumulators of xi per r bin ((8 + n_dim) where
// decorated, (12 + n_dim) for the Leauthaud11 family).  The likelihood is finished in the
// accumulators themselves (`chi2` costs nothing).
constexpr size_t grad_interp_common_rows(int n_r, int n_dim, int n_params = kGradParams) {
  return 2 * (size_t)n_dim * kGradMaxAxis + (size_t)(n_params + 1 + n_dim) * n_r;
}
// grad_interp_auto_kernel: the rows of grad_auto_kernel for one class at a time, its totals.
constexpr size_t grad_interp_auto_lds_bytes(int n_bins, int n_central, int n_r, int n_dim,
                                            bool /* chi2 */, int n_params = kGradParams) {
  return ((size_t)grad_auto_rows(n_bins, n_central, n_params) + (n_params + 1) +
          grad_interp_common_rows(n_r, n_dim, n_params)) *
         kGradDraws * sizeof(double);
}
// grad_interp_cross_kernel: one slab (of the family's length: grad_interp_cross_slab), the totals
// and the weighted products (6 + n_dim, n_r) of the class in flight.
constexpr size_t grad_interp_cross_lds_bytes(int n_r, int n_dim, bool /* chi2 */,
                                             int n_params = kGradParams) {
  return ((size_t)(n_params + 1) * ((size_t)grad_interp_cross_slab(n_params) + 1) +
          (size_t)(n_params + 1 + n_dim) * n_r + grad_interp_common_rows(n_r, n_dim, n_params)) *
         kGradDraws * sizeof(double);
}

}  // namespace tc
