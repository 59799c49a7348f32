// Joint likelihood of several tables that share one halo table (the data vector (w_p, DeltaSigma)
// of the reference's documented likelihood step, docs/guides/overview.rst:86-92): the argument
// block of grad_joint_kernel (joint_kernels.hip.h) and its LDS budget.  Plain C++ for the
// host-only unit that fills it in (joint.cpp).
//
// The tables' result rows are concatenated in list order: table t owns the rows r_offset[t] ..
// r_offset[t] + n_r[t] of the N = sum_t n_r[t] of a draw, and `precision` is (N, N) with whatever
// blocks couple the tables.
#pragma once

#include "../../include/tabcorr_amd.h"
#include "grad.h"

namespace tc {

constexpr int kJointMaxTables = 16;

struct JointArgs {
  // What the tables share, as for one table: theta, the sizes, the quadrature constants, n_h,
  // percentile, math_table, row_tiles / k_steps and the result arrays -- with n_r := N wherever
  // n_r stands: xi (n_draws, N), dxi (n_draws, 5, N), chi2_data = data (N), then the precision
  // matrix (N, N).  grad.matrix is not read: every table has its own below.
  GradArgs grad;
  int n_tables;
  int mode[kJointMaxTables];              // TC_MODE_AUTO / TC_MODE_CROSS
  int n_r[kJointMaxTables];
  int r_offset[kJointMaxTables];
  // GradArgs::matrix of every table: the dense operand layout of grad.h in mode auto, (n_bins in
  // library order, n_r[t]) in mode cross
  const double* matrix[kJointMaxTables];
};

// LDS of grad_joint_kernel: that of grad_auto_kernel with N result rows -- the rows of w and dw,
// the totals and, for the likelihood, (6, N, kGradDraws) residuals and derivatives.  EVERY joint
// keeps the rows in LDS, also one made of mode-cross tables only (grad_cross_kernel walks the bins
// in slabs instead): a joint of cross tables with more bins than this budget admits is refused
// although each of its tables alone is served.
constexpr size_t joint_lds_bytes(int n_bins, int n_central, int n_r_total, bool chi2,
                                 int n_params = kGradParams) {
  return grad_auto_lds_bytes(n_bins, n_central, n_r_total, chi2, n_params);
}

}  // namespace tc
