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
#include "vjp.h"

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

// ---- the occupation seam (joint_vjp_kernels.hip.h: vjp_joint_kernel) ----------------------------
// predict(occupation) of every table, its vector-Jacobian product with respect to the occupation
// array, and chi2 of the concatenated data vector with or without its gradient -- for ANY
// occupation model.  The formulas are those of vjp.h, summed over the tables:
//   g_n,i = n_h,i [ g_ngal + (2 / ngal^2) sum_auto g_r U_ri + (1 / ngal) sum_cross g_r T_ri
//                   - (2 / ngal) sum_auto g_r xi_r - (1 / ngal) sum_cross g_r xi_r ]
struct JointVjpArgs {
  // What the tables share, as for one table, with n_r := N wherever n_r stands: g_xi and xi
  // (n_draws, N), chi2_data = data (N), then the precision matrix (N, N).  vjp.matrix is not
  // read: every table has its own below.  vjp.g_occupation NULL: the forward-only form, which
  // writes (ngal, xi) or (ngal, chi2); otherwise vjp.g_xi NULL is the likelihood form.
  VjpArgs vjp;
  int n_tables;
  int mode[kJointMaxTables];              // TC_MODE_AUTO / TC_MODE_CROSS
  int n_r[kJointMaxTables];
  int r_offset[kJointMaxTables];
  int n_r_auto;                           // rows of the mode-auto tables in all
  int n_cross;                            // mode-cross tables
  // VjpArgs::matrix of every table
  const double* matrix[kJointMaxTables];
};

// LDS of vjp_joint_kernel in rows of kGradDraws doubles: w of every bin, one row of zeros and the
// auto tables' sum_r g_r U_ri of every bin; one partial q_r per wave and auto row, later (P e) of
// all N rows; the cotangent and xi of all N rows; ngal and the two sums of g_r xi_r.  EVERY joint
// keeps the bins in LDS, as grad_joint_kernel does.
constexpr int joint_vjp_rows(int n_bins, int n_r_total, int n_r_auto) {
  return 2 * n_bins + 1 +
         (kGradWaves * n_r_auto > n_r_total ? kGradWaves * n_r_auto : n_r_total) +
         2 * n_r_total + 3;
}
constexpr size_t joint_vjp_lds_bytes(int n_bins, int n_r_total, int n_r_auto) {
  return (size_t)joint_vjp_rows(n_bins, n_r_total, n_r_auto) * kGradDraws * sizeof(double);
}

// ---- the forward form (joint_forward_kernels.hip.h: joint_forward_kernel) -----------------------
// One launch per batch, kJointForwardDraws draws per workgroup of kJointForwardWaves waves: the
// occupations once, every mode-auto table's packed triangle (the table's own forward unit layout)
// on the matrix cores, every mode-cross table by one fma chain per row, then the concatenated
// prediction or chi2 against the (N, N) precision matrix.
constexpr int kJointForwardWaves = 8;
constexpr int kJointForwardDraws = kLanes;      // two tiles of kQuadTile draws
// Parts a mode-auto table's triangle is cut into per tile of 32 draws: with the two tiles and the
// pairs of r sub-tiles, (n_u + 1) / 2 * 2 * parts passes per table are dealt to the waves.
constexpr int joint_forward_parts(int waves) { return waves / 2; }

struct JointForwardArgs {
  const double* theta;       // (n_draws, n_theta)
  int n_theta;
  int n_bins;
  int n_central;
  int n_gauss;
  int dens_rows;             // rows of the LDS density array: whole blocks of four
  int n_r;                   // N, the concatenated rows
  int64_t n_draws;
  const double* log_m;       // quadrature constants as in FusedArgs
  const double* m;
  const double* weight;
  const double* n_h;
  const double* percentile;
  double split;
  const double* math_table;
  double* ngal;              // (n_draws)
  double* xi;                // (n_draws, N); NULL: the likelihood form
  const double* chi2_data;   // data (N), then the precision matrix (N, N)
  double* chi2;              // (n_draws)
  int n_tables;
  int mode[kJointMaxTables];
  int n_rows[kJointMaxTables];            // a table's n_r
  int r_offset[kJointMaxTables];
  // mode auto: the table's unit layout of the whole triangle (QuadTable::d_table), n_u sub-tiles
  // of four r values, table_bytes long; mode cross: (n_bins in library order, n_r) doubles
  const void* matrix[kJointMaxTables];
  uint32_t table_bytes[kJointMaxTables];
  int n_u[kJointMaxTables];
  int job_begin[kJointMaxTables + 1];     // first pass of every table (mode cross: none)
  // the parts of the triangle (hostmath.h: triangle_parts; the tables share their bins, so also
  // the triangle) and the component's place in the densities and in the unit numbering
  int part_rb0[kFusedMaxParts];
  int part_cb0[kFusedMaxParts];
  int part_count[kFusedMaxParts];
  int n_cb;
  int i_row0, j_row0;
  int unit_base;
};

constexpr size_t joint_forward_max(size_t a, size_t b) { return a > b ? a : b; }

// LDS of joint_forward_kernel in bytes, for tables of n_bins bins, N = n_r_total rows and `waves`
// waves per workgroup, in the order of the regions:
//   B  the densities (rows in whole blocks of four, 64), later the results tile (N, 65);
//   A  the math table, later the likelihood's data and precision matrix, N (N + 1);
//   the waves' sums of the number density and of chi2, (2, waves, 64);
//   the passes' sums, (parts, N, 64): a mode-cross row takes part 0 only.
constexpr size_t joint_forward_lds_bytes(int n_bins, int n_r_total, int waves) {
  const size_t n = (size_t)n_r_total;
  const size_t dens_rows = ((size_t)n_bins + 3) / 4 * 4;
  // (region B in whole 16-byte words: the math table behind it is read by such)
  return 8 * (joint_forward_max(dens_rows * kLanes, (n * (kLanes + 1) + 1) / 2 * 2) +
              joint_forward_max((size_t)kMathTableDoubles, n * (n + 1)) +
              2 * (size_t)waves * kLanes +
              (size_t)joint_forward_parts(waves) * n * kLanes);
}

}  // namespace tc
