// Joint likelihood of several INTERPOLATORS built over one grid of simulations (the reference's
// AbacusSummit database and its own suite: `wp` and `ds` interpolators read for the same model):
// the argument block of grad_joint_interp_kernel (joint_interp_kernels.hip.h), its LDS budgets
// and the matching of the members' tables by grid node.  Plain C++ for the host-only unit that
// fills it in (joint_interp.cpp) and for tools/sanitize/host_driver.cpp.
//
// The members' result rows are concatenated in list order, as in a joint of tables (joint.h):
// member m owns the rows r_offset[m] .. r_offset[m] + n_r[m] of the N = sum_m n_r[m] of a draw,
// `precision` is (N, N), and the derivatives have 5 + n_dim columns (7 + n_dim where decorated):
// the model's parameters, then the grid's.
#pragma once

#include <cstring>

#include "../../include/tabcorr_amd.h"
#include "grad.h"
#include "joint.h"

namespace tc {

constexpr int kJointInterpMaxMembers = 16;
// The two forms of the kernel, chosen from the members' modes alone.
constexpr int kJointInterpSlabs = 0;   // every member mode cross: the bins in slabs, any number
constexpr int kJointInterpRows = 1;    // a member of mode auto: every bin's rows stay in LDS

struct JointInterpArgs {
  // What the members share, as for ONE interpolator (member 0's: the draws, the grid, the walk
  // over its tables class by class, the classes' quadrature constants and n_h) -- with
  // table.n_r := N wherever n_r stands: dxi (n_draws, 5 + n_dim, N), chi2_data = data (N), then
  // the precision matrix (N, N).  interp.matrices is not read: every member has its own below.
  GradInterpArgs interp;
  int n_members;
  int n_r_cross;                                  // rows of the mode-cross members together
  int mode[kJointInterpMaxMembers];               // TC_MODE_AUTO / TC_MODE_CROSS
  int n_r[kJointInterpMaxMembers];
  int r_offset[kJointInterpMaxMembers];
  // rows form: a cross member's first row among the n_r_cross rows of the per-class products
  int cross_offset[kJointInterpMaxMembers];
  // (K) GradArgs::matrix of the member's table at the grid node of every position of MEMBER 0's
  // walk, whatever the order of the member's own list
  const double* const* matrices[kJointInterpMaxMembers];
};

inline int joint_interp_form(const int* mode, int n_members) {
  for (int m = 0; m < n_members; ++m)
    if (mode[m] == TC_MODE_AUTO) return kJointInterpRows;
  return kJointInterpSlabs;
}

// ---- LDS ------------------------------------------------------------------------------------------
// Rows form: what grad_interp_auto_kernel keeps with N result rows -- one class's rows of w and
// dw, its totals, the weights of every axis, the (6 + n_dim, N) accumulators -- and, where a
// member is mode cross, the weighted products (6 + n_dim, n_r_cross) of the class in flight.
constexpr size_t joint_interp_rows_lds_bytes(int n_bins, int n_central, int n_r_total,
                                             int n_r_cross, int n_dim,
                                             int n_params = kGradParams) {
  return grad_interp_auto_lds_bytes(n_bins, n_central, n_r_total, n_dim, false, n_params) +
         (size_t)(n_params + 1 + n_dim) * n_r_cross * kGradDraws * sizeof(double);
}
// Slab form: what grad_interp_cross_kernel keeps with N result rows.
constexpr size_t joint_interp_slabs_lds_bytes(int n_r_total, int n_dim,
                                              int n_params = kGradParams) {
  return grad_interp_cross_lds_bytes(n_r_total, n_dim, false, n_params);
}
constexpr size_t joint_interp_lds_bytes(int form, int n_bins, int n_central, int n_r_total,
                                        int n_r_cross, int n_dim, int n_params = kGradParams) {
  return form == kJointInterpRows
             ? joint_interp_rows_lds_bytes(n_bins, n_central, n_r_total, n_r_cross, n_dim,
                                           n_params)
             : joint_interp_slabs_lds_bytes(n_r_total, n_dim, n_params);
}

// ---- the forward form (joint_interp_forward_kernels.hip.h: joint_interp_forward_kernel) ----------
// (ngal, xi) or (ngal, chi2) of a batch of draws (theta, x) without any derivative, one launch
// per batch in the geometry of joint_forward_kernel (joint.h): kJointForwardDraws draws per
// workgroup of kJointForwardWaves waves.  The classes in member 0's walk order, the occupations
// of a class once for all members; a mode-auto member's table at a grid node in its own forward
// unit layout on the matrix cores, a mode-cross member's by one fma chain per (row, draw).
constexpr int kJointInterpForwardSlab = 64;   // slab form: bins whose densities one LDS slab holds
// most bins of a mode-auto member: beyond them a table has no one-launch unit layout (table.cpp)
constexpr int kJointInterpForwardAutoBins = 248;
static_assert(kJointInterpForwardSlab % kJointForwardWaves == 0,
              "a wave sums the same bins of a class in both forms: ngal has one set of bits");

struct JointInterpForwardArgs {
  const double* theta;       // (n_draws, n_theta)
  const double* x;           // (n_draws, n_dim)
  int n_theta;
  int n_dim;
  int n_bins;
  int n_central;
  int n_gauss;
  int dens_rows;             // rows form: rows of the LDS density array, whole blocks of four
  int n_r;                   // N, the concatenated rows
  int64_t n_draws;
  double split;
  const double* math_table;
  // the grid, as in GradInterpArgs; weight_row[d]: the first of axis d's n_axis[d] rows among the
  // n_weight_rows = sum_d n_axis[d] rows of spline weights in LDS
  int n_axis[kGradMaxDim];
  int axis_offset[kGradMaxDim];
  int a_offset[kGradMaxDim];
  int weight_row[kGradMaxDim];
  int n_weight_rows;
  const double* xp;
  const double* a;
  // member 0's walk and the classes' quadrature constants and n_h, as in GradInterpArgs
  int n_classes;
  const int32_t* class_begin;
  const int32_t* walk_node;
  const double* const* class_log_m;
  const double* const* class_m;
  const double* const* class_weight;
  const double* const* class_n_h;
  const double* const* class_percentile;
  double* ngal;              // (n_draws)
  double* xi;                // (n_draws, N); NULL: the likelihood form
  const double* chi2_data;   // data (N), then the precision matrix (N, N)
  double* chi2;              // (n_draws)
  int n_members;
  int mode[kJointInterpMaxMembers];
  int n_rows[kJointInterpMaxMembers];
  int r_offset[kJointInterpMaxMembers];
  // (K) per member, at every position of member 0's walk: mode auto the table's unit layout of
  // the whole triangle (QuadTable::d_table, table_bytes long, n_u sub-tiles of four r values),
  // mode cross (n_bins in library order, n_r) doubles
  const void* const* matrices[kJointInterpMaxMembers];
  uint32_t table_bytes[kJointInterpMaxMembers];
  int n_u[kJointInterpMaxMembers];
  int job_begin[kJointInterpMaxMembers + 1];   // first pass of every member (mode cross: none)
  // the parts of the triangle and the component's place, as in JointForwardArgs
  int part_rb0[kFusedMaxParts];
  int part_cb0[kFusedMaxParts];
  int part_count[kFusedMaxParts];
  int n_cb;
  int i_row0, j_row0;
  int unit_base;
};

// LDS of the rows form in bytes: the regions of joint_forward_kernel (joint.h:
// joint_forward_lds_bytes) -- the passes' per-part slabs of `sums` ARE the accumulators of the
// walk, sums[part][row][draw] += scale x F, reduced once at the end --, then the spline weights of
// the 64 draws (n_weight_rows, 64) and the class's 1 / ngal and 1 / ngal^2 (2, 64).
constexpr size_t joint_interp_forward_rows_lds_bytes(int n_bins, int n_r_total, int n_weight_rows,
                                                     int waves) {
  return joint_forward_lds_bytes(n_bins, n_r_total, waves) +
         8 * ((size_t)n_weight_rows + 2) * kLanes;
}
// ... of the slab form, in the order of the regions:
//   B  one slab of densities (kJointInterpForwardSlab, 64), later the results tile (N, 65);
//   A  the math table, later the likelihood's data and precision matrix, N (N + 1);
//   the waves' sums of the number density and of chi2, (2, waves, 64);
//   the products of the class in flight and the accumulators, (2, N, 64);
//   the spline weights (n_weight_rows, 64) and the class's 1 / ngal and 1 / ngal^2 (2, 64).
constexpr size_t joint_interp_forward_slabs_lds_bytes(int n_r_total, int n_weight_rows,
                                                      int waves) {
  const size_t n = (size_t)n_r_total;
  return 8 * (joint_forward_max((size_t)kJointInterpForwardSlab * kLanes,
                                (n * (kLanes + 1) + 1) / 2 * 2) +
              joint_forward_max((size_t)kMathTableDoubles, n * (n + 1)) +
              2 * (size_t)waves * kLanes + 2 * n * kLanes +
              ((size_t)n_weight_rows + 2) * kLanes);
}
constexpr size_t joint_interp_forward_lds_bytes(int form, int n_bins, int n_r_total,
                                                int n_weight_rows, int waves) {
  return form == kJointInterpRows
             ? joint_interp_forward_rows_lds_bytes(n_bins, n_r_total, n_weight_rows, waves)
             : joint_interp_forward_slabs_lds_bytes(n_r_total, n_weight_rows, waves);
}

// ---- the members' tables, matched by grid node ---------------------------------------------------
// walk0 (K): member 0's list index at every position of its walk; node0 and node (K, n_dim): the
// grid node of every table of member 0's and of the member's list.  out[s]: the member's list
// index of the table at the node of walk position s.  False where the member's nodes are not
// member 0's, each once.
inline bool joint_interp_permutation(int n_tables, int n_dim, const int32_t* walk0,
                                     const int32_t* node0, const int32_t* node, int32_t* out) {
  std::vector<char> taken((size_t)n_tables, 0);
  for (int s = 0; s < n_tables; ++s) {
    const int32_t* want = node0 + (size_t)walk0[s] * n_dim;
    int found = -1;
    for (int k = 0; k < n_tables && found < 0; ++k)
      if (!taken[k] && std::memcmp(want, node + (size_t)k * n_dim, sizeof(int32_t) * n_dim) == 0)
        found = k;
    if (found < 0) return false;
    taken[found] = 1;
    out[s] = found;
  }
  return true;
}

}  // namespace tc
