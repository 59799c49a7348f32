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
