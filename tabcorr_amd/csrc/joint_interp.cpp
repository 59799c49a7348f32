// Joint handle of interpolators of the C ABI (include/tabcorr_amd.h): 1 .. 16 interpolators built
// over one grid, evaluated for a batch of draws (theta, x) in ONE launch of
// grad_joint_interp_kernel (joint_interp_kernels.hip.h) -- the concatenated prediction with its
// derivatives with respect to the model's and the grid's parameters, or chi2, its gradient and the
// Fisher matrix against the full (N, N) precision matrix.  The handle works THROUGH its members:
// the grid, the walk, the classes' quadrature, the lanes, the staging buffers and the kernel timer
// are member 0's (as InterpGrad takes them, interp.cpp), the matrices every member's own tables'
// (launch.hip: build_grad_table), matched to member 0's walk by grid node.
#include "internal.h"

using namespace tc::host;

struct tc_joint_interp {
  int device = 0;
  int n_dim = 0;
  int n_tables = 0;                       // of every member
  std::vector<tc_interp*> members;
  std::vector<std::vector<tc_table*>> tables;   // per member, in its list order
  std::vector<int> mode, n_r, r_offset, cross_offset;
  int n_r_total = 0;
  int n_r_cross = 0;
  int form = tc::kJointInterpSlabs;
  // per member: the list index of its table at every position of member 0's walk
  std::vector<std::vector<int32_t>> order;
  std::vector<void*> d_matrices;          // per member (K) device pointers, at the first call
  Chi2Operands chi2;                      // data (N), then the precision matrix (N, N)
};

namespace {

int joint_params(unsigned flags) {
  return (flags & TC_FLAG_ASSEMBIAS) ? tc::kGradParamsAssembias : tc::kGradParams;
}

tc_table* table_of(const tc_joint_interp* joint, int member) { return joint->tables[member][0]; }

size_t joint_lds(const tc_joint_interp* joint, int n_params) {
  const tc_table* t0 = table_of(joint, 0);
  return tc::joint_interp_lds_bytes(joint->form, t0->n_bins, t0->plan.n_central, joint->n_r_total,
                                    joint->n_r_cross, joint->n_dim, n_params);
}

// Every table's gradient operand, and per member the device array of them in walk order.
int build_matrices(tc_joint_interp* joint) {
  const int n_members = (int)joint->members.size();
  for (int m = 0; m < n_members; ++m) {
    const std::vector<tc_table*>& tables = joint->tables[m];
    for (tc_table* t : tables) {
      int status = TC_OK;
      if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
      if ((status = build_grad_table(t)) != TC_OK) return status;
    }
    if (joint->d_matrices[m] != nullptr) continue;
    std::vector<void*> matrices;
    for (int32_t k : joint->order[m]) matrices.push_back(tables[k]->grad.d_matrix);
    const int status = upload(matrices, &joint->d_matrices[m]);
    if (status != TC_OK) return status;
  }
  return TC_OK;
}

// A joint of interpolators as grad_entry sees it: it works through member 0.
struct JointInterpGrad {
  tc_joint_interp* joint;
  // What the interpolator entry points refuse (check_grad_args on member 0's first table, the
  // family's flag taken out of the flags; the tables are float64 and share their bins node by
  // node by construction) and a joint beyond the LDS of a workgroup.
  int check(const GradRequest& request, int n_theta, bool likelihood) const {
    TC_CHECK(joint != nullptr, "joint handle is NULL");
    GradRequest unflagged = request;
    unflagged.flags &= ~(unsigned)TC_FLAG_ASSEMBIAS;
    int status = check_grad_args(table_of(joint, 0), unflagged, n_theta, likelihood,
                                 /*fit=*/false);
    const size_t lds = joint_lds(joint, request.n_params);
    for (size_t m = 0; status == TC_OK && m < joint->members.size(); ++m)
      status = check_grad_fit(table_of(joint, (int)m), "joint interpolator gradients", lds,
                              joint->n_r_total);
    return status;
  }
  const char* null_message(bool) const { return "NULL pointer"; }
  int device_id() const { return joint->device; }
  Chi2Operands& operands() const { return joint->chi2; }
  // (the launches go to member 0's lanes: earlier kernels there may still read the old operands)
  int drain() const { return tc_interp_synchronize(joint->members[0]); }
  GradStaging staging() const { return interp_grad_staging(joint->members[0]); }
  // One launch per slab of draws on lane 0 (pinned) or the next lane of member 0; the resident
  // kernels of every table of every member stop.
  int device(GradLane lane, const GradRequest& request) const {
    TC_HIP(hipSetDevice(joint->device));
    tc_interp* first = joint->members[0];
    tc_table* t0 = table_of(joint, 0);
    tc::JointInterpArgs ja{};
    int status = build_matrices(joint);
    if (status == TC_OK) status = interp_grad_args(first, request, &ja.interp);
    if (status != TC_OK) return status;
    ja.interp.table.n_r = joint->n_r_total;
    ja.interp.matrices = nullptr;
    ja.n_members = (int)joint->members.size();
    ja.n_r_cross = joint->n_r_cross;
    for (int m = 0; m < ja.n_members; ++m) {
      ja.mode[m] = joint->mode[m];
      ja.n_r[m] = joint->n_r[m];
      ja.r_offset[m] = joint->r_offset[m];
      ja.cross_offset[m] = joint->cross_offset[m];
      ja.matrices[m] = (const double* const*)joint->d_matrices[m];
    }
    hipStream_t stream = interp_grad_stream(first, lane);
    const int n_params = request.n_params;
    const int lds = (int)joint_lds(joint, n_params);
    return for_each_slab(request.n_draws, max_slab(t0), [&](int64_t begin, int64_t n) {
      Range range("joint interpolator gradients (one launch)");
      const GradRequest slab = request.slab(begin, n);
      ja.interp.table.theta = slab.theta;
      ja.interp.x = slab.x;
      ja.interp.table.n_draws = n;
      slab.outputs(&ja.interp.table);
      // (timed through member 0's first table's timer)
      return launch_grad_batch(t0, n, lds, [&](dim3 grid, hipEvent_t k0, hipEvent_t k1) {
        return launch_grad_joint_interp_instance(n_params, joint->form, joint->device, grid, lds,
                                                 stream, k0, k1, ja);
      });
    });
  }
};

// The request of an entry point, in the order of the C arguments: the family by the flags, the
// n_dim extra parameters columns behind the family's.
GradRequest joint_interp_request(const tc_joint_interp* joint, const double* theta,
                                 const double* x, int64_t n_draws, int n_gauss, unsigned flags,
                                 double* ngal, double* value, double* dngal, double* dvalue,
                                 double* fisher) {
  GradRequest request{};
  request.n_params = joint_params(flags);
  request.n_extra = joint ? joint->n_dim : 0;
  request.n_gauss = n_gauss;
  request.flags = flags;
  request.n_draws = n_draws;
  request.n_r = joint ? joint->n_r_total : 0;
  request.theta = theta;
  request.x = x;
  request.ngal = ngal;
  request.dngal = dngal;
  request.value = value;
  request.dvalue = dvalue;
  request.fisher = fisher;
  return request;
}

}  // namespace

extern "C" {

int tc_joint_interp_create(tc_interp* const* members, int n_members, tc_joint_interp** joint) {
  TC_CHECK(joint != nullptr, "joint output pointer is NULL");
  *joint = nullptr;
  TC_CHECK(members != nullptr, "members is NULL");
  TC_CHECK(n_members >= 1 && n_members <= tc::kJointInterpMaxMembers,
           "a joint takes 1 to %d interpolators, got %d", tc::kJointInterpMaxMembers, n_members);
  for (int m = 0; m < n_members; ++m) {
    TC_CHECK(members[m] != nullptr, "member %d is NULL", m);
    for (int l = 0; l < m; ++l)
      TC_CHECK(members[l] != members[m], "member %d is the same handle as member %d", m, l);
  }
  std::unique_ptr<tc_joint_interp> out(new tc_joint_interp);
  const InterpParts first = interp_parts(members[0]);
  const int n_tables = (int)first.tables->size();
  out->device = first.device;
  out->n_dim = first.n_dim;
  out->n_tables = n_tables;
  out->members.assign(members, members + n_members);
  out->d_matrices.assign(n_members, nullptr);
  for (int m = 0; m < n_members; ++m) {
    const InterpParts parts = interp_parts(members[m]);
    TC_CHECK(parts.device == first.device, "member %d is on device %d, member 0 on device %d", m,
             parts.device, first.device);
    TC_CHECK(parts.n_dim == first.n_dim && (int)parts.tables->size() == n_tables,
             "member %d does not have the grid of member 0", m);
    for (int d = 0; d < first.n_dim; ++d) {
      const std::vector<double>&mine = (*parts.xp)[d], &theirs = (*first.xp)[d];
      TC_CHECK(mine.size() == theirs.size() &&
                   std::memcmp(mine.data(), theirs.data(), mine.size() * sizeof(double)) == 0,
               "member %d does not have the abscissae of member 0 in dimension %d", m, d);
    }
    std::vector<int32_t> order((size_t)n_tables);
    TC_CHECK(tc::joint_interp_permutation(n_tables, first.n_dim, first.walk.data(),
                                          first.table_node->data(), parts.table_node->data(),
                                          order.data()),
             "member %d does not have the grid nodes of member 0", m);
    const tc_table* shape = (*parts.tables)[0];
    for (int s = 0; s < n_tables; ++s) {
      const tc_table* t = (*parts.tables)[order[s]];
      TC_CHECK(t->compute_dtype == TC_DTYPE_F64,
               "member %d: table %d does not have a float64 compute dtype", m, order[s]);
      TC_CHECK(same_bins(t, (*first.tables)[first.walk[s]]),
               "member %d: table %d does not have the bins (gal_type) of member 0's table at its "
               "grid node", m, order[s]);
    }
    out->order.push_back(order);
    out->tables.push_back(*parts.tables);
    out->mode.push_back(shape->mode);
    out->n_r.push_back(shape->n_r);
    out->r_offset.push_back(out->n_r_total);
    out->cross_offset.push_back(out->n_r_cross);
    out->n_r_total += shape->n_r;
    if (shape->mode == TC_MODE_CROSS) out->n_r_cross += shape->n_r;
  }
  out->form = tc::joint_interp_form(out->mode.data(), n_members);
  *joint = out.release();
  return TC_OK;
}

int tc_joint_interp_destroy(tc_joint_interp* joint) {
  if (joint == nullptr) return TC_OK;
  // (hipFree waits for the kernels that may still read the operands and the pointer arrays; the
  // members are not touched: they may be gone already)
  (void)hipSetDevice(joint->device);
  joint->chi2.buffer.release();
  for (void* p : joint->d_matrices)
    if (p) (void)hipFree(p);
  delete joint;
  return TC_OK;
}

int tc_joint_interp_synchronize(tc_joint_interp* joint) {
  TC_CHECK(joint != nullptr, "joint handle is NULL");
  return tc_interp_synchronize(joint->members[0]);
}

int tc_joint_interp_info(const tc_joint_interp* joint, int* n_members, int* n_dim, int* n_r_total,
                         int* r_offset) {
  TC_CHECK(joint != nullptr, "joint handle is NULL");
  if (n_members) *n_members = (int)joint->members.size();
  if (n_dim) *n_dim = joint->n_dim;
  if (n_r_total) *n_r_total = joint->n_r_total;
  if (r_offset) std::copy(joint->r_offset.begin(), joint->r_offset.end(), r_offset);
  return TC_OK;
}

int tc_joint_interp_predict_grad_batch_device(tc_joint_interp* joint, const double* theta_device,
                                              int n_theta, const double* x_device,
                                              int64_t n_draws, int n_gauss, unsigned flags,
                                              double* ngal_device, double* xi_device,
                                              double* dngal_device, double* dxi_device) {
  return grad_entry(JointInterpGrad{joint}, GradRoute::kDevice,
                    joint_interp_request(joint, theta_device, x_device, n_draws, n_gauss, flags,
                                         ngal_device, xi_device, dngal_device, dxi_device,
                                         nullptr),
                    n_theta, nullptr, false);
}

int tc_joint_interp_predict_grad_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                       const double* x, int64_t n_draws, int n_gauss,
                                       unsigned flags, double* ngal, double* xi, double* dngal,
                                       double* dxi) {
  return grad_entry(JointInterpGrad{joint}, GradRoute::kHost,
                    joint_interp_request(joint, theta, x, n_draws, n_gauss, flags, ngal, xi, dngal,
                                         dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_joint_interp_chi2_grad_batch_device(tc_joint_interp* joint, const double* theta_device,
                                           int n_theta, const double* x_device, int64_t n_draws,
                                           int n_gauss, unsigned flags, const double* data,
                                           const double* precision, double* ngal_device,
                                           double* chi2_device, double* dngal_device,
                                           double* dchi2_device, double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(JointInterpGrad{joint}, GradRoute::kDevice,
                    joint_interp_request(joint, theta_device, x_device, n_draws, n_gauss, flags,
                                         ngal_device, chi2_device, dngal_device, dchi2_device,
                                         fisher_device),
                    n_theta, &operands, false);
}

int tc_joint_interp_chi2_grad_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                    const double* x, int64_t n_draws, int n_gauss,
                                    unsigned flags, const double* data, const double* precision,
                                    double* ngal, double* chi2, double* dngal, double* dchi2,
                                    double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(JointInterpGrad{joint}, GradRoute::kHost,
                    joint_interp_request(joint, theta, x, n_draws, n_gauss, flags, ngal, chi2,
                                         dngal, dchi2, fisher),
                    n_theta, &operands, false);
}

int tc_debug_joint_interp_lds_bytes(int form, int n_bins, int n_central, int n_r_total,
                                    int n_r_cross, int n_dim, int n_params, int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK(form == tc::kJointInterpRows || form == tc::kJointInterpSlabs,
           "form must be %d (rows) or %d (slabs)", tc::kJointInterpRows, tc::kJointInterpSlabs);
  TC_CHECK(n_r_total >= 1 && n_r_cross >= 0 && n_r_cross <= n_r_total && n_dim >= 1 &&
               n_dim <= tc::kGradMaxDim,
           "invalid shape");
  if (form == tc::kJointInterpRows)
    TC_CHECK(n_bins >= 1 && n_central >= 0 && n_central <= n_bins && n_r_cross < n_r_total,
             "invalid shape");
  else
    TC_CHECK(n_r_cross == n_r_total, "the slab form has mode-cross members only");
  TC_CHECK(n_params == tc::kGradParams || n_params == tc::kGradParamsAssembias,
           "n_params must be %d or %d", tc::kGradParams, tc::kGradParamsAssembias);
  *bytes = (int64_t)tc::joint_interp_lds_bytes(form, n_bins, n_central, n_r_total, n_r_cross,
                                               n_dim, n_params);
  return TC_OK;
}

}  // extern "C"
