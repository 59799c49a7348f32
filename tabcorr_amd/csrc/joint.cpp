// Joint handle of the C ABI (include/tabcorr_amd.h): 1 .. 16 tables that share one halo table,
// evaluated for a batch of draws in ONE launch of grad_joint_kernel (joint_kernels.hip.h) -- the
// concatenated prediction with its derivatives, or chi2, its gradient and the Fisher matrix
// against the full (N, N) precision matrix.  The handle works THROUGH its tables, as an
// interpolator does: the quadrature, the lanes, the staging buffers and the kernel timer are the
// first table's, the matrices every table's own (launch.hip: build_grad_table).
#include "internal.h"

using namespace tc::host;

struct tc_joint {
  int device = 0;
  std::vector<tc_table*> tables;
  std::vector<int> r_offset;
  int n_r_total = 0;
  Chi2Operands chi2;                  // data (N), then the precision matrix (N, N)
};

namespace {

// The family a call's flags select: plain Zheng07, or (TC_FLAG_ASSEMBIAS) the decorated model.
int joint_params(unsigned flags) {
  return (flags & TC_FLAG_ASSEMBIAS) ? tc::kGradParamsAssembias : tc::kGradParams;
}

// A joint as grad_entry sees it: it works through its first table.
struct JointGrad {
  tc_joint* joint;
  // What the table entry points refuse (check_grad_args on the first table, with the family's
  // flag taken out of the flags and without the table's own fit; the tables are float64 and
  // share their bins by construction) and a joint beyond the LDS of a workgroup.
  int check(const GradRequest& request, int n_theta, bool likelihood) const {
    TC_CHECK(joint != nullptr, "joint handle is NULL");
    const tc_table* t0 = joint->tables[0];
    GradRequest unflagged = request;
    unflagged.flags &= ~(unsigned)TC_FLAG_ASSEMBIAS;
    int status = check_grad_args(t0, unflagged, n_theta, likelihood, /*fit=*/false);
    const size_t lds = tc::joint_lds_bytes(t0->n_bins, t0->plan.n_central, joint->n_r_total,
                                           likelihood, request.n_params);
    for (size_t k = 0; status == TC_OK && k < joint->tables.size(); ++k)
      status = check_grad_fit(joint->tables[k], "joint gradients", lds, joint->n_r_total);
    return status;
  }
  const char* null_message(bool likelihood) const {
    return likelihood ? "NULL pointer" : "output pointer is NULL";
  }
  int device_id() const { return joint->device; }
  Chi2Operands& operands() const { return joint->chi2; }
  // (earlier kernels of any lane of the first table may still read the old operands)
  int drain() const { return tc_table_synchronize(joint->tables[0]); }
  GradStaging staging() const {
    tc_table* t0 = joint->tables[0];
    return {&t0->theta, nullptr, &t0->out_ngal, &t0->out_xi, t0->stream};
  }
  // One launch per slab of draws on lane 0 (pinned) or the next lane of the first table; the
  // resident kernels of all the tables stop.
  int device(GradLane lane, const GradRequest& request) const {
    TC_HIP(hipSetDevice(joint->device));
    tc_table* t0 = joint->tables[0];
    tc::JointArgs ja{};
    fill_grad_shape(t0, request.n_gauss, request.flags, &ja.grad);
    ja.grad.n_r = joint->n_r_total;
    ja.grad.n_h = (const double*)t0->d_n_h;
    ja.grad.percentile = request.n_params == tc::kGradParamsAssembias
                             ? (const double*)t0->d_percentile
                             : nullptr;
    ja.n_tables = (int)joint->tables.size();
    for (int k = 0; k < ja.n_tables; ++k) {
      tc_table* t = joint->tables[k];
      int status = TC_OK;
      if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
      if ((status = build_grad_table(t)) != TC_OK) return status;
      ja.mode[k] = t->mode;
      ja.n_r[k] = t->n_r;
      ja.r_offset[k] = joint->r_offset[k];
      ja.matrix[k] = (const double*)t->grad.d_matrix;
    }
    return grad_slabs(t0, lane, request.n_draws,
                      [&](int64_t begin, int64_t n, hipStream_t stream) {
                        return run_grad_joint(t0, ja, request.slab(begin, n), stream);
                      });
  }
};

// The request of a joint entry point, in the order of the C arguments: the family by the flags.
GradRequest joint_request(const tc_joint* joint, const double* theta, int64_t n_draws, int n_gauss,
                          unsigned flags, double* ngal, double* value, double* dngal,
                          double* dvalue, double* fisher) {
  GradRequest request{};
  request.n_params = joint_params(flags);
  request.n_gauss = n_gauss;
  request.flags = flags;
  request.n_draws = n_draws;
  request.n_r = joint ? joint->n_r_total : 0;
  request.theta = theta;
  request.ngal = ngal;
  request.dngal = dngal;
  request.value = value;
  request.dvalue = dvalue;
  request.fisher = fisher;
  return request;
}

}  // namespace

extern "C" {

int tc_joint_create(tc_table* const* tables, int n_tables, tc_joint** joint) {
  TC_CHECK(joint != nullptr, "joint output pointer is NULL");
  *joint = nullptr;
  TC_CHECK(tables != nullptr, "tables is NULL");
  TC_CHECK(n_tables >= 1 && n_tables <= tc::kJointMaxTables,
           "a joint takes 1 to %d tables, got %d", tc::kJointMaxTables, n_tables);
  for (int k = 0; k < n_tables; ++k) {
    TC_CHECK(tables[k] != nullptr, "table %d is NULL", k);
    for (int l = 0; l < k; ++l)
      TC_CHECK(tables[l] != tables[k], "table %d is the same handle as table %d", k, l);
    TC_CHECK(tables[k]->device == tables[0]->device,
             "table %d is on device %d, table 0 on device %d", k, tables[k]->device,
             tables[0]->device);
    TC_CHECK(tables[k]->compute_dtype == TC_DTYPE_F64,
             "table %d does not have a float64 compute dtype", k);
    TC_CHECK(same_bins(tables[k], tables[0]),
             "table %d does not have the bins (gal_type) of table 0", k);
  }
  std::unique_ptr<tc_joint> out(new tc_joint);
  out->device = tables[0]->device;
  out->tables.assign(tables, tables + n_tables);
  for (int k = 0; k < n_tables; ++k) {
    out->r_offset.push_back(out->n_r_total);
    out->n_r_total += tables[k]->n_r;
  }
  *joint = out.release();
  return TC_OK;
}

int tc_joint_destroy(tc_joint* joint) {
  if (joint == nullptr) return TC_OK;
  // (hipFree waits for the kernels that may still read the likelihood's operands; the tables
  // are not touched: they may be gone already)
  (void)hipSetDevice(joint->device);
  joint->chi2.buffer.release();
  delete joint;
  return TC_OK;
}

int tc_joint_synchronize(tc_joint* joint) {
  TC_CHECK(joint != nullptr, "joint handle is NULL");
  return tc_table_synchronize(joint->tables[0]);
}

int tc_joint_info(const tc_joint* joint, int* n_tables, int* n_r_total, int* r_offset) {
  TC_CHECK(joint != nullptr, "joint handle is NULL");
  if (n_tables) *n_tables = (int)joint->tables.size();
  if (n_r_total) *n_r_total = joint->n_r_total;
  if (r_offset) std::copy(joint->r_offset.begin(), joint->r_offset.end(), r_offset);
  return TC_OK;
}

int tc_joint_predict_grad_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                       int64_t n_draws, int n_gauss, unsigned flags,
                                       double* ngal_device, double* xi_device,
                                       double* dngal_device, double* dxi_device) {
  return grad_entry(JointGrad{joint}, GradRoute::kDevice,
                    joint_request(joint, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  xi_device, dngal_device, dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_joint_predict_grad_batch(tc_joint* joint, const double* theta, int n_theta,
                                int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                                double* xi, double* dngal, double* dxi) {
  return grad_entry(JointGrad{joint}, GradRoute::kHost,
                    joint_request(joint, theta, n_draws, n_gauss, flags, ngal, xi, dngal, dxi,
                                  nullptr),
                    n_theta, nullptr, false);
}

int tc_joint_chi2_grad_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                    int64_t n_draws, int n_gauss, unsigned flags,
                                    const double* data, const double* precision,
                                    double* ngal_device, double* chi2_device,
                                    double* dngal_device, double* dchi2_device,
                                    double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(JointGrad{joint}, GradRoute::kDevice,
                    joint_request(joint, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  chi2_device, dngal_device, dchi2_device, fisher_device),
                    n_theta, &operands, false);
}

int tc_joint_chi2_grad_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                             int n_gauss, unsigned flags, const double* data,
                             const double* precision, double* ngal, double* chi2, double* dngal,
                             double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(JointGrad{joint}, GradRoute::kHost,
                    joint_request(joint, theta, n_draws, n_gauss, flags, ngal, chi2, dngal, dchi2,
                                  fisher),
                    n_theta, &operands, false);
}

int tc_debug_joint_lds_bytes(int n_bins, int n_central, int n_r_total, int chi2, int n_params,
                             int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK(n_bins >= 1 && n_central >= 0 && n_central <= n_bins && n_r_total >= 1,
           "invalid shape");
  TC_CHECK(n_params == tc::kGradParams || n_params == tc::kGradParamsAssembias,
           "n_params must be %d or %d", tc::kGradParams, tc::kGradParamsAssembias);
  *bytes = (int64_t)tc::joint_lds_bytes(n_bins, n_central, n_r_total, chi2 != 0, n_params);
  return TC_OK;
}

}  // extern "C"
