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
  DeviceBuffer chi2_data;             // data (N), then the precision matrix (N, N)
  std::vector<double> chi2_host;      // host copy of what chi2_data holds
};

namespace {

// Data vector and precision matrix of the joint likelihood: uploaded when they differ from the
// last upload.
int upload_chi2_data(tc_joint* joint, const double* data, const double* precision) {
  tc_table* t0 = joint->tables[0];
  const size_t n = (size_t)joint->n_r_total;
  const size_t data_count = (n + 1) * n;
  int status = joint->chi2_data.reserve(data_count * 8, t0->stream);
  if (status != TC_OK) return status;
  if (joint->chi2_host.size() != data_count ||
      memcmp(joint->chi2_host.data(), data, n * 8) != 0 ||
      memcmp(joint->chi2_host.data() + n, precision, n * n * 8) != 0) {
    // (earlier kernels of any lane may still read the old ones)
    status = tc_table_synchronize(t0);
    if (status != TC_OK) return status;
    joint->chi2_host.assign(data, data + n);
    joint->chi2_host.insert(joint->chi2_host.end(), precision, precision + n * n);
    TC_HIP(hipMemcpyAsync(joint->chi2_data.ptr, joint->chi2_host.data(), data_count * 8,
                          hipMemcpyHostToDevice, t0->stream));
    TC_HIP(hipStreamSynchronize(t0->stream));
  }
  return TC_OK;
}

// The family a call's flags select: plain Zheng07, or (TC_FLAG_ASSEMBIAS) the decorated model.
int joint_params(unsigned flags) {
  return (flags & TC_FLAG_ASSEMBIAS) ? tc::kGradParamsAssembias : tc::kGradParams;
}

// What the table entry points refuse (check_grad_args on the first table; the tables are float64
// and share their bins by construction) and a joint beyond the LDS of a workgroup.
int check_joint_args(const tc_joint* joint, const void* theta, int n_theta, int64_t n_draws,
                     int n_gauss, unsigned flags, bool chi2) {
  TC_CHECK(joint != nullptr, "joint handle is NULL");
  const int n_params = joint_params(flags);
  const tc_table* t0 = joint->tables[0];
  int status = check_grad_args(t0, theta, n_theta, n_draws, n_gauss,
                               flags & ~(unsigned)TC_FLAG_ASSEMBIAS, chi2, n_params, false);
  const size_t lds = tc::joint_lds_bytes(t0->n_bins, t0->plan.n_central, joint->n_r_total, chi2,
                                         n_params);
  for (size_t k = 0; status == TC_OK && k < joint->tables.size(); ++k)
    status = check_grad_fit(joint->tables[k], "joint gradients", lds, joint->n_r_total);
  return status;
}

// One launch per slab of draws on lane 0 (pinned) or the next lane of the first table.  xi / dxi
// NULL: chi2 / dchi2 from chi2_data and, where `fisher` is given, the Fisher matrix.
int joint_device(tc_joint* joint, GradLane request, const double* theta_device, int64_t n_draws,
                 int n_gauss, unsigned flags, double* ngal, double* xi, double* dngal,
                 double* dxi, const double* chi2_data, double* chi2, double* dchi2,
                 double* fisher) {
  TC_HIP(hipSetDevice(joint->device));
  tc_table* t0 = joint->tables[0];
  const int n_params = joint_params(flags);
  const int64_t np = n_params, n_total = joint->n_r_total;
  tc::JointArgs ja{};
  fill_grad_shape(t0, n_gauss, flags, &ja.grad);
  ja.grad.n_r = joint->n_r_total;
  ja.grad.n_h = (const double*)t0->d_n_h;
  ja.grad.percentile =
      n_params == tc::kGradParamsAssembias ? (const double*)t0->d_percentile : nullptr;
  ja.grad.chi2_data = chi2_data;
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
  return grad_slabs(t0, request, n_draws, [&](int64_t begin, int64_t n, hipStream_t stream) {
    ja.grad.theta = theta_device + begin * np;
    ja.grad.n_draws = n;
    ja.grad.ngal = ngal + begin;
    ja.grad.dngal = dngal + begin * np;
    ja.grad.xi = xi ? xi + begin * n_total : nullptr;
    ja.grad.dxi = dxi ? dxi + begin * np * n_total : nullptr;
    ja.grad.chi2 = chi2 ? chi2 + begin : nullptr;
    ja.grad.dchi2 = dchi2 ? dchi2 + begin * np : nullptr;
    ja.grad.fisher = fisher ? fisher + begin * np * np : nullptr;
    return run_grad_joint(t0, ja, n_params, stream);
  });
}

// Host arrays through the first table's staging buffers: `value` / `dvalue` are xi and dxi, or
// (chi2_data given) chi2 and dchi2.
int joint_host(tc_joint* joint, const double* theta, int64_t n_draws, int n_gauss, unsigned flags,
               const double* chi2_data, double* ngal, double* value, double* dngal,
               double* dvalue, double* fisher) {
  const bool chi2 = chi2_data != nullptr;
  const int n_params = joint_params(flags);
  return grad_host_arrays(
      joint->tables[0], theta, n_params, n_draws, n_params,
      chi2 ? (size_t)1 : (size_t)joint->n_r_total, ngal, value, dngal, dvalue, fisher,
      [&](const double* d_theta, double* d_ngal, double* d_dngal, double* d_value,
          double* d_dvalue, double* d_fisher) {
        return joint_device(joint, GradLane::kPinned, d_theta, n_draws, n_gauss, flags, d_ngal,
                            chi2 ? nullptr : d_value, d_dngal, chi2 ? nullptr : d_dvalue,
                            chi2_data, chi2 ? d_value : nullptr, chi2 ? d_dvalue : nullptr,
                            d_fisher);
      });
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
  joint->chi2_data.release();
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
  const int status =
      check_joint_args(joint, theta_device, n_theta, n_draws, n_gauss, flags, false);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(ngal_device && xi_device && dngal_device && dxi_device, "output pointer is NULL");
  return joint_device(joint, GradLane::kNext, theta_device, n_draws, n_gauss, flags, ngal_device,
                      xi_device, dngal_device, dxi_device, nullptr, nullptr, nullptr, nullptr);
}

int tc_joint_predict_grad_batch(tc_joint* joint, const double* theta, int n_theta,
                                int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                                double* xi, double* dngal, double* dxi) {
  const int status = check_joint_args(joint, theta, n_theta, n_draws, n_gauss, flags, false);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(ngal && xi && dngal && dxi, "output pointer is NULL");
  return joint_host(joint, theta, n_draws, n_gauss, flags, nullptr, ngal, xi, dngal, dxi,
                    nullptr);
}

int tc_joint_chi2_grad_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                    int64_t n_draws, int n_gauss, unsigned flags,
                                    const double* data, const double* precision,
                                    double* ngal_device, double* chi2_device,
                                    double* dngal_device, double* dchi2_device,
                                    double* fisher_device) {
  int status = check_joint_args(joint, theta_device, n_theta, n_draws, n_gauss, flags, true);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(data && precision && ngal_device && chi2_device && dngal_device && dchi2_device,
           "NULL pointer");
  TC_HIP(hipSetDevice(joint->device));
  status = upload_chi2_data(joint, data, precision);
  if (status != TC_OK) return status;
  return joint_device(joint, GradLane::kNext, theta_device, n_draws, n_gauss, flags, ngal_device,
                      nullptr, dngal_device, nullptr, (const double*)joint->chi2_data.ptr,
                      chi2_device, dchi2_device, fisher_device);
}

int tc_joint_chi2_grad_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                             int n_gauss, unsigned flags, const double* data,
                             const double* precision, double* ngal, double* chi2, double* dngal,
                             double* dchi2, double* fisher) {
  int status = check_joint_args(joint, theta, n_theta, n_draws, n_gauss, flags, true);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(data && precision && ngal && chi2 && dngal && dchi2, "NULL pointer");
  TC_HIP(hipSetDevice(joint->device));
  status = upload_chi2_data(joint, data, precision);
  if (status != TC_OK) return status;
  return joint_host(joint, theta, n_draws, n_gauss, flags, (const double*)joint->chi2_data.ptr,
                    ngal, chi2, dngal, dchi2, fisher);
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
