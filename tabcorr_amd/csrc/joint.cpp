// Joint handle of the C ABI (include/tabcorr_amd.h): 1 .. 16 tables that share one halo table,
// evaluated for a batch of draws in ONE launch of grad_joint_kernel (joint_kernels.hip.h) -- the
// concatenated prediction with its derivatives, or chi2, its gradient and the Fisher matrix
// against the full (N, N) precision matrix.  The handle works THROUGH its tables, as an
// interpolator does: the quadrature, the lanes, the staging buffers and the kernel timer are the
// first table's, the matrices every table's own (launch.hip: build_grad_table).
// The forward entries -- the concatenated prediction or chi2 alone -- take ONE launch of
// joint_forward_kernel (joint_forward_kernels.hip.h) on the mode-auto tables' own forward unit
// layouts, and the forward call path of the tables (predict_call.h) through the first table, in the
// entry sequence the two joints share (joint_forward_call.h).
// The entries at the occupation seam -- any occupation model -- take ONE launch of vjp_joint_kernel
// (joint_vjp_kernels.hip.h) on the tables' gradient matrices, in the entry sequence and the staging
// path of the tables' own VJP entries (grad_call.h: vjp_entry) through the first table.
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

// What every call of a joint shares (grad_entry, vjp_entry, joint_forward_entry): it works
// through its first table.
struct JointHandle {
  tc_joint* joint;
  tc_table* first() const { return joint->tables[0]; }
  int device_id() const { return joint->device; }
  Chi2Operands& operands() const { return joint->chi2; }
  // (earlier kernels of any lane of the first table may still read the old operands)
  int upload_chi2(const Chi2Host& host) const {
    tc_table* t0 = first();
    return joint->chi2.upload(joint->n_r_total, host.data, host.precision, t0->stream,
                              [t0] { return tc_table_synchronize(t0); });
  }
  // The tables of a derivative kernel's argument block (JointArgs, JointVjpArgs): every table's
  // resident kernel stops and its gradient matrix is built.
  template <typename Args>
  int members(Args* ja) const {
    ja->n_tables = (int)joint->tables.size();
    for (int k = 0; k < ja->n_tables; ++k) {
      tc_table* t = joint->tables[k];
      int status = TC_OK;
      if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
      if ((status = build_grad_table(t)) != TC_OK) return status;
      ja->mode[k] = t->mode;
      ja->n_r[k] = t->n_r;
      ja->r_offset[k] = joint->r_offset[k];
      ja->matrix[k] = (const double*)t->grad.d_matrix;
    }
    return TC_OK;
  }
};

// A joint as grad_entry sees it.
struct JointGrad : JointHandle {
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
  GradStaging staging() const {
    tc_table* t0 = first();
    return {&t0->theta, nullptr, &t0->out_ngal, &t0->out_xi, t0->stream};
  }
  // One launch per slab of draws on lane 0 (pinned) or the next lane of the first table.
  int device(GradLane lane, const GradRequest& request) const {
    TC_HIP(hipSetDevice(joint->device));
    tc_table* t0 = first();
    tc::JointArgs ja{};
    fill_grad_shape(t0, request.n_gauss, request.flags, &ja.grad);
    ja.grad.n_r = joint->n_r_total;
    ja.grad.n_h = (const double*)t0->d_n_h;
    ja.grad.percentile = request.n_params == tc::kGradParamsAssembias
                             ? (const double*)t0->d_percentile
                             : nullptr;
    const int status = members(&ja);
    if (status != TC_OK) return status;
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

// ---- forward calls (joint_forward_kernels.hip.h; predict_call.h) --------------------------------

// What joint_forward_kernel does not serve, from plain numbers (tc_debug_joint_forward_fit asks
// with them too): a member that is not float64, a mode-auto member beyond one r tile, a workgroup
// beyond the LDS of a CU.  *lds_bytes: the workgroup's LDS, where the members are served.
int joint_forward_fit(int n_bins, int n_tables, const int* mode, const int* n_r, const int* dtype,
                      int64_t* lds_bytes) {
  int total = 0;
  for (int k = 0; k < n_tables; ++k) {
    if (dtype[k] != TC_DTYPE_F64)
      return fail(TC_ERR_UNSUPPORTED,
                  "joint forward calls need a float64 compute dtype: table %d has none", k);
    if (mode[k] == TC_MODE_AUTO && n_r[k] > 4 * tc::kQuadMaxU)
      return fail(TC_ERR_UNSUPPORTED,
                  "joint forward calls: table %d (mode auto) has %d correlation function bins, "
                  "more than the one r tile of %d that the one-launch form serves",
                  k, n_r[k], 4 * tc::kQuadMaxU);
    total += n_r[k];
  }
  const size_t lds = tc::joint_forward_lds_bytes(n_bins, total, tc::kJointForwardWaves);
  if (lds_bytes != nullptr) *lds_bytes = (int64_t)lds;
  if (lds > (size_t)kMaxLdsBytes)
    return fail(TC_ERR_UNSUPPORTED,
                "joint forward calls: tables of %d bins and %d correlation function bins in all "
                "need %zu bytes of LDS per workgroup, beyond the %d there are",
                n_bins, total, lds, kMaxLdsBytes);
  return TC_OK;
}

// A joint as joint_forward_entry, forward_chunked and forward_zero_copy see it (table.cpp:
// TableForward): the staging areas, the tickets, the lanes and the chunk events are the first
// table's.
struct JointForward : JointHandle {
  static constexpr bool kThreadedCopyOut = true;
  using Args = tc::JointForwardArgs;
  const Args* shape = nullptr;
  // The arguments of a forward entry point, the NULL handle first; then what the kernel refuses.
  int check(const PredictRequest& request) const {
    TC_CHECK(joint != nullptr, "joint handle is NULL");
    int status = check_joint_forward_flags("joint forward calls", request.flags);
    if (status != TC_OK) return status;
    const tc_table* t0 = first();
    status = check_predict_args(t0, request.theta, request.n_theta, request.n_draws,
                                request.n_gauss, request.flags);
    if (status != TC_OK) return status;
    const int n_tables = (int)joint->tables.size();
    int mode[tc::kJointMaxTables], n_r[tc::kJointMaxTables], dtype[tc::kJointMaxTables];
    for (int k = 0; k < n_tables; ++k) {
      mode[k] = joint->tables[k]->mode;
      n_r[k] = joint->tables[k]->n_r;
      dtype[k] = joint->tables[k]->compute_dtype;
    }
    status = joint_forward_fit(t0->n_bins, n_tables, mode, n_r, dtype, nullptr);
    if (status != TC_OK) return status;
    for (int k = 0; k < n_tables; ++k) {
      const tc_table* t = joint->tables[k];
      if (t->mode == TC_MODE_AUTO && !has_joint_forward_layout(t))
        return fail(TC_ERR_UNSUPPORTED,
                    "joint forward calls: table %d (mode auto, %d bins) does not have the unit "
                    "layout of the one-launch form", k, t->n_bins);
    }
    return TC_OK;
  }
  // The argument block but for the draws and the outputs: the resident kernels of the tables
  // stop, the mode-cross matrices are built (launch.hip: build_grad_table), the passes are numbered.
  int args(const PredictRequest& request, Args* out) const {
    tc_table* t0 = first();
    Args ja{};
    ja.n_theta = request.n_theta;
    ja.n_bins = t0->n_bins;
    ja.n_central = t0->plan.n_central;
    ja.n_gauss = request.n_gauss;
    ja.dens_rows = (t0->n_bins + 3) / 4 * 4;
    ja.n_r = joint->n_r_total;
    Quadrature* q = nullptr;
    int status = get_quadrature(t0, request.n_gauss, &q);
    if (status != TC_OK) return status;
    ja.log_m = (const double*)q->log_m;
    ja.m = (const double*)q->m;
    ja.weight = (const double*)q->weight;
    ja.n_h = (const double*)t0->d_n_h;
    ja.percentile = (const double*)t0->d_percentile;
    ja.split = 0.5;
    ja.math_table = (const double*)t0->d_math_table;
    ja.n_tables = (int)joint->tables.size();
    for (int k = 0; k < ja.n_tables; ++k) {
      tc_table* t = joint->tables[k];
      if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
      if (t->mode != TC_MODE_AUTO && (status = build_grad_table(t)) != TC_OK) return status;
      ja.matrix[k] = t->mode == TC_MODE_AUTO ? t->quad_total.d_table : t->grad.d_matrix;
      number_joint_forward_member(&ja, k, t->mode, t->n_r, joint->r_offset[k], t);
    }
    *out = ja;
    return TC_OK;
  }
  // One launch per slab of the draws of `r` (device pointers) on `stream`.
  int launches(const PredictRequest& r, hipStream_t stream) const {
    Range range("joint forward (one launch)");
    const int lds = (int)tc::joint_forward_lds_bytes(shape->n_bins, shape->n_r,
                                                     tc::kJointForwardWaves);
    return joint_forward_slabs(
        first(), *shape, joint->chi2.device(), r, lds,
        [&](const Args& ja, const PredictRequest&, dim3 grid, hipEvent_t k0, hipEvent_t k1) {
          return launch_joint_forward_instance(
              shape->n_gauss, (r.flags & TC_FLAG_ASSEMBIAS) != 0,
              (r.flags & TC_FLAG_MODULATE_WITH_CENOCC) != 0, joint->device, grid, lds, stream, k0,
              k1, ja);
        });
  }
  // (the first table's next lane, where a call of the table's may chain to it)
  int device(const PredictRequest& request) const {
    tc_table* t0 = first();
    t0->cur = next_lane(false, t0->tuning.pipeline != 0, t0->n_lanes, &t0->device_calls);
    const int status = launches(request, t0->lanes[t0->cur].stream);
    if (status == TC_OK) t0->prev = t0->cur;
    return status;
  }
  const char* missing(const PredictRequest& r) const {
    return r.ngal && r.second ? nullptr : "output pointer is NULL";
  }
  tc::SyncChunkPlan plan(const PredictRequest& request) const {
    return plan_forward_chunks(first(), first()->n_lanes, false, false, request);
  }
  // (the draws through the page-locked stage of the first table)
  int copy_up(const PredictRequest& request, const double** theta, const double**,
              double** out) const {
    tc_table* t0 = first();
    int status = t0->theta.reserve(request.theta_bytes(), t0->stream);
    if (status == TC_OK) status = t0->out_ngal.reserve(request.out_bytes(), t0->stream);
    if (status != TC_OK) return status;
    *theta = (const double*)t0->theta.ptr;
    *out = (double*)t0->out_ngal.ptr;
    return copy_in(&t0->h_in, t0->theta.ptr, request.theta, request.theta_bytes(), t0->stream);
  }

  tc_table* handle() const { return first(); }
  // (one form: a draw's result does not depend on the chunks)
  Call hints(const PredictRequest&, const tc::SyncChunkPlan&) const {
    return probe_call(handle());
  }
  std::vector<hipEvent_t>* chunk_events() const { return &handle()->chunk_events; }
  // A chunk on the first table's next lane: draws up, the launch, results down, the ticket.
  int enqueue(const PredictRequest& part, const Call&, hipEvent_t wait_for,
              hipEvent_t kernels_done, int64_t* ticket) const {
    tc_table* t0 = handle();
    tc_table::Lane& lane = t0->lanes[next_lane(false, t0->tuning.pipeline != 0, t0->n_lanes,
                                               &t0->device_calls)];
    int status = lane.in_theta.reserve(part.theta_bytes(), lane.stream);
    if (status == TC_OK) status = lane.out.reserve(part.out_bytes(), lane.stream);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(lane.in_theta.ptr, part.theta, part.theta_bytes(),
                          hipMemcpyHostToDevice, lane.stream));
    if (wait_for != nullptr) TC_HIP(hipStreamWaitEvent(lane.stream, wait_for, 0));
    double* out = (double*)lane.out.ptr;
    status = launches(
        part.on((const double*)lane.in_theta.ptr, nullptr, out, out + part.ngal_count()),
        lane.stream);
    if (status != TC_OK) return status;
    if (kernels_done != nullptr) TC_HIP(hipEventRecord(kernels_done, lane.stream));
    // (the staged results lie side by side, [ngal | second]: one copy command)
    TC_HIP(hipMemcpyAsync(part.ngal, out, part.out_bytes(), hipMemcpyDeviceToHost, lane.stream));
    return t0->tickets.issue(lane.stream, ticket);
  }
  int synchronize() const { return tc_table_synchronize(handle()); }
  // (the pinned lane of the first table)
  int run(const PredictRequest& s) const { return launches(s, handle()->stream); }
};

// The request of a joint forward entry point, in the order of the C arguments.
PredictRequest joint_forward_request(const tc_joint* joint, const double* theta, int n_theta,
                                     int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                                     double* second, bool likelihood) {
  return PredictRequest{n_theta, 0,     n_gauss, flags,  n_draws,   joint ? joint->n_r_total : 0,
                        1,       theta, nullptr, ngal,   second,    likelihood};
}

// ---- the occupation seam (joint_vjp_kernels.hip.h; grad_call.h: vjp_entry) ----------------------

int joint_rows_auto(const tc_joint* joint) {
  int rows = 0;
  for (const tc_table* t : joint->tables)
    if (t->mode == TC_MODE_AUTO) rows += t->n_r;
  return rows;
}

// A joint as vjp_entry sees it: g_xi and g_occupation go together.
struct JointVjp : JointHandle {
  // What the entries at the occupation seam refuse, the NULL handle first: flags, a negative
  // number of draws, a workgroup beyond the LDS of a CU (check_grad_fit, for all the tables
  // together).
  int check(int64_t n_draws, unsigned flags) const {
    TC_CHECK(joint != nullptr, "joint handle is NULL");
    TC_CHECK(flags == 0, "joint occupation VJP: flags must be 0, got 0x%x", flags);
    TC_CHECK(n_draws >= 0, "n_draws must be non-negative");
    const size_t lds = tc::joint_vjp_lds_bytes(first()->n_bins, joint->n_r_total,
                                               joint_rows_auto(joint));
    int status = TC_OK;
    for (size_t k = 0; status == TC_OK && k < joint->tables.size(); ++k)
      status = check_grad_fit(joint->tables[k], "joint occupation VJP", lds, joint->n_r_total);
    return status;
  }
  VjpRule rule() const {
    return {false, true,
            {"g_xi and g_occupation go together: both NULL is the forward-only form", nullptr}};
  }
  VjpStaging staging() const {
    tc_table* t0 = first();
    return {&t0->occupation, &t0->out_ngal, &t0->out_xi, t0->stream, max_slab(t0)};
  }
  // One launch per slab of draws on lane 0 (pinned) or the next lane of the first table.
  int device(GradLane lane, const VjpRequest& request) const {
    tc_table* t0 = first();
    tc::JointVjpArgs ja{};
    ja.vjp.n_bins = t0->n_bins;
    ja.vjp.n_r = joint->n_r_total;
    ja.vjp.perm = (const int32_t*)t0->d_perm;
    ja.vjp.n_h = (const double*)t0->d_n_h;
    ja.vjp.row_tiles = tc::grad_row_tiles(t0->n_bins);
    ja.vjp.k_steps = tc::grad_k_steps(t0->n_bins);
    const int status = members(&ja);
    if (status != TC_OK) return status;
    ja.n_r_auto = joint_rows_auto(joint);
    for (const tc_table* t : joint->tables) ja.n_cross += t->mode != TC_MODE_AUTO;
    return grad_slabs(t0, lane, request.n_draws,
                      [&](int64_t begin, int64_t n, hipStream_t stream) {
                        return run_vjp_joint(t0, ja, request.slab(begin, n), stream);
                      });
  }
};

// The request of such an entry, in the order of the C arguments.
VjpRequest joint_vjp_request(const tc_joint* joint, const double* occupation, int64_t n_draws,
                             const double* g_ngal, const double* g_xi, double* ngal, double* xi,
                             double* chi2, double* g_occupation) {
  return VjpRequest{n_draws, joint ? joint->tables[0]->n_bins : 0, joint ? joint->n_r_total : 0,
                    occupation, g_ngal, g_xi, nullptr, ngal, xi, chi2, g_occupation,
                    1, 0, nullptr, nullptr, nullptr};
}

}  // namespace

extern "C" {

int tc_joint_predict_occupation_vjp_batch(tc_joint* joint, const double* occupation,
                                          int64_t n_draws, unsigned flags, const double* g_ngal,
                                          const double* g_xi, double* ngal, double* xi,
                                          double* g_occupation) {
  return vjp_entry(JointVjp{joint}, GradRoute::kHost, flags,
                   joint_vjp_request(joint, occupation, n_draws, g_ngal, g_xi, ngal, xi,
                                     nullptr, g_occupation),
                   nullptr);
}

int tc_joint_predict_occupation_vjp_batch_device(tc_joint* joint, const double* occupation_device,
                                                 int64_t n_draws, unsigned flags,
                                                 const double* g_ngal_device,
                                                 const double* g_xi_device, double* ngal_device,
                                                 double* xi_device, double* g_occupation_device) {
  return vjp_entry(JointVjp{joint}, GradRoute::kDevice, flags,
                   joint_vjp_request(joint, occupation_device, n_draws, g_ngal_device,
                                     g_xi_device, ngal_device, xi_device, nullptr,
                                     g_occupation_device),
                   nullptr);
}

int tc_joint_chi2_occupation_grad_batch(tc_joint* joint, const double* occupation,
                                        int64_t n_draws, unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dchi2_docc) {
  const Chi2Host operands{data, precision};
  return vjp_entry(JointVjp{joint}, GradRoute::kHost, flags,
                   joint_vjp_request(joint, occupation, n_draws, nullptr, nullptr, ngal,
                                     nullptr, chi2, dchi2_docc),
                   &operands);
}

int tc_joint_chi2_occupation_grad_batch_device(tc_joint* joint, const double* occupation_device,
                                               int64_t n_draws, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dchi2_docc_device) {
  const Chi2Host operands{data, precision};
  return vjp_entry(JointVjp{joint}, GradRoute::kDevice, flags,
                   joint_vjp_request(joint, occupation_device, n_draws, nullptr, nullptr,
                                     ngal_device, nullptr, chi2_device, dchi2_docc_device),
                   &operands);
}

int tc_debug_joint_vjp_lds_bytes(int n_bins, int n_r_total, int n_r_auto, int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK(n_bins >= 1 && n_r_total >= 1 && n_r_auto >= 0 && n_r_auto <= n_r_total,
           "invalid shape");
  *bytes = (int64_t)tc::joint_vjp_lds_bytes(n_bins, n_r_total, n_r_auto);
  return TC_OK;
}

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

int tc_joint_predict_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                  int64_t n_draws, int n_gauss, unsigned flags,
                                  double* ngal_device, double* xi_device) {
  return joint_forward_entry(JointForward{{joint}}, GradRoute::kDevice,
                             joint_forward_request(joint, theta_device, n_theta, n_draws, n_gauss,
                                                   flags, ngal_device, xi_device, false),
                             nullptr);
}

int tc_joint_predict_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                           int n_gauss, unsigned flags, double* ngal, double* xi) {
  return joint_forward_entry(JointForward{{joint}}, GradRoute::kHost,
                             joint_forward_request(joint, theta, n_theta, n_draws, n_gauss, flags,
                                                   ngal, xi, false),
                             nullptr);
}

int tc_joint_chi2_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                               int64_t n_draws, int n_gauss, unsigned flags, const double* data,
                               const double* precision, double* ngal_device,
                               double* chi2_device) {
  const Chi2Host operands{data, precision};
  return joint_forward_entry(JointForward{{joint}}, GradRoute::kDevice,
                             joint_forward_request(joint, theta_device, n_theta, n_draws, n_gauss,
                                                   flags, ngal_device, chi2_device, true),
                             &operands);
}

int tc_joint_chi2_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                        int n_gauss, unsigned flags, const double* data, const double* precision,
                        double* ngal, double* chi2) {
  const Chi2Host operands{data, precision};
  return joint_forward_entry(JointForward{{joint}}, GradRoute::kHost,
                             joint_forward_request(joint, theta, n_theta, n_draws, n_gauss, flags,
                                                   ngal, chi2, true),
                             &operands);
}

int tc_debug_joint_forward_lds_bytes(int n_bins, int n_r_total, int waves, int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK(n_bins >= 1 && n_r_total >= 1 && waves >= 2 && waves % 2 == 0 &&
               waves <= 2 * tc::kFusedMaxParts,
           "invalid shape");
  *bytes = (int64_t)tc::joint_forward_lds_bytes(n_bins, n_r_total, waves);
  return TC_OK;
}

int tc_debug_joint_forward_fit(int n_bins, int n_tables, const int* mode, const int* n_r,
                               const int* compute_dtype, int64_t* lds_bytes) {
  TC_CHECK(mode != nullptr && n_r != nullptr && compute_dtype != nullptr, "NULL pointer");
  TC_CHECK(n_bins >= 1 && n_tables >= 1 && n_tables <= tc::kJointMaxTables, "invalid shape");
  for (int k = 0; k < n_tables; ++k)
    TC_CHECK((mode[k] == TC_MODE_AUTO || mode[k] == TC_MODE_CROSS) && n_r[k] >= 1,
             "invalid table %d", k);
  return joint_forward_fit(n_bins, n_tables, mode, n_r, compute_dtype, lds_bytes);
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
