// Joint handle of interpolators of the C ABI (include/tabcorr_amd.h): 1 .. 16 interpolators built
// over one grid, evaluated for a batch of draws (theta, x) in ONE launch of
// grad_joint_interp_kernel (joint_interp_kernels.hip.h) -- the concatenated prediction with its
// derivatives with respect to the model's and the grid's parameters, or chi2, its gradient and the
// Fisher matrix against the full (N, N) precision matrix.  The handle works THROUGH its members:
// the grid, the walk, the classes' quadrature, the lanes, the staging buffers and the kernel timer
// are member 0's (as InterpGrad takes them, interp.cpp), the matrices every member's own tables'
// (launch.hip: build_grad_table), matched to member 0's walk by grid node.
// The forward entries -- the concatenated prediction or chi2 alone -- take ONE launch of
// joint_interp_forward_kernel (joint_interp_forward_kernels.hip.h) on the mode-auto members' own
// forward unit layouts, and the forward call path of the tables (predict_call.h) through member 0.
#include <optional>

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
  // ... of the forward kernel: a mode-auto member's unit layouts, at the first forward call
  std::vector<void*> d_forward_matrices;
  Chi2Operands chi2;                      // data (N), then the precision matrix (N, N)
};

namespace {

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

// What every call of a joint of interpolators shares (grad_entry, joint_forward_entry): it works
// through member 0.
struct JointInterpHandle {
  tc_joint_interp* joint;
  tc_interp* first() const { return joint->members[0]; }
  int device_id() const { return joint->device; }
  Chi2Operands& operands() const { return joint->chi2; }
  // (the launches go to member 0's lanes: earlier kernels there may still read the old operands)
  int upload_chi2(const Chi2Host& host) const {
    tc_interp* it = first();
    return joint->chi2.upload(joint->n_r_total, host.data, host.precision,
                              interp_grad_staging(it).stream,
                              [it] { return tc_interp_synchronize(it); });
  }
};

// A joint of interpolators as grad_entry sees it.
struct JointInterpGrad : JointInterpHandle {
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
  GradStaging staging() const { return interp_grad_staging(first()); }
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

// ---- forward calls (joint_interp_forward_kernels.hip.h; predict_call.h) -------------------------

// What joint_interp_forward_kernel does not serve, from plain numbers
// (tc_debug_joint_interp_forward_fit asks with them too): a mode-auto member beyond the
// one-launch unit layout -- one r tile, 248 bins --, a workgroup beyond the LDS of a CU.  *form: the
// joint's; *lds_bytes: the workgroup's LDS, where the members are served.
int joint_interp_forward_fit(int n_bins, int n_members, const int* mode, const int* n_r, int n_dim,
                             const int* n_axis, int* form, int64_t* lds_bytes) {
  int total = 0, weight_rows = 0;
  for (int m = 0; m < n_members; ++m) {
    if (mode[m] == TC_MODE_AUTO && n_r[m] > 4 * tc::kQuadMaxU)
      return fail(TC_ERR_UNSUPPORTED,
                  "joint interpolator forward calls: member %d (mode auto) has %d correlation "
                  "function bins, more than the one r tile of %d that the one-launch form serves",
                  m, n_r[m], 4 * tc::kQuadMaxU);
    if (mode[m] == TC_MODE_AUTO && n_bins > tc::kJointInterpForwardAutoBins)
      return fail(TC_ERR_UNSUPPORTED,
                  "joint interpolator forward calls: member %d (mode auto) has %d bins, more "
                  "than the %d whose unit layout the one-launch form serves",
                  m, n_bins, tc::kJointInterpForwardAutoBins);
    total += n_r[m];
  }
  for (int d = 0; d < n_dim; ++d) weight_rows += n_axis[d];
  const int chosen = tc::joint_interp_form(mode, n_members);
  const size_t lds = tc::joint_interp_forward_lds_bytes(chosen, n_bins, total, weight_rows,
                                                        tc::kJointForwardWaves);
  if (form != nullptr) *form = chosen;
  if (lds_bytes != nullptr) *lds_bytes = (int64_t)lds;
  if (lds > (size_t)kMaxLdsBytes)
    return fail(TC_ERR_UNSUPPORTED,
                "joint interpolator forward calls: members of %d bins and %d correlation "
                "function bins in all over a grid of %d nodes along its axes need %zu bytes of "
                "LDS per workgroup, beyond the %d there are",
                n_bins, total, weight_rows, lds, kMaxLdsBytes);
  return TC_OK;
}

// A joint of interpolators as joint_forward_entry, forward_chunked and forward_zero_copy see it
// (joint.cpp: JointForward): the staging areas, the tickets and the lanes are member 0's.
struct JointInterpForward : JointInterpHandle {
  static constexpr bool kThreadedCopyOut = true;
  using Args = tc::JointInterpForwardArgs;
  // member 0's staging areas under the names the forward path reads
  struct Staging {
    PinnedBuffer& h_in;
    PinnedBuffer& h_out;
    Tickets& tickets;
    hipStream_t stream;
  };
  const Args* shape = nullptr;
  std::optional<Staging> areas;   // (from args() on: the handle is known not to be NULL)
  // The arguments of a forward entry point, the NULL handle first; then what the kernel refuses.
  int check(const PredictRequest& request) const {
    TC_CHECK(joint != nullptr, "joint handle is NULL");
    int status = check_joint_forward_flags("joint interpolator forward calls", request.flags);
    if (status != TC_OK) return status;
    const tc_table* t0 = table_of(joint, 0);
    status = check_predict_args(t0, request.theta, request.n_theta, request.n_draws,
                                request.n_gauss, request.flags);
    if (status != TC_OK) return status;
    const InterpParts parts = interp_parts(first());
    int n_axis[tc::kGradMaxDim];
    for (int d = 0; d < joint->n_dim; ++d) n_axis[d] = (int)(*parts.xp)[d].size();
    status = joint_interp_forward_fit(t0->n_bins, (int)joint->members.size(), joint->mode.data(),
                                      joint->n_r.data(), joint->n_dim, n_axis, nullptr, nullptr);
    if (status != TC_OK) return status;
    for (size_t m = 0; m < joint->members.size(); ++m) {
      if (joint->mode[m] != TC_MODE_AUTO) continue;
      for (const tc_table* t : joint->tables[m])
        if (!has_joint_forward_layout(t))
          return fail(TC_ERR_UNSUPPORTED,
                      "joint interpolator forward calls: a table of member %d (mode auto, %d "
                      "bins) does not have the unit layout of the one-launch form",
                      (int)m, t->n_bins);
    }
    return TC_OK;
  }
  // The argument block but for the draws and the outputs: the resident kernels of every table
  // stop, member 0's walk and classes are built (interp_grad_args, without the gradient matrices:
  // only a mode-cross member's (bins, r) matrices are built here), every member's matrices are
  // matched to the walk, the passes are numbered; member 0's staging areas are taken.
  int args(const PredictRequest& request, Args* out) {
    const InterpForwardParts parts = interp_forward_parts(first());
    areas.emplace(Staging{*parts.h_in, *parts.h_out, *parts.tickets, parts.stream});
    const tc_table* t0 = table_of(joint, 0);
    GradRequest walk{};
    walk.n_params = joint_params(request.flags);
    walk.n_gauss = request.n_gauss;
    walk.flags = request.flags;
    tc::GradInterpArgs ia{};
    // (the walk and the classes alone: no table's gradient matrix is built for a forward call)
    int status = interp_grad_args(first(), walk, &ia, /*with_matrices=*/false);
    if (status != TC_OK) return status;
    Args ja{};
    ja.n_theta = request.n_theta;
    ja.n_dim = joint->n_dim;
    ja.n_bins = t0->n_bins;
    ja.n_central = t0->plan.n_central;
    ja.n_gauss = request.n_gauss;
    ja.dens_rows = (t0->n_bins + 3) / 4 * 4;
    ja.n_r = joint->n_r_total;
    ja.split = 0.5;
    ja.math_table = (const double*)t0->d_math_table;
    for (int d = 0; d < joint->n_dim; ++d) {
      ja.n_axis[d] = ia.n_axis[d];
      ja.axis_offset[d] = ia.axis_offset[d];
      ja.a_offset[d] = ia.a_offset[d];
      ja.weight_row[d] = ja.n_weight_rows;
      ja.n_weight_rows += ia.n_axis[d];
    }
    ja.xp = ia.xp;
    ja.a = ia.a;
    ja.n_classes = ia.n_classes;
    ja.class_begin = ia.class_begin;
    ja.walk_node = ia.walk_node;
    ja.class_log_m = ia.class_log_m;
    ja.class_m = ia.class_m;
    ja.class_weight = ia.class_weight;
    ja.class_n_h = ia.class_n_h;
    ja.class_percentile = ia.class_percentile;
    ja.n_members = (int)joint->members.size();
    for (int m = 0; m < ja.n_members; ++m) {
      const std::vector<tc_table*>& tables = joint->tables[m];
      const bool is_auto = joint->mode[m] == TC_MODE_AUTO;
      for (tc_table* t : tables) {
        if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
        if (!is_auto && (status = build_grad_table(t)) != TC_OK) return status;
      }
      if (joint->d_forward_matrices[m] == nullptr) {
        std::vector<void*> matrices;
        for (int32_t k : joint->order[m])
          matrices.push_back(is_auto ? tables[k]->quad_total.d_table : tables[k]->grad.d_matrix);
        if ((status = upload(matrices, &joint->d_forward_matrices[m])) != TC_OK) return status;
      }
      ja.matrices[m] = (const void* const*)joint->d_forward_matrices[m];
      number_joint_forward_member(&ja, m, joint->mode[m], joint->n_r[m], joint->r_offset[m],
                                  tables[0]);
    }
    *out = ja;
    return TC_OK;
  }
  // One launch per slab of the draws of `r` (device pointers) on `stream`.
  int launches(const PredictRequest& r, hipStream_t stream) const {
    Range range("joint interpolator forward (one launch)");
    const int lds = (int)tc::joint_interp_forward_lds_bytes(
        joint->form, shape->n_bins, shape->n_r, shape->n_weight_rows, tc::kJointForwardWaves);
    return joint_forward_slabs(
        table_of(joint, 0), *shape, joint->chi2.device(), r, lds,
        [&](Args& ja, const PredictRequest& slab, dim3 grid, hipEvent_t k0, hipEvent_t k1) {
          ja.x = slab.x;
          return launch_joint_interp_forward_instance(
              shape->n_gauss, (r.flags & TC_FLAG_ASSEMBIAS) != 0,
              (r.flags & TC_FLAG_MODULATE_WITH_CENOCC) != 0, joint->form, joint->device, grid, lds,
              stream, k0, k1, ja);
        });
  }
  // (member 0's next lane)
  int device(const PredictRequest& request) const {
    return launches(request, interp_grad_stream(first(), GradLane::kNext));
  }
  const char* missing(const PredictRequest& r) const {
    return r.x && r.ngal && r.second ? nullptr : "NULL pointer";
  }
  tc::SyncChunkPlan plan(const PredictRequest& request) const {
    return plan_forward_chunks(table_of(joint, 0), interp_forward_parts(first()).n_lanes, false,
                               false, request);
  }
  // (the draws by two copy commands into member 0's buffers)
  int copy_up(const PredictRequest& request, const double** theta, const double** x,
              double** out) const {
    const InterpForwardParts parts = interp_forward_parts(first());
    int status = parts.theta->reserve(request.theta_bytes(), parts.stream);
    if (status == TC_OK) status = parts.x->reserve(request.x_bytes(), parts.stream);
    if (status == TC_OK) status = parts.out->reserve(request.out_bytes(), parts.stream);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(parts.theta->ptr, request.theta, request.theta_bytes(),
                          hipMemcpyHostToDevice, parts.stream));
    TC_HIP(hipMemcpyAsync(parts.x->ptr, request.x, request.x_bytes(), hipMemcpyHostToDevice,
                          parts.stream));
    *theta = (const double*)parts.theta->ptr;
    *x = (const double*)parts.x->ptr;
    *out = (double*)parts.out->ptr;
    return TC_OK;
  }

  const Staging* handle() const { return &*areas; }
  // (one form: a draw's result does not depend on the chunks)
  Call hints(const PredictRequest&, const tc::SyncChunkPlan&) const { return Call(); }
  std::vector<hipEvent_t>* chunk_events() const { return nullptr; }   // (never staggered)
  // A chunk on member 0's next lane: draws up, the launch, results down, the ticket.
  int enqueue(const PredictRequest& part, const Call&, hipEvent_t, hipEvent_t,
              int64_t* ticket) const {
    const InterpForwardLane lane = interp_forward_lane(first());
    int status = lane.stage_in->reserve(part.in_bytes(), lane.stream);
    if (status == TC_OK) status = lane.stage_out->reserve(part.out_bytes(), lane.stream);
    if (status != TC_OK) return status;
    // (the staged draws lie side by side, [theta | x], and so do the results, [ngal | second]:
    // one copy command each way)
    double* in = (double*)lane.stage_in->ptr;
    double* result = (double*)lane.stage_out->ptr;
    TC_HIP(hipMemcpyAsync(in, part.theta, part.in_bytes(), hipMemcpyHostToDevice, lane.stream));
    status = launches(
        part.on(in, in + part.n_draws * part.n_theta, result, result + part.ngal_count()),
        lane.stream);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(part.ngal, result, part.out_bytes(), hipMemcpyDeviceToHost,
                          lane.stream));
    return areas->tickets.issue(lane.stream, ticket);
  }
  int synchronize() const { return tc_interp_synchronize(first()); }
  // (lane 0 of member 0)
  int run(const PredictRequest& s) const { return launches(s, areas->stream); }
};

// The request of a forward entry point, in the order of the C arguments.
PredictRequest joint_interp_forward_request(const tc_joint_interp* joint, const double* theta,
                                            int n_theta, const double* x, int64_t n_draws,
                                            int n_gauss, unsigned flags, double* ngal,
                                            double* second, bool likelihood) {
  return PredictRequest{n_theta, joint ? joint->n_dim : 0, n_gauss, flags, n_draws,
                        joint ? joint->n_r_total : 0, 1, theta, x, ngal, second, likelihood};
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
  out->d_forward_matrices.assign(n_members, nullptr);
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
  for (void* p : joint->d_forward_matrices)
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

int tc_joint_interp_predict_batch_device(tc_joint_interp* joint, const double* theta_device,
                                         int n_theta, const double* x_device, int64_t n_draws,
                                         int n_gauss, unsigned flags, double* ngal_device,
                                         double* xi_device) {
  return joint_forward_entry(
      JointInterpForward{{joint}}, GradRoute::kDevice,
      joint_interp_forward_request(joint, theta_device, n_theta, x_device, n_draws, n_gauss, flags,
                                   ngal_device, xi_device, false),
      nullptr);
}

int tc_joint_interp_predict_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                  const double* x, int64_t n_draws, int n_gauss, unsigned flags,
                                  double* ngal, double* xi) {
  return joint_forward_entry(
      JointInterpForward{{joint}}, GradRoute::kHost,
      joint_interp_forward_request(joint, theta, n_theta, x, n_draws, n_gauss, flags, ngal, xi,
                                   false),
      nullptr);
}

int tc_joint_interp_chi2_batch_device(tc_joint_interp* joint, const double* theta_device,
                                      int n_theta, const double* x_device, int64_t n_draws,
                                      int n_gauss, unsigned flags, const double* data,
                                      const double* precision, double* ngal_device,
                                      double* chi2_device) {
  const Chi2Host operands{data, precision};
  return joint_forward_entry(
      JointInterpForward{{joint}}, GradRoute::kDevice,
      joint_interp_forward_request(joint, theta_device, n_theta, x_device, n_draws, n_gauss, flags,
                                   ngal_device, chi2_device, true),
      &operands);
}

int tc_joint_interp_chi2_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                               const double* x, int64_t n_draws, int n_gauss, unsigned flags,
                               const double* data, const double* precision, double* ngal,
                               double* chi2) {
  const Chi2Host operands{data, precision};
  return joint_forward_entry(
      JointInterpForward{{joint}}, GradRoute::kHost,
      joint_interp_forward_request(joint, theta, n_theta, x, n_draws, n_gauss, flags, ngal, chi2,
                                   true),
      &operands);
}

int tc_debug_joint_interp_forward_lds_bytes(int form, int n_bins, int n_r_total,
                                            int n_weight_rows, int waves, int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK(form == tc::kJointInterpRows || form == tc::kJointInterpSlabs,
           "form must be %d (rows) or %d (slabs)", tc::kJointInterpRows, tc::kJointInterpSlabs);
  TC_CHECK(n_bins >= 1 && n_r_total >= 1 && n_weight_rows >= 4 && waves >= 2 && waves % 2 == 0 &&
               waves <= 2 * tc::kFusedMaxParts,
           "invalid shape");
  *bytes = (int64_t)tc::joint_interp_forward_lds_bytes(form, n_bins, n_r_total, n_weight_rows,
                                                       waves);
  return TC_OK;
}

int tc_debug_joint_interp_forward_fit(int n_bins, int n_members, const int* mode, const int* n_r,
                                      int n_dim, const int* n_axis, int* form,
                                      int64_t* lds_bytes) {
  TC_CHECK(mode != nullptr && n_r != nullptr && n_axis != nullptr, "NULL pointer");
  TC_CHECK(n_bins >= 1 && n_members >= 1 && n_members <= tc::kJointInterpMaxMembers &&
               n_dim >= 1 && n_dim <= tc::kGradMaxDim,
           "invalid shape");
  for (int m = 0; m < n_members; ++m)
    TC_CHECK((mode[m] == TC_MODE_AUTO || mode[m] == TC_MODE_CROSS) && n_r[m] >= 1,
             "invalid member %d", m);
  for (int d = 0; d < n_dim; ++d)
    TC_CHECK(n_axis[d] >= 4 && n_axis[d] <= tc::kGradMaxAxis, "invalid axis %d", d);
  return joint_interp_forward_fit(n_bins, n_members, mode, n_r, n_dim, n_axis, form, lds_bytes);
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
