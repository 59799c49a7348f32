// The forward calls of the two joints -- of tables (joint.cpp) and of interpolators
// (joint_interp.cpp) -- on their way from a C entry point to their launches (host only, behind
// internal.h): what both refuse, the numbering of the mode-auto passes, the slab launch loop and
// the one entry sequence.  The kernels' argument blocks stay two structs (joint.h, joint_interp.h);
// what is written here once works on the fields they name alike.
#pragma once

namespace tc {
namespace host {

// The family a joint call's flags select: plain Zheng07, or (TC_FLAG_ASSEMBIAS) the decorated model.
inline int joint_params(unsigned flags) {
  return (flags & TC_FLAG_ASSEMBIAS) ? tc::kGradParamsAssembias : tc::kGradParams;
}

// The flags a joint forward call does not serve; `noun`: "joint forward calls", "joint
// interpolator forward calls".
inline int check_joint_forward_flags(const char* noun, unsigned flags) {
  if (flags & TC_FLAG_SEPARATE_GAL_TYPE)
    return fail(TC_ERR_UNSUPPORTED,
                "%s are implemented for the total prediction only (not separate_gal_type)", noun);
  if (flags & TC_FLAG_LEAUTHAUD11)
    return fail(TC_ERR_UNSUPPORTED, "%s are implemented for the Zheng07 family only", noun);
  const unsigned unserved =
      flags & ~(unsigned)(TC_FLAG_MODULATE_WITH_CENOCC | TC_FLAG_ASSEMBIAS);
  if (unserved != 0) return fail(TC_ERR_UNSUPPORTED, "%s: unknown flags 0x%x", noun, unserved);
  return TC_OK;
}

// Whether a mode-auto table has the unit layout of the one-launch form: its own forward layout
// of the total prediction, one r tile, one triangular component.
inline bool has_joint_forward_layout(const tc_table* t) {
  const tc::QuadLayout& layout = t->quad_total.layout;
  return t->quad && t->quad_total.d_table != nullptr && t->quad_tiling.n_rtiles == 1 &&
         layout.comps.size() == 1 && layout.comps[0].triangular;
}

// Member k of the argument block `ja` (JointForwardArgs, JointInterpForwardArgs) but for its
// matrices, the members before it done: its rows and, mode auto, its passes behind theirs, read off
// `t` (the table, an interpolator's first); the first mode-auto member gives the parts of the
// triangle and the component's place, which all of them share.
template <typename Args>
void number_joint_forward_member(Args* ja, int k, int mode, int n_rows, int r_offset,
                                 const tc_table* t) {
  const int parts = tc::joint_forward_parts(tc::kJointForwardWaves);
  ja->mode[k] = mode;
  ja->n_rows[k] = n_rows;
  ja->r_offset[k] = r_offset;
  ja->job_begin[k + 1] = ja->job_begin[k];
  if (mode != TC_MODE_AUTO) return;
  const tc::QuadComp& comp = t->quad_total.layout.comps[0];
  const int n_u = t->quad_tiling.n_u;
  ja->n_u[k] = n_u;
  ja->table_bytes[k] =
      (uint32_t)((size_t)t->quad_total.layout.n_units * (size_t)((n_u + 1) / 2) * 1024);
  ja->job_begin[k + 1] += (n_u + 1) / 2 * 2 * parts;
  // (every mode-auto member adds at least 2 * parts passes, so job_begin[k] is 0 exactly when
  // none stands before this one)
  if (ja->job_begin[k] != 0) return;
  tc::triangle_parts(comp.n_rb, parts, ja->part_rb0, ja->part_cb0, ja->part_count);
  ja->n_cb = comp.n_cb;
  ja->i_row0 = comp.i_bin0;
  ja->j_row0 = comp.j_bin0;
  ja->unit_base = (int)comp.unit_base;
}

// One launch per slab of the draws of `r` (device pointers), timed and reported through `t0`:
// launch(ja, slab, grid, k0, k1) with `ja` = `shape` and the slab's theta, draws and outputs (an
// interpolator's x: the kind's own), in a workgroup of `lds` bytes.
template <typename Args, typename Launch>
int joint_forward_slabs(tc_table* t0, const Args& shape, const double* chi2_data,
                        const PredictRequest& r, int lds, Launch launch) {
  return for_each_slab(r.n_draws, max_slab(t0), [&](int64_t begin, int64_t n) {
    const PredictRequest slab = r.chunk(begin, n);
    Args ja = shape;
    ja.theta = slab.theta;
    ja.n_draws = n;
    ja.ngal = slab.ngal;
    ja.xi = r.likelihood ? nullptr : slab.second;
    ja.chi2_data = r.likelihood ? chi2_data : nullptr;
    ja.chi2 = r.likelihood ? slab.second : nullptr;
    const dim3 grid((unsigned)((n + tc::kJointForwardDraws - 1) / tc::kJointForwardDraws));
    hipEvent_t k0 = nullptr, k1 = nullptr;
    int status = next_kernel_events(t0, &k0, &k1);
    if (status != TC_OK) return status;
    status = launch(ja, slab, grid, k0, k1);
    if (status != TC_OK) return status;
    t0->last_workgroups = (int)grid.x;
    t0->last_waves = tc::kJointForwardWaves;
    t0->last_splits = 0;
    t0->last_lds = lds;
    return TC_OK;
  });
}

// Every forward entry point of a joint: the checks, the likelihood's operands, the argument
// block, then the launches on device pointers or the forward path of host arrays (predict_call.h).
// A kind supplies, next to its base (device_id(), upload_chi2()) and to what forward_chunked and
// forward_zero_copy ask of it (table.cpp: TableForward),
//   Args, shape                           its argument block; where the entry leaves it
//   check(request)                        what it refuses, the NULL handle first
//   missing(request)                      the words of its NULL-array refusal, or NULL
//   args(request, &shape)                 the block but for the draws and the outputs
//   device(request)                       the launches on its next lane
//   plan(request)                         the chunks of a synchronous call over its lanes
//   copy_up(request, &theta, &x, &out)    the serial tail's draws on their way up, its own way
template <typename Adapter>
int joint_forward_entry(Adapter adapter, GradRoute where, const PredictRequest& request,
                        const Chi2Host* operands) {
  int status = adapter.check(request);
  if (status != TC_OK) return status;
  if (request.n_draws == 0) return TC_OK;
  const char* missing = adapter.missing(request);
  TC_CHECK(missing == nullptr, "%s", missing);
  TC_CHECK(operands == nullptr || (operands->data && operands->precision), "NULL pointer");
  TC_HIP(hipSetDevice(adapter.device_id()));
  if (operands != nullptr && (status = adapter.upload_chi2(*operands)) != TC_OK) return status;
  typename Adapter::Args shape;
  if ((status = adapter.args(request, &shape)) != TC_OK) return status;
  adapter.shape = &shape;
  if (where == GradRoute::kDevice) return adapter.device(request);
  if (zero_copy_serves(adapter, request)) return forward_zero_copy(adapter, request);
  const tc::SyncChunkPlan plan = adapter.plan(request);
  if (plan.n_chunks > 0) return forward_chunked(adapter, request, plan);
  const double *d_theta = nullptr, *d_x = nullptr;
  double* d_ngal = nullptr;
  if ((status = adapter.copy_up(request, &d_theta, &d_x, &d_ngal)) != TC_OK) return status;
  double* d_second = d_ngal + request.ngal_count();
  status = adapter.run(request.on(d_theta, d_x, d_ngal, d_second));
  if (status != TC_OK) return status;
  return copy_out(&adapter.handle()->h_out, request.ngal, request.ngal_count(), d_ngal,
                  request.second, request.second_count(), d_second, adapter.handle()->stream);
}

}  // namespace host
}  // namespace tc
