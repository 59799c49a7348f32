// A derivative call on its way from a C entry point to its launches (host only): the request that
// every gradient entry of a table, an interpolator and a joint fills, and -- for the translation
// units that know the handles (internal.h includes this header behind them) -- the one staging
// path of the host-array entries and the one entry sequence.  The first part is plain C++ without
// the HIP runtime: tools/sanitize/host_driver.cpp and tc_debug_grad_slab evaluate it as it stands.
#pragma once

#include <cstddef>
#include <cstdint>

#include "grad.h"
#include "vjp.h"

namespace tc {
namespace host {

// The lane a derivative call asks for: lane 0, pinned (the host-array entry points stage their
// copies on it), or the next lane of the handle's rotation (the device-pointer entry points).
enum class GradLane { kPinned, kNext };

// One gradient call, or one slab of it, on device pointers.  `value` / `dvalue` are xi (n_draws,
// n_r) and dxi (n_draws, n_cols, n_r) of the prediction form, chi2 (n_draws) and dchi2 (n_draws,
// n_cols) of the likelihood form: likelihood() says which, and outputs() is the one place that
// tells the kernels.
struct GradRequest {
  int n_params;              // the family: tc::kGradParams, tc::kGradParamsAssembias (7 columns
                             // wherever 5 stand) or tc::kGradParamsLeauthaud11 (11, of 14 of theta)
  int n_extra;               // an interpolator's n_dim: columns behind the family's; else 0
  int n_gauss;
  unsigned flags;
  int64_t n_draws;
  int n_r;                   // rows of a draw's result: a table's n_r, a joint's n_r_total
  const double* theta;       // (n_draws, theta_columns())
  const double* x;           // (n_draws, n_extra), or NULL
  const double* chi2_data;   // on the device: data (n_r), then the precision matrix (n_r, n_r);
                             // NULL: the prediction form
  double* ngal;              // (n_draws)
  double* dngal;             // (n_draws, n_cols())
  double* value;
  double* dvalue;
  double* fisher;            // (n_draws, n_cols(), n_cols()), likelihood form only; NULL: not asked for

  bool likelihood() const { return chi2_data != nullptr; }
  int n_cols() const { return n_params + n_extra; }
  int theta_columns() const { return tc::grad_theta_columns(n_params); }
  // doubles per draw of `value`, and per draw and column of `dvalue`
  int64_t wide() const { return likelihood() ? 1 : n_r; }

  // The draws [begin, begin + n) of the call: every offset a 64-bit product.
  GradRequest slab(int64_t begin, int64_t n) const {
    const int64_t cols = n_cols();
    GradRequest out = *this;
    out.n_draws = n;
    out.theta = theta + begin * theta_columns();
    out.x = x ? x + begin * n_extra : nullptr;
    out.ngal = ngal + begin;
    out.dngal = dngal + begin * cols;
    out.value = value + begin * wide();
    out.dvalue = dvalue + begin * cols * wide();
    out.fisher = fisher ? fisher + begin * cols * cols : nullptr;
    return out;
  }

  // The result arrays and the likelihood's operands of the argument block.
  void outputs(tc::GradArgs* ga) const {
    ga->ngal = ngal;
    ga->dngal = dngal;
    ga->xi = likelihood() ? nullptr : value;
    ga->dxi = likelihood() ? nullptr : dvalue;
    ga->chi2_data = chi2_data;
    ga->chi2 = likelihood() ? value : nullptr;
    ga->dchi2 = likelihood() ? dvalue : nullptr;
    ga->fisher = fisher;
  }
};

// One call at the occupation seam (vjp.h), or one slab of it, of a table, of a joint or of an
// interpolator.  Which arrays are there says the form: g_occupation NULL is the forward-only form
// (a joint's, an interpolator's), and chi2_data the likelihood form, whose value is chi2 (n_draws)
// where the prediction's is xi (n_draws, n_r) with the cotangents g_xi and, or NULL = 0, g_ngal.
// An interpolator's draws carry n_classes rows of occupations and n_extra grid parameters x, and
// its adjoint forms return g_x (the likelihood form: dchi2 / dx, and dngal_dx beside it).
struct VjpRequest {
  int64_t n_draws;
  int n_bins;
  int n_r;                   // rows of a draw's result: a table's n_r, a joint's n_r_total
  const double* occupation;  // (n_draws, n_classes, n_bins)
  const double* g_ngal;      // (n_draws), or NULL
  const double* g_xi;        // (n_draws, n_r), or NULL
  const double* chi2_data;   // on the device: data (n_r), then the precision matrix (n_r, n_r)
  double* ngal;              // (n_draws)
  double* xi;                // (n_draws, n_r), or NULL
  double* chi2;              // (n_draws), or NULL
  double* g_occupation;      // (n_draws, n_classes, n_bins), or NULL
  // an interpolator's (a table and a joint: 1, 0 and NULLs)
  int n_classes;
  int n_extra;               // an interpolator's n_dim
  const double* x;           // (n_draws, n_extra), or NULL
  double* g_x;               // (n_draws, n_extra), or NULL
  double* dngal_dx;          // (n_draws, n_extra), or NULL

  bool likelihood() const { return chi2_data != nullptr; }
  // doubles of a draw's occupations
  int64_t wide() const { return (int64_t)n_classes * n_bins; }

  // The draws [begin, begin + n) of the call: every offset a 64-bit product.
  VjpRequest slab(int64_t begin, int64_t n) const {
    VjpRequest out = *this;
    out.n_draws = n;
    out.occupation = occupation + begin * wide();
    out.g_ngal = g_ngal ? g_ngal + begin : nullptr;
    out.g_xi = g_xi ? g_xi + begin * n_r : nullptr;
    out.ngal = ngal + begin;
    out.xi = xi ? xi + begin * n_r : nullptr;
    out.chi2 = chi2 ? chi2 + begin : nullptr;
    out.g_occupation = g_occupation ? g_occupation + begin * wide() : nullptr;
    out.x = x ? x + begin * n_extra : nullptr;
    out.g_x = g_x ? g_x + begin * n_extra : nullptr;
    out.dngal_dx = dngal_dx ? dngal_dx + begin * n_extra : nullptr;
    return out;
  }

  // The arrays of the argument block (x and the two x-outputs stand beside it: InterpVjpArgs).
  void arrays(tc::VjpArgs* va) const {
    va->occupation = occupation;
    va->n_draws = n_draws;
    va->g_ngal = g_ngal;
    va->g_xi = g_xi;
    va->chi2_data = chi2_data;
    va->ngal = ngal;
    va->xi = xi;
    va->chi2 = chi2;
    va->g_occupation = g_occupation;
  }
};

// Which arrays a call at the occupation seam must bring, as a handle kind states it.  The adjoint
// arrays of a request are g_xi and g_occupation (the likelihood form: g_occupation, there
// dchi2_docc, alone) and, with_x, g_x (the likelihood form: and dngal_dx).
struct VjpRule {
  bool with_x;               // an interpolator: x is required, its adjoints belong to the group
  bool forward_only;         // the adjoint arrays all NULL is a form of its own (not a table's)
  const char* together[2];   // what a mixed set is told: the prediction, the likelihood form
};

// NULL where `request` (operands: the likelihood's are there, or it is the prediction form) is
// complete under `rule`, else the words of the refusal.
inline const char* vjp_incomplete(const VjpRule& rule, const VjpRequest& request, bool likelihood,
                                  bool operands) {
  const void* value = likelihood ? (const void*)request.chi2 : request.xi;
  if (!(request.occupation && request.ngal && value && operands && (!rule.with_x || request.x)))
    return "NULL pointer";
  const void* group[4];
  int n = 0, given = 0;
  if (!likelihood) group[n++] = request.g_xi;
  group[n++] = request.g_occupation;
  if (rule.with_x) group[n++] = request.g_x;
  if (rule.with_x && likelihood) group[n++] = request.dngal_dx;
  for (int k = 0; k < n; ++k) given += group[k] != nullptr;
  if (given == n || (given == 0 && rule.forward_only)) return nullptr;
  return rule.forward_only ? rule.together[likelihood] : "NULL pointer";
}

// The element offsets that slab `begin` adds to the seven arrays of a request of this shape --
// theta, x, ngal, dngal, value, dvalue, fisher; -1: the request has no such array -- read off
// slab() itself (tc_debug_grad_slab; tools/sanitize/host_driver.cpp).
inline void grad_slab_offsets(int n_params, int n_extra, int n_r, bool likelihood, int64_t begin,
                              int64_t offsets[7]) {
  static double anchor[1];
  GradRequest whole{};
  whole.n_params = n_params;
  whole.n_extra = n_extra;
  whole.n_r = n_r;
  whole.n_draws = begin + 1;
  whole.theta = anchor;
  whole.x = n_extra > 0 ? anchor : nullptr;
  whole.chi2_data = likelihood ? anchor : nullptr;
  whole.ngal = whole.dngal = whole.value = whole.dvalue = anchor;
  whole.fisher = likelihood ? anchor : nullptr;
  const GradRequest slab = whole.slab(begin, 1);
  offsets[0] = slab.theta - whole.theta;
  offsets[1] = whole.x ? slab.x - whole.x : -1;
  offsets[2] = slab.ngal - whole.ngal;
  offsets[3] = slab.dngal - whole.dngal;
  offsets[4] = slab.value - whole.value;
  offsets[5] = slab.dvalue - whole.dvalue;
  offsets[6] = whole.fisher ? slab.fisher - whole.fisher : -1;
}

}  // namespace host
}  // namespace tc

#ifdef TC_INTERNAL_HANDLES   // (internal.h: the handles and the HIP runtime are known)

namespace tc {
namespace host {

// Where the arrays of an entry point live: device pointers (the *_device symbols, which take
// the next lane and return once the work is queued) or host arrays (staged through the handle's
// buffers on lane 0, complete when the call returns).
enum class GradRoute { kDevice, kHost };

// The likelihood's operands as an entry point receives them, on the host.
struct Chi2Host {
  const double* data;
  const double* precision;
};

// What check_grad_args refuses (TC_ERR_UNSUPPORTED with a message) or finds wrong about a request
// of `t`'s: flags, dtype, the shape of theta (`n_theta` columns as the caller states them), the
// workgroup's LDS for the prediction or the `likelihood` form.  fit = false: everything but the
// table's own fit (check_grad_fit), which a joint of tables decides for all of them together.
int check_grad_args(const tc_table* t, const GradRequest& request, int n_theta, bool likelihood,
                    bool fit);
// One launch of the family's kernel for a request of at most max_slab(t) draws on `stream`.
int run_grad(tc_table* t, const GradRequest& request, hipStream_t stream);
// The joint gradient kernel (joint_kernels.hip.h) for such a request on `stream`, timed and
// reported through the first table: `ja` complete but for what the request holds and
// grad.log_m / m / weight (the first table's quadrature of ja.grad.n_gauss nodes).
int run_grad_joint(tc_table* t0, tc::JointArgs ja, const GradRequest& request, hipStream_t stream);

// One launch of the table's occupation-seam kernel (vjp_kernels.hip.h) for a request of at most
// max_slab(t) draws on `stream`, against the gradient table.
int run_vjp(tc_table* t, const VjpRequest& request, hipStream_t stream);
// The occupation-seam kernel of a joint (joint_vjp_kernels.hip.h) for such a request on `stream`,
// timed and reported through the first table: `ja` complete but for what the request holds.
int run_vjp_joint(tc_table* t0, tc::JointVjpArgs ja, const VjpRequest& request,
                  hipStream_t stream);

// A derivative call on device pointers: run(begin, n, stream) for every slab of the batch, one
// launch each, on lane 0 (pinned) or on the next lane of the rotation (as
// tc_predict_zheng07_batch_device).
template <typename Run>
int grad_slabs(tc_table* t, GradLane request, int64_t n_draws, Run run) {
  TC_HIP(hipSetDevice(t->device));
  int status = TC_OK;
  if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  const bool pinned = request == GradLane::kPinned;
  t->cur = next_lane(pinned, t->tuning.pipeline != 0, t->n_lanes, &t->device_calls);
  hipStream_t stream = t->lanes[t->cur].stream;
  status = for_each_slab(n_draws, max_slab(t),
                         [&](int64_t begin, int64_t n) { return run(begin, n, stream); });
  if (status != TC_OK) return status;
  t->prev = pinned ? -1 : t->cur;
  return TC_OK;
}

// A call at the occupation seam on device pointers, on a stream the handle chose itself (an
// interpolator's lanes; a table's go through grad_slabs): run(slab) for every slab of at most `max`
// draws.
template <typename Run>
int vjp_slabs(const VjpRequest& request, int64_t max, Run run) {
  return for_each_slab(request.n_draws, max,
                       [&](int64_t begin, int64_t n) { return run(request.slab(begin, n)); });
}

// The buffers a host-array call at the occupation seam is staged through, the stream of its
// copies and the draws of one slab: a table's own (a joint: its first table's), an interpolator's.
struct VjpStaging {
  DeviceBuffer* in;          // occupations, cotangents, x
  DeviceBuffer* out_ngal;
  DeviceBuffer* out;         // g_occupation, the value, g_x, dngal_dx
  hipStream_t stream;
  int64_t max_slab;
};

// A call at the occupation seam on host arrays (chi2_data on the device), slab by slab: the
// occupations, the cotangents and x go up in one workspace, device(staged slab) enqueues the
// launches on the stream of the staging, and the results come down from another.
template <typename Device>
int vjp_host_arrays(const VjpStaging& stage, const VjpRequest& request, Device device) {
  const bool chi2 = request.likelihood();
  const bool cotangents = !chi2 && request.g_xi != nullptr;
  const bool backward = request.g_occupation != nullptr;
  const size_t n_r = (size_t)request.n_r, wide = (size_t)request.wide();
  const size_t n_extra = (size_t)request.n_extra;
  return for_each_slab(request.n_draws, stage.max_slab, [&](int64_t begin, int64_t n_slab) {
    const VjpRequest host = request.slab(begin, n_slab);
    const size_t n = (size_t)n_slab;
    const size_t value_count = chi2 ? n : n * n_r;
    int status = stage.in->reserve(n * (wide + n_r + 1 + n_extra) * 8, stage.stream);
    if (status == TC_OK) status = stage.out_ngal->reserve(n * 8, stage.stream);
    if (status == TC_OK)
      status = stage.out->reserve((n * wide + value_count + 2 * n * n_extra) * 8, stage.stream);
    if (status != TC_OK) return status;
    double* d_occupation = (double*)stage.in->ptr;
    double* d_g_xi = d_occupation + n * wide;
    double* d_g_ngal = d_g_xi + n * n_r;
    double* d_x = d_g_ngal + n;
    double* d_g_occupation = (double*)stage.out->ptr;
    double* d_value = d_g_occupation + n * wide;
    double* d_g_x = d_value + value_count;
    double* d_dngal_dx = d_g_x + n * n_extra;
    TC_HIP(hipMemcpyAsync(d_occupation, host.occupation, n * wide * 8, hipMemcpyHostToDevice,
                          stage.stream));
    if (cotangents)
      TC_HIP(hipMemcpyAsync(d_g_xi, host.g_xi, n * n_r * 8, hipMemcpyHostToDevice, stage.stream));
    if (cotangents && host.g_ngal != nullptr)
      TC_HIP(hipMemcpyAsync(d_g_ngal, host.g_ngal, n * 8, hipMemcpyHostToDevice, stage.stream));
    if (host.x != nullptr)
      TC_HIP(hipMemcpyAsync(d_x, host.x, n * n_extra * 8, hipMemcpyHostToDevice, stage.stream));
    VjpRequest staged = host;
    staged.occupation = d_occupation;
    staged.g_ngal = cotangents && host.g_ngal != nullptr ? d_g_ngal : nullptr;
    staged.g_xi = cotangents ? d_g_xi : nullptr;
    staged.x = host.x != nullptr ? d_x : nullptr;
    staged.ngal = (double*)stage.out_ngal->ptr;
    staged.xi = chi2 ? nullptr : d_value;
    staged.chi2 = chi2 ? d_value : nullptr;
    staged.g_occupation = backward ? d_g_occupation : nullptr;
    staged.g_x = host.g_x != nullptr ? d_g_x : nullptr;
    staged.dngal_dx = host.dngal_dx != nullptr ? d_dngal_dx : nullptr;
    status = device(staged);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(host.ngal, staged.ngal, n * 8, hipMemcpyDeviceToHost, stage.stream));
    TC_HIP(hipMemcpyAsync(chi2 ? host.chi2 : host.xi, d_value, value_count * 8,
                          hipMemcpyDeviceToHost, stage.stream));
    if (backward)
      TC_HIP(hipMemcpyAsync(host.g_occupation, d_g_occupation, n * wide * 8,
                            hipMemcpyDeviceToHost, stage.stream));
    if (host.g_x != nullptr)
      TC_HIP(hipMemcpyAsync(host.g_x, d_g_x, n * n_extra * 8, hipMemcpyDeviceToHost,
                            stage.stream));
    if (host.dngal_dx != nullptr)
      TC_HIP(hipMemcpyAsync(host.dngal_dx, d_dngal_dx, n * n_extra * 8, hipMemcpyDeviceToHost,
                            stage.stream));
    TC_HIP(hipStreamSynchronize(stage.stream));
    return (int)TC_OK;
  });
}

// The buffers of a handle that a host-array call is staged through, and the stream of its copies.
struct GradStaging {
  DeviceBuffer* theta;
  DeviceBuffer* x;           // NULL: the handle's calls have no extra parameters
  DeviceBuffer* out_ngal;    // ngal, then dngal
  DeviceBuffer* out_xi;      // value, then dvalue, then the Fisher matrix
  hipStream_t stream;
};

// A request on host arrays: the draws go up, device(staged request) enqueues the launches on the
// staging buffers, and the results come down -- ngal, dngal, value, dvalue and, where asked for,
// the Fisher matrix.
template <typename Device>
int grad_host_arrays(const GradStaging& stage, const GradRequest& request, Device device) {
  const size_t n = (size_t)request.n_draws, cols = (size_t)request.n_cols();
  const size_t value_count = n * (size_t)request.wide();
  const size_t theta_bytes = n * (size_t)request.theta_columns() * 8;
  const size_t x_bytes = n * (size_t)request.n_extra * 8;
  const size_t fisher_count = request.fisher ? n * cols * cols : 0;
  int status = stage.theta->reserve(theta_bytes, stage.stream);
  if (status == TC_OK && stage.x) status = stage.x->reserve(x_bytes, stage.stream);
  if (status == TC_OK) status = stage.out_ngal->reserve(n * (1 + cols) * 8, stage.stream);
  if (status == TC_OK)
    status = stage.out_xi->reserve((value_count * (1 + cols) + fisher_count) * 8, stage.stream);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(stage.theta->ptr, request.theta, theta_bytes, hipMemcpyHostToDevice,
                        stage.stream));
  if (stage.x)
    TC_HIP(hipMemcpyAsync(stage.x->ptr, request.x, x_bytes, hipMemcpyHostToDevice, stage.stream));
  GradRequest staged = request;
  staged.theta = (const double*)stage.theta->ptr;
  staged.x = stage.x ? (const double*)stage.x->ptr : nullptr;
  staged.ngal = (double*)stage.out_ngal->ptr;
  staged.dngal = staged.ngal + n;
  staged.value = (double*)stage.out_xi->ptr;
  staged.dvalue = staged.value + value_count;
  staged.fisher = request.fisher ? staged.dvalue + value_count * cols : nullptr;
  status = device(staged);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(request.ngal, staged.ngal, n * 8, hipMemcpyDeviceToHost, stage.stream));
  TC_HIP(hipMemcpyAsync(request.dngal, staged.dngal, n * cols * 8, hipMemcpyDeviceToHost,
                        stage.stream));
  TC_HIP(hipMemcpyAsync(request.value, staged.value, value_count * 8, hipMemcpyDeviceToHost,
                        stage.stream));
  TC_HIP(hipMemcpyAsync(request.dvalue, staged.dvalue, value_count * cols * 8,
                        hipMemcpyDeviceToHost, stage.stream));
  if (request.fisher)
    TC_HIP(hipMemcpyAsync(request.fisher, staged.fisher, fisher_count * 8, hipMemcpyDeviceToHost,
                          stage.stream));
  TC_HIP(hipStreamSynchronize(stage.stream));
  return TC_OK;
}

// Every gradient entry point of the C ABI: the request as the caller stated it (chi2_data not
// yet known) and, for the likelihood form, its operands on the host; fisher_required: the entry
// has a Fisher matrix among its outputs, which then must not be NULL.  A handle kind supplies
//   check(request, n_theta, likelihood)   what it refuses, the NULL handle first
//   null_message(likelihood)              the words of its NULL-pointer refusal
//   device_id(), operands()               its device; its operand cache
//   upload_chi2(host)                     the operands' way up, behind the wait for everything
//                                         that may still read the old values (the three in one
//                                         base per kind: its gradient, seam and forward calls)
//   staging()                             the buffers and the stream of its host-array calls
//   device(lane, request)                 the launches of a request on device pointers
template <typename Adapter>
int grad_entry(Adapter adapter, GradRoute where, GradRequest request, int n_theta,
               const Chi2Host* operands, bool fisher_required) {
  const bool likelihood = operands != nullptr;
  int status = adapter.check(request, n_theta, likelihood);
  if (status != TC_OK) return status;
  if (request.n_draws == 0) return TC_OK;
  const bool complete =
      request.ngal && request.value && request.dngal && request.dvalue &&
      (request.n_extra == 0 || request.x) &&
      (!likelihood ||
       (operands->data && operands->precision && (!fisher_required || request.fisher)));
  TC_CHECK(complete, "%s", adapter.null_message(likelihood));
  TC_HIP(hipSetDevice(adapter.device_id()));
  if (likelihood) {
    if ((status = adapter.upload_chi2(*operands)) != TC_OK) return status;
    request.chi2_data = adapter.operands().device();
  }
  if (where == GradRoute::kDevice) return adapter.device(GradLane::kNext, request);
  return grad_host_arrays(adapter.staging(), request, [&](const GradRequest& staged) {
    return adapter.device(GradLane::kPinned, staged);
  });
}

// Every entry point at the occupation seam, in grad_entry's sequence: `request` as the caller
// stated it (chi2_data not yet known) and, for the likelihood form, its operands on the host.  A
// handle kind supplies, next to its base,
//   check(n_draws, flags)                 what it refuses, the NULL handle first
//   rule()                                which arrays it needs (VjpRule)
//   staging()                             the buffers of its host-array calls (VjpStaging)
//   device(lane, request)                 everything of its own: the resident kernels stop, the
//                                         gradient tables or the walk are built, the argument block
//                                         is filled, the lane is chosen, the slabs are launched
template <typename Adapter>
int vjp_entry(Adapter adapter, GradRoute where, unsigned flags, VjpRequest request,
              const Chi2Host* operands) {
  const bool likelihood = operands != nullptr;
  int status = adapter.check(request.n_draws, flags);
  if (status != TC_OK) return status;
  if (request.n_draws == 0) return TC_OK;
  const char* missing = vjp_incomplete(adapter.rule(), request, likelihood,
                                       !likelihood || (operands->data && operands->precision));
  TC_CHECK(missing == nullptr, "%s", missing);
  TC_HIP(hipSetDevice(adapter.device_id()));
  if (likelihood) {
    if ((status = adapter.upload_chi2(*operands)) != TC_OK) return status;
    request.chi2_data = adapter.operands().device();
  }
  if (where == GradRoute::kDevice) return adapter.device(GradLane::kNext, request);
  return vjp_host_arrays(adapter.staging(), request, [&](const VjpRequest& staged) {
    return adapter.device(GradLane::kPinned, staged);
  });
}

// ---- what a joint of interpolators takes from its members (interp.cpp; joint_interp.cpp) -------
// A member as the joint reads it: the tables in list order, their grid nodes (K, n_dim), the
// axes, and the list index of the table at every position of the member's walk (class by class,
// inside a class in list order).
struct InterpParts {
  int device;
  int n_dim;
  const std::vector<tc_table*>* tables;
  const std::vector<std::vector<double>>* xp;
  const std::vector<int32_t>* table_node;
  std::vector<int32_t> walk;
};
InterpParts interp_parts(const tc_interp* it);
// The argument block of an interpolator's derivative kernels but for the draws and the outputs:
// the resident kernels of its tables stop, the walk and the classes' pointers are built.
// with_matrices = false: the walk and the classes alone -- ga->matrices stays as it is (NULL
// before the first derivative call) and no table's gradient matrix is built: what the forward
// calls of a joint ask for, which read every member's own forward layouts.
int interp_grad_args(tc_interp* it, const GradRequest& request, tc::GradInterpArgs* ga,
                     bool with_matrices = true);
GradStaging interp_grad_staging(tc_interp* it);
// The stream of the lane a derivative call takes: lane 0 (pinned) or the next of the rotation.
hipStream_t interp_grad_stream(tc_interp* it, GradLane lane);
// What the forward calls of a joint take from member 0 (predict_call.h: forward_chunked,
// forward_zero_copy): its page-locked staging areas, its tickets, the device buffers of its
// host-array calls and the stream of lane 0; n_lanes: the lanes its calls rotate over.
struct InterpForwardParts {
  PinnedBuffer* h_in;
  PinnedBuffer* h_out;
  Tickets* tickets;
  DeviceBuffer* theta;
  DeviceBuffer* x;
  DeviceBuffer* out;
  hipStream_t stream;
  int n_lanes;
};
InterpForwardParts interp_forward_parts(tc_interp* it);
// The next lane of the rotation: its stream and the staging buffers of a chunk's draws and results.
struct InterpForwardLane {
  hipStream_t stream;
  DeviceBuffer* stage_in;
  DeviceBuffer* stage_out;
};
InterpForwardLane interp_forward_lane(tc_interp* it);

}  // namespace host
}  // namespace tc

#endif  // TC_INTERNAL_HANDLES
