// A forward call -- a prediction or a likelihood of a table or an interpolator: the request every
// such entry fills, the one place that knows the shapes of its arrays (plain C++ without the HIP
// runtime: tools/sanitize/host_driver.cpp evaluates it), and -- behind internal.h -- the ticket ring
// of the asynchronous calls, the chunk loop of the synchronous ones and their small-call branch.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/tabcorr_amd.h"
#include "hostmath.h"

namespace tc {
namespace host {

// One forward call, or one chunk of it.  `second` is xi (n_draws, n_comp, n_r) of a prediction,
// chi2 (n_draws) of a likelihood.
struct PredictRequest {
  int n_theta;               // columns of theta
  int n_extra;               // an interpolator's n_dim; else 0
  int n_gauss;
  unsigned flags;
  int64_t n_draws;
  int n_r;
  int n_components;          // of the table's plan: what separate_gal_type gives per draw
  const double* theta;       // (n_draws, n_theta)
  const double* x;           // (n_draws, n_extra), or NULL
  double* ngal;              // (n_draws, ngal_cols())
  double* second;            // (n_draws, second_cols())
  bool likelihood;

  bool separate() const { return (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0; }
  size_t ngal_cols() const { return separate() ? 2 : 1; }
  size_t second_cols() const {
    return likelihood ? 1 : (size_t)(separate() ? n_components : 1) * n_r;
  }
  size_t in_cols() const { return (size_t)n_theta + n_extra; }
  size_t out_cols() const { return ngal_cols() + second_cols(); }
  size_t ngal_count() const { return (size_t)n_draws * ngal_cols(); }
  size_t second_count() const { return (size_t)n_draws * second_cols(); }
  size_t theta_bytes() const { return (size_t)n_draws * n_theta * sizeof(double); }
  size_t x_bytes() const { return (size_t)n_draws * n_extra * sizeof(double); }
  size_t in_bytes() const { return theta_bytes() + x_bytes(); }
  size_t out_bytes() const { return (size_t)n_draws * out_cols() * sizeof(double); }
  // The same shape on other arrays.
  PredictRequest on(const double* theta_at, const double* x_at, double* ngal_at,
                    double* second_at) const {
    return {n_theta, n_extra, n_gauss, flags, n_draws, n_r, n_components,
            theta_at, x_at, ngal_at, second_at, likelihood};
  }
  // The draws [begin, begin + n) of the call: every offset a 64-bit product.
  PredictRequest chunk(int64_t begin, int64_t n) const {
    PredictRequest out = on(theta + begin * n_theta, x ? x + begin * n_extra : nullptr,
                            ngal + begin * (int64_t)ngal_cols(),
                            second + begin * (int64_t)second_cols());
    out.n_draws = n;
    return out;
  }
};

#ifdef TC_INTERNAL_HANDLES   // (internal.h: the HIP runtime and the staging buffers are known)

// Tickets of the asynchronous host calls (tc_*_async): a ring of events; a ticket whose slot was
// reused is older than everything now queued on the handle.
struct Tickets {
  static constexpr int kMaxTickets = 64;
  struct Slot { hipEvent_t done = nullptr; int64_t id = -1; };
  Slot ring[kMaxTickets];
  int64_t next = 0;
  // The next ticket: its event (created on first use of the slot) recorded on `stream`.
  int issue(hipStream_t stream, int64_t* id) {
    Slot& slot = ring[next % kMaxTickets];
    if (slot.done == nullptr)
      TC_HIP(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    *id = slot.id = next++;
    TC_HIP(hipEventRecord(slot.done, stream));
    return TC_OK;
  }
  // Blocks until the ticket is done; synchronize_all(): the handle's wait for everything queued,
  // which a ticket whose slot was reused is older than.
  template <typename SynchronizeAll>
  int wait(int64_t id, SynchronizeAll synchronize_all) const {
    TC_CHECK(id >= 0 && id < next, "unknown ticket %lld", (long long)id);
    const Slot& slot = ring[id % kMaxTickets];
    if (slot.id != id) return synchronize_all();
    TC_HIP(hipEventSynchronize(slot.done));
    return TC_OK;
  }
  // Whether the ticket is done; one whose slot was reused: once every lane's stream (NULL: a lane
  // without one) has passed its later work.  what[2]: the handle kind's names of the two queries.
  template <typename Lane, int n_lanes>
  int query(int64_t id, int* done, const Lane (&lanes)[n_lanes], const char* const what[2]) const {
    TC_CHECK(id >= 0 && id < next, "unknown ticket %lld", (long long)id);
    const Slot& slot = ring[id % kMaxTickets];
    const bool reused = slot.id != id;
    hipError_t state = reused ? hipSuccess : hipEventQuery(slot.done);
    for (int k = 0; reused && k < n_lanes; ++k) {
      if (lanes[k].stream == nullptr) continue;
      const hipError_t lane_state = hipStreamQuery(lanes[k].stream);
      if (state == hipSuccess || state == hipErrorNotReady)
        state = lane_state == hipSuccess ? state : lane_state;
    }
    *done = state == hipSuccess ? 1 : 0;
    if (state != hipSuccess && state != hipErrorNotReady)
      return fail(TC_ERR_HIP, "%s failed: %s", what[reused], hipGetErrorString(state));
    return TC_OK;
  }
  void release() {
    for (Slot& slot : ring)
      if (slot.done != nullptr) (void)hipEventDestroy(slot.done);
  }
};

// A synchronous host-array call as the chunks of `plan` (hostmath.h: plan_sync_chunks): chunk k is
// staged and queued through the handle's asynchronous path while chunk k - 1 computes; its results
// are copied to the caller's arrays (parallel_copy) while later chunks compute and travel.  In a
// staggered plan chunk k's kernels wait for chunk k - 1's.  What a handle kind supplies: see
// table.cpp, TableForward.

// The draws [begin, begin + n) of `request` in the handle's staging areas: a chunk's draws side by
// side, [theta | x], and its results too, [ngal | second] -- one copy command.
template <typename Adapter>
PredictRequest staged(Adapter adapter, const PredictRequest& request, int64_t begin, int64_t n) {
  double* in = (double*)adapter.handle()->h_in.ptr + begin * (int64_t)request.in_cols();
  double* out = (double*)adapter.handle()->h_out.ptr + begin * (int64_t)request.out_cols();
  return request.chunk(begin, n).on(in, request.x ? in + n * request.n_theta : nullptr, out,
                                    out + n * (int64_t)request.ngal_cols());
}
template <typename Adapter>
int forward_chunked(Adapter adapter, const PredictRequest& request, const SyncChunkPlan& plan) {
  int status = adapter.handle()->h_in.reserve(request.in_bytes());
  if (status == TC_OK) status = adapter.handle()->h_out.reserve(request.out_bytes());
  if (status != TC_OK) return status;
  std::vector<hipEvent_t>* events = plan.staggered ? adapter.chunk_events() : nullptr;
  while (events != nullptr && (int)events->size() < plan.n_chunks) {
    hipEvent_t event;
    TC_HIP(hipEventCreateWithFlags(&event, hipEventDisableTiming));
    events->push_back(event);
  }
  auto hints = adapter.hints(request, plan);
  hints.cross_target = 512 / plan.n_chunks;   // (ALL chunks' workgroups fill the chip once)
  int64_t tickets[64];
  int n_chunks = plan.n_chunks;
  for (int k = 0; k < n_chunks && status == TC_OK; ++k) {
    const int64_t begin = plan.begins[k], n = plan.begins[k + 1] - begin;
    const PredictRequest from = request.chunk(begin, n), part = staged(adapter, request, begin, n);
    memcpy((void*)part.theta, from.theta, from.theta_bytes());
    if (from.x) memcpy((void*)part.x, from.x, from.x_bytes());
    status = adapter.enqueue(part, hints, events && k > 0 ? (*events)[k - 1] : nullptr,
                             events ? (*events)[k] : nullptr, &tickets[k]);
    if (status != TC_OK) n_chunks = k;       // (wait for what was queued, then report)
  }
  for (int k = 0; k < n_chunks; ++k) {
    const int64_t begin = plan.begins[k], n = plan.begins[k + 1] - begin;
    const int waited =
        adapter.handle()->tickets.wait(tickets[k], [&] { return adapter.synchronize(); });
    if (waited != TC_OK) {
      (void)adapter.synchronize();
      return waited;
    }
    if (status != TC_OK) continue;
    const PredictRequest to = request.chunk(begin, n), part = staged(adapter, request, begin, n);
    memcpy(to.ngal, part.ngal, part.ngal_count() * 8);
    parallel_copy(to.second, part.second, part.second_count() * 8);
  }
  return status;
}

// Small and medium calls: no copy commands at all.  The kernels read the draws from and write the
// results to page-locked host memory, which the device addresses directly; two API calls and two
// copy-engine round trips less (a table's 1 draw 45 -> 40 us, 1000 draws 72 -> 54 us; beyond ~1 MB
// the copy engines win).  For calls of at most zero_copy_limit() bytes, the staging areas given:
template <typename Adapter>
bool zero_copy_serves(Adapter adapter, const PredictRequest& request) {
  return request.in_bytes() + request.out_bytes() <= zero_copy_limit() &&
         adapter.handle()->h_in.reserve(request.in_bytes()) == TC_OK &&
         adapter.handle()->h_out.reserve(request.out_bytes()) == TC_OK;
}
template <typename Adapter>
int forward_zero_copy(Adapter adapter, const PredictRequest& request) {
  const PredictRequest part = staged(adapter, request, 0, request.n_draws);
  memcpy((void*)part.theta, request.theta, request.theta_bytes());
  if (request.x) memcpy((void*)part.x, request.x, request.x_bytes());
  const int status = adapter.run(part);
  if (status != TC_OK) return status;
  TC_HIP(hipStreamSynchronize(adapter.handle()->stream));
  memcpy(request.ngal, part.ngal, request.ngal_count() * 8);
  // (a table's second array on the copy threads from 256 KB on, an interpolator's by one memcpy)
  const size_t bytes = request.second_count() * 8;
  if (Adapter::kThreadedCopyOut) parallel_copy(request.second, part.second, bytes);
  else memcpy(request.second, part.second, bytes);
  return TC_OK;
}

#endif  // TC_INTERNAL_HANDLES

}  // namespace host
}  // namespace tc
