// One-launch kernels of mode cross (predict_cross_small_kernel, predict_cross_fused_kernel):
// the instances launch.hip: run_cross_fused can select, in a translation unit of their own.
#include "dispatch.h"
#include "internal.h"
#include "kernels.hip.h"

namespace tc {
namespace host {

namespace {
struct CrossLaunch {
  int device, rows;
  dim3 grid, block;
  int lds;
  hipStream_t stream;
  hipEvent_t k0, k1;
  const tc::CrossFusedArgs& ca;
};

template <bool AB, bool MO, bool DE>
int launch_cross_fused(const CrossLaunch& l) {
  // the chunk form with N rows per wave
  auto chunked = [&](auto n, auto defer) {
    const auto kernel = tc::predict_cross_fused_kernel<n(), AB, MO, defer()>;
    if (l.lds > 64 * 1024) {
      // (the kernel holds a few bytes of static LDS besides)
      const int status = ensure_lds_limit((const void*)kernel, l.device, 160 * 1024 - 256);
      if (status != TC_OK) return status;
    }
    hipExtLaunchKernelGGL(kernel, l.grid, l.block, l.lds, l.stream, l.k0, l.k1, 0, l.ca);
    return TC_OK;
  };
  constexpr std::bool_constant<DE> defer{};
  int status = TC_OK;
  switch (l.rows / tc::kCrossWaves) {      // rows per wave
    case 4: status = chunked(int_c<4>{}, defer); break;
    case 8: status = chunked(int_c<8>{}, defer); break;
    case 16: status = chunked(int_c<16>{}, std::false_type{}); break;
    case 2:     // up to 16 rows: the sums in every wave's registers
      // (the instance with the deferred pairs exists in the source and is not shipped: 16 row
      // sums next to the expansions do not fit 128 registers -- 59.2 against 58.9 us per 10^4
      // draws of the AbacusSummit table with the expansions of round 5's first half, 80 with the
      // group records; undecorated batches go through the 32-row chunk form instead:
      // choose_cross_fused)
      hipExtLaunchKernelGGL((tc::predict_cross_small_kernel<AB, MO, false>), l.grid, l.block,
                            l.lds, l.stream, l.k0, l.k1, 0, l.ca);
      break;
    default:
      return fail(TC_ERR_UNSUPPORTED, "no cross kernel for %d rows", l.rows);
  }
  if (status != TC_OK) return status;
  TC_HIP(hipGetLastError());
  return TC_OK;
}
}  // namespace

// Instances: the (assembias, modulate) square without deferred pairs, and the undecorated
// kernels with them.
int launch_cross_instance(bool assembias, bool modulate, bool defer, int device, int rows,
                          dim3 grid, dim3 block, int lds, hipStream_t stream, hipEvent_t k0,
                          hipEvent_t k1, const tc::CrossFusedArgs& ca) {
  const CrossLaunch l{device, rows, grid, block, lds, stream, k0, k1, ca};
  if (defer) return launch_cross_fused<false, false, true>(l);
  return with_bools([&](auto ab, auto mo) { return launch_cross_fused<ab(), mo(), false>(l); },
                    assembias, modulate);
}

}  // namespace host
}  // namespace tc
