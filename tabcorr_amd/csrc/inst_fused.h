// launch_fused<...>: one instance of predict_fused_kernel per number of r sub-tiles, and
// launch_fused_shape<W, DL>: the instances of one workgroup shape (shared by the
// inst_fused*.hip units, each of which instantiates its part of the family).
#pragma once
#include "dispatch.h"
#include "internal.h"
#include "kernels.hip.h"

namespace tc {
namespace host {

// What launch_fused_instance was called with, besides the instance.
struct FusedLaunch {
  int device, n_u;
  dim3 grid, block;
  int lds;
  hipStream_t stream;
  hipEvent_t k0, k1;
  const tc::FusedArgs& fa;
};

namespace {
template <int NG, bool AB, bool MO, bool LE = false, int W = tc::kFusedWaves, int DL = 64,
          bool GR = false, int SD = 0>
int launch_fused(const FusedLaunch& l) {
  return with_int<1, 2, 3, 4, 5>(
      l.n_u,
      [&](auto n_u) {
        const auto kernel = tc::predict_fused_kernel<NG, n_u(), AB, MO, LE, W, DL, GR, SD>;
        if (l.lds > 64 * 1024) {
          const int status = ensure_lds_limit((const void*)kernel, l.device, 160 * 1024);
          if (status != TC_OK) return status;
        }
        hipExtLaunchKernelGGL(kernel, l.grid, l.block, l.lds, l.stream, l.k0, l.k1, 0, l.fa);
        TC_HIP(hipGetLastError());
        return TC_OK;
      },
      [&] { return fail(TC_ERR_UNSUPPORTED, "no fused kernel for %d r sub-tiles", l.n_u); });
}

// The instances of W waves x DL draws (64 or 32), in the order the flags are looked at:
//   tables with groups of bins: Zheng07 with ten nodes, (assembias, modulate) square;
//   Leauthaud11: modulate or not;
//   64 draws, any number of nodes but ten: undecorated Zheng07;
//   8 x 64, undecorated, ten nodes: deferred pairs (SATDEFER 1, 2);
//   Zheng07 with ten nodes: (assembias, modulate) square.
template <int W, int DL>
int launch_fused_shape(const FusedInstance& in, const FusedLaunch& l) {
  if (!in.grouped && in.leauthaud)
    return with_bools(
        [&](auto mo) { return launch_fused<0, false, mo(), true, W, DL>(l); }, in.modulate);
  if constexpr (DL == 64) {
    if (!in.grouped && in.n_gauss != 10) return launch_fused<0, false, false, false, W, DL>(l);
  }
  if constexpr (W == 8 && DL == 64) {
    if (!in.grouped && !in.assembias && !in.modulate && (in.defer == 1 || in.defer == 2))
      return in.defer == 2 ? launch_fused<10, false, false, false, 8, 64, false, 2>(l)
                           : launch_fused<10, false, false, false, 8, 64, false, 1>(l);
  }
  return with_bools(
      [&](auto gr, auto ab, auto mo) {
        return launch_fused<10, ab(), mo(), false, W, DL, gr()>(l);
      },
      in.grouped, in.assembias, in.modulate);
}
}  // namespace

// (the parts of the family: 8 waves x 64 draws in inst_fused.hip, 8 x 32 in inst_fused32.hip,
// 16 x 64 in inst_fused16.hip, 8 x 40 -- the latency form -- in inst_fused40.hip)
int launch_fused_instance_32(const FusedInstance& in, const FusedLaunch& l);
int launch_fused_instance_40(const FusedInstance& in, const FusedLaunch& l);
int launch_fused_instance_16(const FusedInstance& in, const FusedLaunch& l);

}  // namespace host
}  // namespace tc
