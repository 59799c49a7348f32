// Occupation VJP kernels (vjp_kernels.hip.h: vjp_auto_kernel, vjp_cross_kernel) and their launch,
// in a translation unit of their own.  Each has one form; launch.hip: run_vjp fills the arguments.
#include "internal.h"
#include "vjp_kernels.hip.h"

namespace tc {
namespace host {

int launch_vjp_instance(int mode, int device, dim3 grid, int lds, hipStream_t stream,
                        hipEvent_t k0, hipEvent_t k1, const tc::VjpArgs& va) {
  const dim3 block(tc::kGradThreads);
  auto launch = [&](auto kernel) {
    if (lds > 64 * 1024) {
      const int status = ensure_lds_limit((const void*)kernel, device, lds);
      if (status != TC_OK) return status;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, k0, k1, 0, va);
    return (int)TC_OK;
  };
  const int status = mode == TC_MODE_AUTO ? launch(tc::vjp_auto_kernel)
                                          : launch(tc::vjp_cross_kernel);
  if (status != TC_OK) return status;
  TC_HIP(hipGetLastError());
  return TC_OK;
}

}  // namespace host
}  // namespace tc
