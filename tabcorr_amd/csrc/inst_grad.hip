// Gradient kernels (grad_kernels.hip.h: grad_auto_kernel, grad_cross_kernel; grad_interp_kernels.
// hip.h: grad_interp_auto_kernel, grad_interp_cross_kernel) and their launch, in a translation unit
// of their own.  Each has one form; launch.hip: run_grad and interp.cpp fill the arguments.
#include "internal.h"
#include "grad_interp_kernels.hip.h"

namespace tc {
namespace host {

int launch_grad_instance(int mode, int device, dim3 grid, int lds, hipStream_t stream,
                         hipEvent_t k0, hipEvent_t k1, const tc::GradArgs& ga) {
  const dim3 block(tc::kGradThreads);
  auto launch = [&](auto kernel) {
    if (lds > 64 * 1024) {
      const int status = ensure_lds_limit((const void*)kernel, device, lds);
      if (status != TC_OK) return status;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, k0, k1, 0, ga);
    return (int)TC_OK;
  };
  const int status = mode == TC_MODE_AUTO ? launch(tc::grad_auto_kernel)
                                          : launch(tc::grad_cross_kernel);
  if (status != TC_OK) return status;
  TC_HIP(hipGetLastError());
  return TC_OK;
}

int launch_grad_interp_instance(int mode, int device, dim3 grid, int lds, hipStream_t stream,
                                hipEvent_t k0, hipEvent_t k1, const tc::GradInterpArgs& ga) {
  const dim3 block(tc::kGradThreads);
  auto launch = [&](auto kernel) {
    if (lds > 64 * 1024) {
      const int status = ensure_lds_limit((const void*)kernel, device, lds);
      if (status != TC_OK) return status;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, k0, k1, 0, ga);
    return (int)TC_OK;
  };
  const int status = mode == TC_MODE_AUTO ? launch(tc::grad_interp_auto_kernel)
                                          : launch(tc::grad_interp_cross_kernel);
  if (status != TC_OK) return status;
  TC_HIP(hipGetLastError());
  return TC_OK;
}

}  // namespace host
}  // namespace tc
