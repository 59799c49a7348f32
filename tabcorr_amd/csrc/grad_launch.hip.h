// The launch of one derivative kernel (inst_grad.hip, inst_vjp.hip): the LDS limit raised where
// the workgroup asks for more than 64 KiB, the extended launch with the two timing events, the
// last error.
#pragma once

#include "internal.h"

namespace tc {
namespace host {

template <typename Args>
int launch_grad_kernel(void (*kernel)(Args), int device, dim3 grid, int lds, hipStream_t stream,
                       hipEvent_t k0, hipEvent_t k1, const Args& args) {
  if (lds > 64 * 1024) {
    const int status = ensure_lds_limit((const void*)kernel, device, lds);
    if (status != TC_OK) return status;
  }
  hipExtLaunchKernelGGL(kernel, grid, dim3(tc::kGradThreads), lds, stream, k0, k1, 0, args);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

}  // namespace host
}  // namespace tc
