// Gradient kernels of the Zheng07 model decorated with assembly bias: the seven-parameter
// instances of grad_kernels.hip.h and grad_interp_kernels.hip.h (inst_grad.hip: the plain ones)
// and their launch, in a translation unit of their own so that the two sets compile side by side.
#include "grad_interp_kernels.hip.h"
#include "grad_launch.hip.h"

namespace tc {
namespace host {

template <>
int launch_grad_family<tc::kGradParamsAssembias, tc::GradArgs>(int mode, int device, dim3 grid,
                                                               int lds, hipStream_t stream,
                                                               hipEvent_t k0, hipEvent_t k1,
                                                               const tc::GradArgs& ga) {
  return launch_grad_kernel(mode == TC_MODE_AUTO
                                ? tc::grad_auto_kernel<tc::kGradParamsAssembias>
                                : tc::grad_cross_kernel<tc::kGradParamsAssembias>,
                            device, grid, lds, stream, k0, k1, ga);
}

template <>
int launch_grad_family<tc::kGradParamsAssembias, tc::GradInterpArgs>(
    int mode, int device, dim3 grid, int lds, hipStream_t stream, hipEvent_t k0, hipEvent_t k1,
    const tc::GradInterpArgs& ga) {
  return launch_grad_kernel(mode == TC_MODE_AUTO
                                ? tc::grad_interp_auto_kernel<tc::kGradParamsAssembias>
                                : tc::grad_interp_cross_kernel<tc::kGradParamsAssembias>,
                            device, grid, lds, stream, k0, k1, ga);
}

}  // namespace host
}  // namespace tc
