// Gradient kernels of the Leauthaud11 family: the eleven-parameter instances of
// grad_kernels.hip.h and grad_interp_kernels.hip.h (grad_leauthaud11.h: the node arithmetic) and
// their launch, in a translation unit of their own as the other two sets (inst_grad.hip,
// inst_grad_assembias.hip).
#include "grad_interp_kernels.hip.h"
#include "grad_launch.hip.h"

namespace tc {
namespace host {

template <>
int launch_grad_family<tc::kGradParamsLeauthaud11, tc::GradArgs>(int mode, int device, dim3 grid,
                                                                 int lds, hipStream_t stream,
                                                                 hipEvent_t k0, hipEvent_t k1,
                                                                 const tc::GradArgs& ga) {
  return launch_grad_kernel(mode == TC_MODE_AUTO
                                ? tc::grad_auto_kernel<tc::kGradParamsLeauthaud11>
                                : tc::grad_cross_kernel<tc::kGradParamsLeauthaud11>,
                            device, grid, lds, stream, k0, k1, ga);
}

template <>
int launch_grad_family<tc::kGradParamsLeauthaud11, tc::GradInterpArgs>(
    int mode, int device, dim3 grid, int lds, hipStream_t stream, hipEvent_t k0, hipEvent_t k1,
    const tc::GradInterpArgs& ga) {
  return launch_grad_kernel(mode == TC_MODE_AUTO
                                ? tc::grad_interp_auto_kernel<tc::kGradParamsLeauthaud11>
                                : tc::grad_interp_cross_kernel<tc::kGradParamsLeauthaud11>,
                            device, grid, lds, stream, k0, k1, ga);
}

}  // namespace host
}  // namespace tc
