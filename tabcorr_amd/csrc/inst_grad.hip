// Gradient kernels (grad_kernels.hip.h: grad_auto_kernel, grad_cross_kernel; grad_interp_kernels.
// hip.h: grad_interp_auto_kernel, grad_interp_cross_kernel) and their launch, in a translation unit
// of their own: the instances of the plain five-parameter model (inst_grad_assembias.hip: the
// seven-parameter ones).  Each has one form; launch.hip: run_grad and interp.cpp fill the
// arguments and reach the family through launch_grad_instance.
#include "grad_interp_kernels.hip.h"
#include "grad_launch.hip.h"

namespace tc {
namespace host {

template <>
int launch_grad_family<tc::kGradParams, tc::GradArgs>(int mode, int device, dim3 grid, int lds,
                                                      hipStream_t stream, hipEvent_t k0,
                                                      hipEvent_t k1, const tc::GradArgs& ga) {
  return launch_grad_kernel(mode == TC_MODE_AUTO ? tc::grad_auto_kernel<tc::kGradParams>
                                                  : tc::grad_cross_kernel<tc::kGradParams>,
                            device, grid, lds, stream, k0, k1, ga);
}

template <>
int launch_grad_family<tc::kGradParams, tc::GradInterpArgs>(int mode, int device, dim3 grid,
                                                            int lds, hipStream_t stream,
                                                            hipEvent_t k0, hipEvent_t k1,
                                                            const tc::GradInterpArgs& ga) {
  return launch_grad_kernel(
      mode == TC_MODE_AUTO ? tc::grad_interp_auto_kernel<tc::kGradParams>
                           : tc::grad_interp_cross_kernel<tc::kGradParams>,
      device, grid, lds, stream, k0, k1, ga);
}

}  // namespace host
}  // namespace tc
