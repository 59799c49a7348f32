// Occupation VJP kernels (vjp_kernels.hip.h: vjp_auto_kernel, vjp_cross_kernel) and their launch,
// in a translation unit of their own.  Each has one form; launch.hip: run_vjp fills the arguments.
#include "grad_launch.hip.h"
#include "vjp_kernels.hip.h"

namespace tc {
namespace host {

int launch_vjp_instance(int mode, int device, dim3 grid, int lds, hipStream_t stream,
                        hipEvent_t k0, hipEvent_t k1, const tc::VjpArgs& va) {
  return launch_grad_kernel(mode == TC_MODE_AUTO ? tc::vjp_auto_kernel : tc::vjp_cross_kernel,
                            device, grid, lds, stream, k0, k1, va);
}

}  // namespace host
}  // namespace tc
