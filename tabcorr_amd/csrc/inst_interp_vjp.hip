// The occupation-seam kernels of an interpolator (interp_vjp_kernels.hip.h) and their launch, in
// a translation unit of their own.  Each has one form; interp.cpp fills the arguments.
#include "grad_launch.hip.h"
#include "interp_vjp_kernels.hip.h"

namespace tc {
namespace host {

int launch_vjp_interp_instance(int mode, int device, dim3 grid, int lds, hipStream_t stream,
                               hipEvent_t k0, hipEvent_t k1, const tc::InterpVjpArgs& ia) {
  return launch_grad_kernel(mode == TC_MODE_AUTO ? tc::vjp_interp_auto_kernel
                                                 : tc::vjp_interp_cross_kernel,
                            device, grid, lds, stream, k0, k1, ia);
}

}  // namespace host
}  // namespace tc
