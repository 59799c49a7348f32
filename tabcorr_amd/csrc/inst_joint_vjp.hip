// The occupation-seam kernel of a joint (joint_vjp_kernels.hip.h: vjp_joint_kernel) and its
// launch, in a translation unit of its own.  It has one form; joint.cpp fills the arguments.
#include "grad_launch.hip.h"
#include "joint_vjp_kernels.hip.h"

namespace tc {
namespace host {

int launch_vjp_joint_instance(int device, dim3 grid, int lds, hipStream_t stream, hipEvent_t k0,
                              hipEvent_t k1, const tc::JointVjpArgs& ja) {
  return launch_grad_kernel(tc::vjp_joint_kernel, device, grid, lds, stream, k0, k1, ja);
}

}  // namespace host
}  // namespace tc
