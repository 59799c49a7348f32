// The joint gradient kernel (joint_kernels.hip.h: grad_joint_kernel) and its launch, in a
// translation unit of its own: the instances of the plain five-parameter model and of the one
// decorated with assembly bias.  It has one form; joint.cpp fills the arguments.
#include "joint_kernels.hip.h"
#include "grad_launch.hip.h"

namespace tc {
namespace host {

int launch_grad_joint_instance(int n_params, int device, dim3 grid, int lds, hipStream_t stream,
                               hipEvent_t k0, hipEvent_t k1, const tc::JointArgs& ja) {
  return launch_grad_kernel(n_params == tc::kGradParamsAssembias
                                ? tc::grad_joint_kernel<tc::kGradParamsAssembias>
                                : tc::grad_joint_kernel<tc::kGradParams>,
                            device, grid, lds, stream, k0, k1, ja);
}

}  // namespace host
}  // namespace tc
