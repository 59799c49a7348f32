// The joint gradient kernel of interpolators (joint_interp_kernels.hip.h: grad_joint_interp_kernel)
// and its launch, in a translation unit of its own: both forms, for the plain five-parameter
// model and for the one decorated with assembly bias.  joint_interp.cpp fills the arguments.
#include "joint_interp_kernels.hip.h"
#include "grad_launch.hip.h"

namespace tc {
namespace host {

namespace {
template <int NP>
int launch_form(int form, int device, dim3 grid, int lds, hipStream_t stream, hipEvent_t k0,
                hipEvent_t k1, const tc::JointInterpArgs& ja) {
  return launch_grad_kernel(form == tc::kJointInterpRows
                                ? tc::grad_joint_interp_kernel<NP, tc::kJointInterpRows>
                                : tc::grad_joint_interp_kernel<NP, tc::kJointInterpSlabs>,
                            device, grid, lds, stream, k0, k1, ja);
}
}  // namespace

int launch_grad_joint_interp_instance(int n_params, int form, int device, dim3 grid, int lds,
                                      hipStream_t stream, hipEvent_t k0, hipEvent_t k1,
                                      const tc::JointInterpArgs& ja) {
  return n_params == tc::kGradParamsAssembias
             ? launch_form<tc::kGradParamsAssembias>(form, device, grid, lds, stream, k0, k1, ja)
             : launch_form<tc::kGradParams>(form, device, grid, lds, stream, k0, k1, ja);
}

}  // namespace host
}  // namespace tc
