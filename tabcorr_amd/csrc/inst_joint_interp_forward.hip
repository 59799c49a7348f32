// The joint forward kernel of interpolators (joint_interp_forward_kernels.hip.h:
// joint_interp_forward_kernel) and its launch, in a translation unit of its own: ten nodes per
// bin or any number, each as an (assembias, modulate) square, in the joint's form (rows or
// slabs); joint_interp.cpp fills the arguments.
#include "dispatch.h"
#include "internal.h"
#include "joint_interp_forward_kernels.hip.h"

namespace tc {
namespace host {

int launch_joint_interp_forward_instance(int n_gauss, bool assembias, bool modulate, int form,
                                         int device, dim3 grid, int lds, hipStream_t stream,
                                         hipEvent_t k0, hipEvent_t k1,
                                         const tc::JointInterpForwardArgs& ja) {
  auto launch = [&](auto ng) {
    return with_bools(
        [&](auto ab, auto mo, auto rows) {
          const auto kernel =
              tc::joint_interp_forward_kernel<ng(), ab(), mo(),
                                              rows() ? tc::kJointInterpRows
                                                     : tc::kJointInterpSlabs>;
          if (lds > 64 * 1024) {
            const int status = ensure_lds_limit((const void*)kernel, device, lds);
            if (status != TC_OK) return status;
          }
          hipExtLaunchKernelGGL(kernel, grid, dim3(64 * tc::kJointForwardWaves), lds, stream, k0,
                                k1, 0, ja);
          TC_HIP(hipGetLastError());
          return TC_OK;
        },
        assembias, modulate, form == tc::kJointInterpRows);
  };
  return n_gauss == 10 ? launch(int_c<10>{}) : launch(int_c<0>{});
}

}  // namespace host
}  // namespace tc
