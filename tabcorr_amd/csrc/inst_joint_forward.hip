// The joint forward kernel (joint_forward_kernels.hip.h: joint_forward_kernel) and its launch, in
// a translation unit of its own: ten nodes per bin or any number, each as an (assembias,
// modulate) square.  It has one form; joint.cpp fills the arguments.
#include "dispatch.h"
#include "internal.h"
#include "joint_forward_kernels.hip.h"

namespace tc {
namespace host {

int launch_joint_forward_instance(int n_gauss, bool assembias, bool modulate, int device,
                                  dim3 grid, int lds, hipStream_t stream, hipEvent_t k0,
                                  hipEvent_t k1, const tc::JointForwardArgs& ja) {
  auto launch = [&](auto ng) {
    return with_bools(
        [&](auto ab, auto mo) {
          const auto kernel = tc::joint_forward_kernel<ng(), ab(), mo()>;
          if (lds > 64 * 1024) {
            const int status = ensure_lds_limit((const void*)kernel, device, lds);
            if (status != TC_OK) return status;
          }
          hipExtLaunchKernelGGL(kernel, grid, dim3(64 * tc::kJointForwardWaves), lds, stream, k0,
                                k1, 0, ja);
          TC_HIP(hipGetLastError());
          return TC_OK;
        },
        assembias, modulate);
  };
  return n_gauss == 10 ? launch(int_c<10>{}) : launch(int_c<0>{});
}

}  // namespace host
}  // namespace tc
