// One-launch kernels of mode auto (predict_fused_kernel), eight waves x 64 draws -- the
// instances launch.hip: run_fused can select, in translation units of their own (the family is
// most of the library's device code; the units compile in parallel).  This unit holds every
// instance inst_fused.h: launch_fused_shape lists, the deferred pairs included.
#include "inst_fused.h"

namespace tc {
namespace host {

int launch_fused_instance(const FusedInstance& in, int device, int n_u, dim3 grid, dim3 block,
                          int lds, hipStream_t stream, hipEvent_t k0, hipEvent_t k1,
                          const tc::FusedArgs& fa) {
  const FusedLaunch l{device, n_u, grid, block, lds, stream, k0, k1, fa};
  if (in.draws == 40) return launch_fused_instance_40(in, l);
  if (in.draws == 32) return launch_fused_instance_32(in, l);
  if (in.waves == 16) return launch_fused_instance_16(in, l);
  return launch_fused_shape<8, 64>(in, l);
}

}  // namespace host
}  // namespace tc
