// predict_fused_kernel, sixteen waves x 64 draws (one workgroup per CU: forced or measured):
// the instances of inst_fused.h: launch_fused_shape but those with deferred pairs.
#include "inst_fused.h"

namespace tc {
namespace host {

int launch_fused_instance_16(const FusedInstance& in, const FusedLaunch& l) {
  return launch_fused_shape<16, 64>(in, l);
}

}  // namespace host
}  // namespace tc
