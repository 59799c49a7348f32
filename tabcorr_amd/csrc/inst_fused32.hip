// predict_fused_kernel, eight waves x 32 draws (batches below 8192 draws, tables of 105-208 bins):
// of the instances of inst_fused.h: launch_fused_shape those with ten nodes and Leauthaud11,
// none with deferred pairs.
#include "inst_fused.h"

namespace tc {
namespace host {

int launch_fused_instance_32(const FusedInstance& in, const FusedLaunch& l) {
  return launch_fused_shape<8, 32>(in, l);
}

}  // namespace host
}  // namespace tc
