// Device code that the derivative kernels share (grad_kernels.hip.h, grad_interp_kernels.hip.h,
// vjp_kernels.hip.h); grad.h itself stays plain C++ for the host-only units.
#pragma once

#include <hip/hip_runtime.h>

#include "grad.h"

namespace tc {
namespace grad {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// The draw a column reads: the columns beyond the batch repeat its last draw and store nothing.
__device__ __forceinline__ int64_t clamp_draw(int64_t draw, int64_t n_draws) {
  return draw < n_draws ? draw : n_draws - 1;
}

// The four row groups of a draw: (0 + 1) + (2 + 3), in every lane.
__device__ __forceinline__ double sum_row_groups(double value) {
  value += __shfl_xor(value, 16);
  value += __shfl_xor(value, 32);
  return value;
}

// One tile of U = S W on the matrix pipe, one wave: a_lane is the lane's first double of the
// tile's `steps` steps of the dense operand (grad.h), matrix column j multiplies the LDS row
// row(j) of w.  lane = (row group, draw col); D[row = group + 4 v][draw] in component v.
template <typename Row>
__device__ __forceinline__ f64x4 dense_tile_product(const double* a_lane, int steps,
                                                    const double* w, int group, int col, Row row) {
  f64x4 u = {0.0, 0.0, 0.0, 0.0};
  // four steps per round, the operands of the next round fetched ahead of this round's
  // matrix instructions (a step beyond the last one repeats it and is not multiplied)
  double a_now[4], a_next[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) a_now[s] = a_lane[(size_t)(s < steps ? s : steps - 1) * 64];
  for (int step0 = 0; step0 < steps; step0 += 4) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int next = step0 + 4 + s;
      a_next[s] = a_lane[(size_t)(next < steps ? next : steps - 1) * 64];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int step = step0 + s;
      if (step < steps) {
        const double b = w[row(4 * step + group) * kGradDraws + col];
        u = __builtin_amdgcn_mfma_f64_16x16x4f64(a_now[s], b, u, 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) a_now[s] = a_next[s];
  }
  return u;
}

// sum + T_r[slab] . (quantity p of the slab) for one draw, in bin order.  SLAB: the bins the
// slab (quantities, SLAB, 16) at w is laid out for.
template <int SLAB = kGradCrossSlab>
__device__ __forceinline__ double cross_slab_product(const double* matrix, int n_r, int r,
                                                     int slab0, int count, const double* w, int p,
                                                     int col, double sum) {
  const double* column = matrix + (size_t)slab0 * n_r + r;
  const double* rows = w + (size_t)p * SLAB * kGradDraws + col;
  for (int li = 0; li < count; ++li)
    sum = fma(column[(size_t)li * n_r], rows[li * kGradDraws], sum);
  return sum;
}

}  // namespace grad
}  // namespace tc
