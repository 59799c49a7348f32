// Weights of the not-a-knot cubic spline of one interpolator axis (interpolator.py:275-331), one
// text for the host and the device: the batch kernels' forward paths (kernels.hip.h), the
// un-batched interpolator call (interp.cpp), the gradient kernels (grad_interp_kernels.hip.h) and
// the host helper tc_spline_weights that tests/test_interp_grad_cpu.py pins against the oracle.
// `a`: the (n - 1, 4, n) matrix of spline_interpolation_matrix; `xp`: the n nodes of the axis.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define TC_SPLINE_HOST_DEVICE __host__ __device__
#else
#define TC_SPLINE_HOST_DEVICE
#endif

namespace tc {

// The segment of x: np.digitize with the right edge special-cased, clamped to the outermost
// segments -- an x beyond the grid gets that segment's polynomial (a NaN the first one).
TC_SPLINE_HOST_DEVICE inline int spline_segment(int n, const double* xp, double x) {
  int seg = -1;
  for (int i = 0; i < n; ++i) seg += xp[i] <= x ? 1 : 0;   // np.digitize(x, xp) - 1
  if (x == xp[n - 1]) seg = n - 2;
  return seg < 0 ? 0 : (seg > n - 2 ? n - 2 : seg);
}

// The weight of node j at x, with m = a + segment * 4 n, x2 = x x and x3 = x2 x.
TC_SPLINE_HOST_DEVICE inline double spline_node_weight(int n, const double* m, int j, double x,
                                                       double x2, double x3) {
  return m[j] + m[n + j] * x + m[2 * n + j] * x2 + m[3 * n + j] * x3;
}

// Weights of one axis: the spline through (xp, y) at x is sum_j weight[j] y[j] and its derivative
// sum_j dweight[j] y[j], for the nodes j = first, first + step, ... < n, stored `stride` doubles
// apart.  Returns the segment.
TC_SPLINE_HOST_DEVICE inline int spline_weights(int n, const double* xp, const double* a,
                                                double x, int first, int step, int stride,
                                                double* weight, double* dweight) {
  const int seg = spline_segment(n, xp, x);
  const double* m = a + (size_t)seg * 4 * n;
  const double x2 = x * x, x3 = x2 * x;
  for (int j = first; j < n; j += step) {
    weight[(size_t)j * stride] = spline_node_weight(n, m, j, x, x2, x3);
    dweight[(size_t)j * stride] = m[n + j] + 2.0 * m[2 * n + j] * x + 3.0 * m[3 * n + j] * x2;
  }
  return seg;
}

}  // namespace tc

#undef TC_SPLINE_HOST_DEVICE
