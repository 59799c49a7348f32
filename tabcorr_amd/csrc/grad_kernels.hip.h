// Gradient kernels: (ngal, xi[, chi2]) of a batch of Zheng07 draws together with their exact
// derivatives with respect to the five parameters, one launch per batch (grad.h: the argument
// block, the LDS budget and the operand layout; launch.hip: run_grad).  NP, a template parameter
// of every kernel and piece, is the number of differentiated parameters: 5, or 7 for the model
// decorated with assembly bias (the two strengths last), or 11 for the Leauthaud11 family
// (grad_leauthaud11.h: its node arithmetic, which the host runs too); "6" below reads NP + 1 there.
//
// A workgroup of four waves carries kGradDraws = 16 draws from theta to the results:
//   1  the node loops of every bin (tabcorr.py:537-578) for <N> and d<N>/dtheta_k, which share
//      their erf / exp / pow; w = n_h <N> and dw stay in LDS;
//   2  mode auto: per r bin U_r = S_r W on the FP64 matrix pipe (v_mfma_f64_16x16x4_f64: 16 rows
//      of S_r x 4 columns x 16 draws per instruction, the A operand one coalesced load from the
//      dense layout), then q_r = w . U_r and dq_r / dtheta_k = 2 dw_k . U_r; wave v takes the r
//      bins v, v + 4, ...;  mode cross: six matrix-vector products per r bin, slab by slab;
//   3  the chain rule (tabcorr.py:623-650) and, with a data vector, chi2, its gradient and, where
//      asked for, the Fisher matrix dxi_k^T P_sym dxi_l of the draw.
// There is ONE form: what a draw's results are made of -- the node sums in node order, the
// matrix products in column order, the sums over rows in row order, the fixed tree over the four
// row groups of a tile -- depends on the table alone, never on the batch or on the draw's
// neighbours: the results are batch-invariant by construction.
// Where the value's own formula divides by zero (ngal = 0, sigma_logM = 0) the derivatives are
// whatever IEEE arithmetic makes of it.
#pragma once

#include <hip/hip_runtime.h>

#include "fastmath.h"
#include "grad_device.hip.h"
#include "grad_leauthaud11.h"

namespace tc {

namespace grad {

struct Draw {
  double log_m_min, inv_sigma, m0, m0_ln10, inv_m1, alpha;
  // decorated: the clipped strengths c(A_cen), c(A_sat) and the clip's derivatives (1 inside
  // [-1, 1], 0 beyond, NaN for a NaN strength)
  double a_cen, da_cen, a_sat, da_sat;
};

constexpr bool decorated(int np) { return np == kGradParamsAssembias; }

// The per-draw constants of a family's node loops.
template <int NP>
struct DrawOf {
  typedef Draw type;
};
template <>
struct DrawOf<kGradParamsLeauthaud11> {
  typedef Leauthaud11Draw type;
};

// <N_cen> and its derivatives with respect to logMmin and sigma_logM at one node:
// N = (1 + erf x) / 2, dN/dlogMmin = -exp(-x^2) / (sigma sqrt(pi)), dN/dsigma = x dN/dlogMmin
// (grad_leauthaud11.h: central_node_at, with the Gaussian's tails).
__device__ __forceinline__ void central_node(const double* mt, const fm::Consts& k, const Draw& d,
                                             double log_m, double* n, double* dn0, double* dn1,
                                             double* x_abs = nullptr,
                                             double* gauss_out = nullptr) {
  central_node_at(mt, k, (log_m - d.log_m_min) * d.inv_sigma, d.inv_sigma, n, dn0, dn1, x_abs,
                  gauss_out);
}

// w = n_h <N> of bin i (library order: the centrals first) and its NP derivatives:
// out[0] = w, out[1 + k] = dw / dtheta_k.
// Decorated, with s = +-c(A) above / below the split as the forward kernels have it
// (kernels.hip.h: occ_nodes_zheng07, `median`): per central node N' = N + s_cen min(N, 1 - N),
// so dN'/dtheta_k = (1 + s_cen tau) dN/dtheta_k with tau = +-1 the branch fmin takes, and
// dN'/dA_cen = +-c'(A_cen) min(N, 1 - N); a satellite bin's sums take the factor 1 + s_sat
// (`modulate` multiplies by the PLAIN <N_cen>) and dN'/dA_sat = +-c'(A_sat) N.
// For the A_cen column min(N, 1 - N) = erfc(|x|) / 2 comes from the node's Gaussian once |x| >=
// fm::kErfcFrom (fastmath.h: half_erfc_from_gauss): as fmin(n, 1 - n) it carries the absolute
// rounding of n, 1e-16, which is 1e-8 of it at |x| = 4 -- nothing in the value N', where it
// stands next to n, but everything in a column that a draw with a narrow sigma_logM makes of
// such terms alone.  Below kErfcFrom it is at least 2e-4 and fmin's 5e-13 relative do.
template <int NP>
__device__ __forceinline__ void bin_values(const GradArgs& a, const fm::Consts& k, const Draw& d,
                                           int i, double out[NP + 1]) {
  const double* mt = a.math_table;
  const double* weight = a.weight + (size_t)i * a.n_gauss;
  double acc[NP + 1];
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) acc[p] = 0.0;
  const bool above = decorated(NP) ? a.percentile[i] > 0.5 : false;
  if (i < a.n_central) {
    const double* log_m = a.log_m + (size_t)i * a.n_gauss;
    const double s_cen = above ? d.a_cen : -d.a_cen;
    for (int node = 0; node < a.n_gauss; ++node) {
      double n, dn0, dn1, x_abs, gauss;
      central_node(mt, k, d, log_m[node], &n, &dn0, &dn1, &x_abs, &gauss);
      const double wn = weight[node];
      if (decorated(NP)) {
        const double rest = 1.0 - n;
        const double least = fmin(n, rest);
        const double factor = n <= rest ? 1.0 + s_cen : 1.0 - s_cen;
        n = fma(s_cen, least, n);
        dn0 *= factor;
        dn1 *= factor;
        const double tail = fm::half_erfc_from_gauss(x_abs, gauss);
        acc[NP - 1] = fma(wn, x_abs >= fm::kErfcFrom ? tail : least, acc[NP - 1]);
      }
      acc[0] = fma(wn, n, acc[0]);
      acc[1] = fma(wn, dn0, acc[1]);
      acc[2] = fma(wn, dn1, acc[2]);
    }
    if (decorated(NP)) acc[NP - 1] *= above ? d.da_cen : -d.da_cen;
  } else {
    const double* m = a.m + (size_t)i * a.n_gauss;
    const double* log_m = a.log_m + (size_t)i * a.n_gauss;
    for (int node = 0; node < a.n_gauss; ++node) {
      // N = s^alpha with s = (M - M0) / M1 for M > M0, else 0 with zero derivatives (a node
      // exactly at M0 included): dN/dlogM0 = -alpha s^(alpha - 1) M0 ln 10 / M1 =
      // -alpha N M0 ln 10 / (M - M0), dN/dlogM1 = -alpha ln 10 N, dN/dalpha = N ln s
      const double diff = m[node] - d.m0;
      const bool use = diff > 0.0;
      const double safe = use ? diff : 1.0;
      const double s = use ? diff * d.inv_m1 : 1.0;
      const double log2_s = fm::log2_fast(mt, k, s);
      const double n = fm::exp2_fast(mt, k, d.alpha * log2_s, use);
      double v[6];
      v[0] = n;
      v[1] = 0.0;
      v[2] = 0.0;
      v[3] = -d.alpha * n * d.m0_ln10 / safe;
      v[4] = -d.alpha * kLn10 * n;
      v[5] = n * fm::ln_from_log2(log2_s);
      if (a.modulate) {
        // product rule with <N_cen> at the satellites' node
        double c, dc0, dc1;
        central_node(mt, k, d, log_m[node], &c, &dc0, &dc1);
        v[1] = n * dc0;
        v[2] = n * dc1;
        v[0] *= c;
        v[3] *= c;
        v[4] *= c;
        v[5] *= c;
      }
      const double wn = weight[node];
#pragma unroll
      for (int p = 0; p < 6; ++p) acc[p] = fma(wn, v[p], acc[p]);
    }
    if (decorated(NP)) {
      const double s_sat = above ? d.a_sat : -d.a_sat;
      acc[NP] = (above ? d.da_sat : -d.da_sat) * acc[0];
#pragma unroll
      for (int p = 0; p < 6; ++p) acc[p] = fma(s_sat, acc[p], acc[p]);
    }
  }
  const double n_h = a.n_h[i];
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) out[p] = n_h * acc[p];
}

// The same for the Leauthaud11 family: out[0] = w, out[1 + k] = dw / dtheta_k, k = 0 .. 10; a
// central bin's last five are zero.  One Newton solve per central node, and with
// modulate_with_cenocc one per satellite node.
template <int NP>
__device__ __forceinline__ void bin_values(const GradArgs& a, const fm::Consts& k,
                                           const Leauthaud11Draw& d, int i, double out[NP + 1]) {
  static_assert(NP == kGradParamsLeauthaud11, "the Leauthaud11 family has eleven parameters");
  const double* mt = a.math_table;
  const double* weight = a.weight + (size_t)i * a.n_gauss;
  const double* log_m = a.log_m + (size_t)i * a.n_gauss;
  double acc[NP + 1];
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) acc[p] = 0.0;
  if (i < a.n_central) {
    for (int node = 0; node < a.n_gauss; ++node) {
      double v[7];
      leauthaud11_central_node(mt, k, d, log_m[node], v);
      const double wn = weight[node];
#pragma unroll
      for (int p = 0; p < 7; ++p) acc[p] = fma(wn, v[p], acc[p]);
    }
  } else {
    const double* m = a.m + (size_t)i * a.n_gauss;
    for (int node = 0; node < a.n_gauss; ++node) {
      double c[7], v[NP + 1];
      if (a.modulate) leauthaud11_central_node(mt, k, d, log_m[node], c);
      leauthaud11_satellite_node(mt, k, d, log_m[node], m[node], a.modulate != 0, c, v);
      const double wn = weight[node];
#pragma unroll
      for (int p = 0; p < NP + 1; ++p) acc[p] = fma(wn, v[p], acc[p]);
    }
  }
  const double n_h = a.n_h[i];
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) out[p] = n_h * acc[p];
}

// The clip of a strength to [-1, 1] as the forward kernels apply it (kernels.hip.h:
// clip_strength; NaN stays NaN) and its derivative, at the boundary the one facing inside.
__device__ __forceinline__ void clip_strength_grad(double a, double* c, double* dc) {
  *c = a > 1.0 ? 1.0 : (a < -1.0 ? -1.0 : a);
  *dc = a != a ? a : (fabs(a) <= 1.0 ? 1.0 : 0.0);
}

template <int NP>
__device__ __forceinline__ typename DrawOf<NP>::type load_draw(const GradArgs& a,
                                                               const fm::Consts& k,
                                                               int64_t draw) {
  const double* theta = a.theta + clamp_draw(draw, a.n_draws) * NP;
  Draw d;
  d.log_m_min = theta[0];
  d.inv_sigma = 1.0 / theta[1];
  d.m0 = fm::exp10_fast(a.math_table, k, theta[2]);
  d.m0_ln10 = d.m0 * kLn10;
  d.inv_m1 = 1.0 / fm::exp10_fast(a.math_table, k, theta[3]);
  d.alpha = theta[4];
  d.a_cen = d.da_cen = d.a_sat = d.da_sat = 0.0;
  if (decorated(NP)) {
    clip_strength_grad(theta[NP - 2], &d.a_cen, &d.da_cen);
    clip_strength_grad(theta[NP - 1], &d.a_sat, &d.da_sat);
  }
  return d;
}

template <>
__device__ __forceinline__ Leauthaud11Draw load_draw<kGradParamsLeauthaud11>(
    const GradArgs& a, const fm::Consts& k, int64_t draw) {
  return prepare_leauthaud11(a.math_table, k,
                             a.theta + clamp_draw(draw, a.n_draws) * kGradThetaLeauthaud11);
}

// LDS row of (bin i, quantity p) in grad_auto_kernel, by the family's trait (grad.h:
// grad_central_row, grad_satellite_row, grad_auto_rows).  Decorated: a central bin's fourth row is
// p = 6 (A_cen), a satellite bin's seventh p = 7 (A_sat).
template <int NP>
__device__ __forceinline__ int auto_row(int i, int p, int n_bins, int n_central, int zero_row) {
  if (i >= n_bins) return zero_row;
  if (i < n_central) {
    const int row = grad_central_row(NP, p);
    return row < 0 ? zero_row : grad_central_rows(NP) * i + row;
  }
  const int row = grad_satellite_row(NP, p);
  return row < 0 ? zero_row
                 : grad_central_rows(NP) * n_central + grad_satellite_rows(NP) * (i - n_central) +
                       row;
}

// chi2 = e^T P e and dchi2 / dtheta_k = 2 e^T P_sym dxi_k with P_sym = (P + P^T) / 2, from the
// residuals e (p = 0) and the derivatives (p = 1 .. n_quantities - 1: NP for a table, NP + n_dim
// for an interpolator) at stash[(p n_r + r) 16 + draw]; threads 0 .. 16 n_quantities - 1 =
// (p, draw).
__device__ __forceinline__ void finish_chi2(const GradArgs& a, const double* stash, int64_t draw0,
                                            int n_quantities) {
  const int t = threadIdx.x;
  if (t >= n_quantities * kGradDraws) return;
  const int p = t / kGradDraws, col = t % kGradDraws;
  const int n_r = a.n_r;
  const double* precision = a.chi2_data + n_r;
  const double* e = stash + col;
  const double* right = stash + (size_t)p * n_r * kGradDraws + col;
  double sum = 0.0;
  for (int r = 0; r < n_r; ++r) {
    double row = 0.0;
    if (p == 0) {
      for (int s = 0; s < n_r; ++s) row = fma(precision[(size_t)r * n_r + s], e[s * kGradDraws], row);
    } else {
      for (int s = 0; s < n_r; ++s)
        row = fma(precision[(size_t)r * n_r + s] + precision[(size_t)s * n_r + r],
                  right[s * kGradDraws], row);
    }
    sum = fma(e[r * kGradDraws], row, sum);
  }
  const int64_t draw = draw0 + col;
  if (draw >= a.n_draws) return;
  if (p == 0)
    a.chi2[draw] = sum;
  else
    a.dchi2[draw * (n_quantities - 1) + (p - 1)] = sum;
}

// Fisher matrix of the likelihood, where a.fisher is given: fisher[k][l] = dxi_k^T P_sym dxi_l =
// 1/2 sum_r dxi_k[r] (sum_s (P[r][s] + P[s][r]) dxi_l[s]) over the n = n_quantities - 1
// differentiated quantities, from the rows p = 1 .. n of the stash that finish_chi2 reads (and
// leaves as they are: no barrier between the two).  Items (pair k <= l, draw), n (n + 1) / 2 x 16
// of them (240 for a table, up to 1456 for an interpolator of kGradMaxDim axes; 448 and 1920
// where decorated), walked by the
// workgroup; s ascending inside r ascending, one fma chain each, as in finish_chi2: a draw's
// matrix depends on the draw alone.  Every pair is computed once and stored to both positions of
// the full (n, n) matrix, which is therefore bit-symmetric.
__device__ __forceinline__ void finish_fisher(const GradArgs& a, const double* stash,
                                              int64_t draw0, int n_quantities) {
  if (a.fisher == nullptr) return;
  const int n = n_quantities - 1;
  const int n_r = a.n_r;
  const double* precision = a.chi2_data + n_r;
  const int n_items = n * (n + 1) / 2 * kGradDraws;
  for (int item = threadIdx.x; item < n_items; item += kGradThreads) {
    const int pair = item / kGradDraws, col = item % kGradDraws;
    // pair = l (l + 1) / 2 + k with k <= l
    int l = 0;
    while ((l + 1) * (l + 2) / 2 <= pair) ++l;
    const int k = pair - l * (l + 1) / 2;
    const double* left = stash + (size_t)(k + 1) * n_r * kGradDraws + col;
    const double* right = stash + (size_t)(l + 1) * n_r * kGradDraws + col;
    double sum = 0.0;
    for (int r = 0; r < n_r; ++r) {
      double row = 0.0;
      for (int s = 0; s < n_r; ++s)
        row = fma(precision[(size_t)r * n_r + s] + precision[(size_t)s * n_r + r],
                  right[s * kGradDraws], row);
      sum = fma(left[r * kGradDraws], row, sum);
    }
    sum *= 0.5;
    const int64_t draw = draw0 + col;
    if (draw >= a.n_draws) continue;
    double* out = a.fisher + draw * n * n;
    out[k * n + l] = sum;
    out[l * n + k] = sum;
  }
}

// ---- the pieces of grad_auto_kernel (grad_interp_auto_kernel runs them per class and table,
// joint_kernels.hip.h: grad_joint_kernel once per draw and then per table of a joint) ----------

// Phase 1: thread = (bin i % 16, draw) writes w and dw of its bins, and the row of zeros.
template <int NP>
__device__ __forceinline__ void auto_node_loops(const GradArgs& a, const fm::Consts& k,
                                                const typename DrawOf<NP>::type& d, double* w,
                                                int zero_row) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central;
  if (t < kGradDraws) w[zero_row * kGradDraws + t] = 0.0;
  for (int i = t / kGradDraws; i < n_bins; i += kGradThreads / kGradDraws) {
    double out[NP + 1];
    bin_values<NP>(a, k, d, i, out);
    if (grad_rows_in_order(NP)) {
      const int base = auto_row<NP>(i, 0, n_bins, n_central, zero_row);
      const int count = i < n_central ? grad_central_rows(NP) : grad_satellite_rows(NP);
#pragma unroll
      for (int p = 0; p < NP + 1; ++p)
        if (p < count) w[(base + p) * kGradDraws + col] = out[p];
    } else {
      // (the rows a bin does not have are the row of zeros: not written)
#pragma unroll
      for (int p = 0; p < NP + 1; ++p) {
        const int row = auto_row<NP>(i, p, n_bins, n_central, zero_row);
        if (row != zero_row) w[row * kGradDraws + col] = out[p];
      }
    }
  }
}

// Total of quantity p over the bins in bin order: ngal (p = 0) or dngal / dtheta_(p - 1).
template <int NP>
__device__ __forceinline__ double auto_total(const double* w, int p, int col, int n_bins,
                                             int n_central, int zero_row) {
  double sum = 0.0;
  for (int i = 0; i < n_bins; ++i)
    sum += w[auto_row<NP>(i, p, n_bins, n_central, zero_row) * kGradDraws + col];
  return sum;
}

// Phase 2 of one r bin, one wave: U_r = S_r W on the matrix pipe against a.matrix, then acc[0] =
// w . U_r and acc[p] = dw_p . U_r, complete in every lane.  lane = (row group l / 16, draw
// l % 16); D[row = l / 16 + 4 v][draw] in register v.
template <int NP>
__device__ __forceinline__ void auto_products(const GradArgs& a, const double* w, int r,
                                              int zero_row, double acc[NP + 1]) {
  const int lane = threadIdx.x % 64;
  const int group = lane / kGradDraws, col = lane % kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central;
  const int tiles = a.row_tiles, steps = a.k_steps;
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) acc[p] = 0.0;
  for (int tile = 0; tile < tiles; ++tile) {
    const double* a_lane = a.matrix + ((size_t)r * tiles + tile) * steps * 64 + lane;
    const f64x4 u = dense_tile_product(a_lane, steps, w, group, col, [=](int j) {
      return auto_row<NP>(j, 0, n_bins, n_central, zero_row);
    });
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = 16 * tile + group + 4 * v;
      const double uv = u[v];
#pragma unroll
      for (int p = 0; p < NP + 1; ++p)
        acc[p] = fma(w[auto_row<NP>(i, p, n_bins, n_central, zero_row) * kGradDraws + col], uv,
                     acc[p]);
    }
  }
#pragma unroll
  for (int p = 0; p < NP + 1; ++p) acc[p] = sum_row_groups(acc[p]);
}

// Phase 3, mode auto: xi = q / ngal^2 and dxi_k = dq_k / ngal^2 - 2 xi dngal_k / ngal with dq_k =
// 2 dw_k . U, from the products and the totals (6, 16) of the draw's column.
__device__ __forceinline__ double auto_xi(const double* acc, double inv_ngal2) {
  return acc[0] * inv_ngal2;
}
__device__ __forceinline__ double auto_dxi(const double* acc, int p, double xi,
                                           const double* total, int col, double inv_ngal,
                                           double inv_ngal2) {
  return 2.0 * acc[p] * inv_ngal2 - 2.0 * xi * total[p * kGradDraws + col] * inv_ngal;
}

// Phase 1 of a workgroup whose rows stay in LDS (grad_auto_kernel, grad_joint_kernel): the node
// loops of every bin into w, then the totals over the bins in bin order -- total (6, 16) = ngal and
// its derivatives, stored for the draws of the batch --; both behind a barrier.
template <int NP>
__device__ __forceinline__ void auto_occupations(const GradArgs& a, const fm::Consts& k, double* w,
                                                 double* total, int64_t draw0, int zero_row) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  {
    const typename DrawOf<NP>::type d = load_draw<NP>(a, k, draw0 + col);
    auto_node_loops<NP>(a, k, d, w, zero_row);
  }
  __syncthreads();
  if (t < (NP + 1) * kGradDraws) {
    const int p = t / kGradDraws;
    const double sum = auto_total<NP>(w, p, col, a.n_bins, a.n_central, zero_row);
    total[t] = sum;
    const int64_t draw = draw0 + col;
    if (draw < a.n_draws) {
      if (p == 0)
        a.ngal[draw] = sum;
      else
        a.dngal[draw * NP + (p - 1)] = sum;
    }
  }
  __syncthreads();
}

// Where quantity p (0: the value, 1 + k: its derivative) of row r of the a.n_r result rows of a
// draw goes: the prediction's arrays, or -- the likelihood -- the stash that finish_chi2 and
// finish_fisher read, the value as its residual against the data.
template <int NP>
__device__ __forceinline__ void store_result(const GradArgs& a, double* stash, int64_t draw,
                                             int col, int r, int p, double value) {
  const int n_r = a.n_r;
  if (a.xi != nullptr) {
    if (draw >= a.n_draws) return;
    if (p == 0)
      a.xi[draw * n_r + r] = value;
    else
      a.dxi[(draw * NP + (p - 1)) * n_r + r] = value;
  } else {
    stash[((size_t)p * n_r + r) * kGradDraws + col] = p == 0 ? value - a.chi2_data[r] : value;
  }
}

// Phase 3 of one r bin of mode auto, one wave: xi and dxi from the products `acc` (auto_products)
// and the totals, written to result row r by the wave's first row group.
template <int NP>
__device__ __forceinline__ void auto_store_row(const GradArgs& a, const double* acc,
                                               const double* total, double* stash, int64_t draw,
                                               int r, double inv_ngal, double inv_ngal2) {
  const int lane = threadIdx.x % 64;
  const int group = lane / kGradDraws, col = lane % kGradDraws;
  const double xi = auto_xi(acc, inv_ngal2);
  if (group == 0) store_result<NP>(a, stash, draw, col, r, 0, xi);
#pragma unroll
  for (int p = 1; p < NP + 1; ++p) {
    const double dxi = auto_dxi(acc, p, xi, total, col, inv_ngal, inv_ngal2);
    if (group == 0) store_result<NP>(a, stash, draw, col, r, p, dxi);
  }
}

// Phase 3, mode cross: xi = y_0 / ngal and dxi_k = (y_k - xi dngal_k) / ngal from the products
// y_p = T_r . (quantity p of the bins).
__device__ __forceinline__ double cross_xi(double y0, double inv_ngal) { return y0 * inv_ngal; }
__device__ __forceinline__ double cross_dxi(double y, double xi, double dngal, double inv_ngal) {
  return (y - xi * dngal) * inv_ngal;
}

// ---- the pieces of grad_cross_kernel ------------------------------------------------------------

// w and dw of the bins slab0 .. slab0 + count - 1 into the slab (6, SLAB, 16).
template <int NP, int SLAB = kGradCrossSlab>
__device__ __forceinline__ void cross_node_loops(const GradArgs& a, const fm::Consts& k,
                                                 const typename DrawOf<NP>::type& d, int slab0,
                                                 int count, double* w) {
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  for (int li = t / kGradDraws; li < count; li += kGradThreads / kGradDraws) {
    double out[NP + 1];
    bin_values<NP>(a, k, d, slab0 + li, out);
#pragma unroll
    for (int p = 0; p < NP + 1; ++p) w[(p * SLAB + li) * kGradDraws + col] = out[p];
  }
}

}  // namespace grad

// ---- mode auto ----------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(kGradThreads) void grad_auto_kernel(const GradArgs a) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_central = a.n_central, n_r = a.n_r;
  const int zero_row = grad_auto_rows(n_bins, n_central, NP) - 1;
  double* w = grad_lds;                                       // (rows, 16)
  double* total = w + (size_t)(zero_row + 1) * kGradDraws;    // (6, 16)
  double* stash = total + NQ * kGradDraws;                     // (6, n_r, 16), likelihood only
  const fm::Consts k = fm::make_consts();

  // phase 1: thread = (bin i % 16, draw); the totals are ngal and its derivatives
  grad::auto_occupations<NP>(a, k, w, total, draw0, zero_row);

  // phase 2: wave v takes the r bins v, v + 4, ...
  const int wave = t / 64;
  const double ngal = total[col];
  const double inv_ngal = 1.0 / ngal;
  const double inv_ngal2 = 1.0 / (ngal * ngal);
  for (int r = wave; r < n_r; r += kGradWaves) {
    double acc[NQ];
    grad::auto_products<NP>(a, w, r, zero_row, acc);
    grad::auto_store_row<NP>(a, acc, total, stash, draw0 + col, r, inv_ngal, inv_ngal2);
  }
  if (a.xi == nullptr) {
    __syncthreads();
    grad::finish_chi2(a, stash, draw0, NQ);
    grad::finish_fisher(a, stash, draw0, NQ);
  }
}

// ---- mode cross ---------------------------------------------------------------------------------
// xi_r = T_r . w / ngal (tabcorr.py:646-649): the bins in slabs of kGradCrossSlab, any number of
// them; thread = (r, quantity, draw) items for the products, which it keeps in LDS.
template <int NP>
__global__ __launch_bounds__(kGradThreads) void grad_cross_kernel(const GradArgs a) {
  constexpr int NQ = NP + 1;
  extern __shared__ double grad_lds[];
  const int t = threadIdx.x;
  const int col = t % kGradDraws;
  const int64_t draw0 = (int64_t)blockIdx.x * kGradDraws;
  const int n_bins = a.n_bins, n_r = a.n_r;
  double* w = grad_lds;                                               // (6, slab, 16)
  double* y = w + NQ * kGradCrossSlab * kGradDraws;                    // (6, n_r, 16)
  double* total = y + (size_t)NQ * n_r * kGradDraws;                   // (6, 16)
  const fm::Consts k = fm::make_consts();
  const typename grad::DrawOf<NP>::type d = grad::load_draw<NP>(a, k, draw0 + col);
  const int n_items = NQ * n_r * kGradDraws;
  for (int item = t; item < n_items; item += kGradThreads) y[item] = 0.0;
  double my_total = 0.0;
  for (int slab0 = 0; slab0 < n_bins; slab0 += kGradCrossSlab) {
    const int count = min(kGradCrossSlab, n_bins - slab0);
    __syncthreads();
    grad::cross_node_loops<NP>(a, k, d, slab0, count, w);
    __syncthreads();
    if (t < NQ * kGradDraws) {
      const int p = t / kGradDraws;
      for (int li = 0; li < count; ++li) my_total += w[(p * kGradCrossSlab + li) * kGradDraws + col];
    }
    for (int item = t; item < n_items; item += kGradThreads) {
      const int r = item / (NQ * kGradDraws), p = item / kGradDraws % NQ;
      const size_t slot = ((size_t)p * n_r + r) * kGradDraws + col;
      y[slot] = grad::cross_slab_product(a.matrix, n_r, r, slab0, count, w, p, col, y[slot]);
    }
  }
  if (t < NQ * kGradDraws) {
    total[t] = my_total;
    const int p = t / kGradDraws;
    const int64_t draw = draw0 + col;
    if (draw < a.n_draws) {
      if (p == 0)
        a.ngal[draw] = my_total;
      else
        a.dngal[draw * NP + (p - 1)] = my_total;
    }
  }
  __syncthreads();
  // xi = y_0 / ngal, dxi_k = (y_k - xi dngal_k) / ngal: first the derivatives (they read y_0),
  // then the values
  const double inv_ngal = 1.0 / total[col];
  const int64_t draw = draw0 + col;
  for (int item = t; item < n_items; item += kGradThreads) {
    const int r = item / (NQ * kGradDraws), p = item / kGradDraws % NQ;
    if (p == 0) continue;
    const size_t slot = ((size_t)p * n_r + r) * kGradDraws + col;
    const double xi = grad::cross_xi(y[(size_t)r * kGradDraws + col], inv_ngal);
    const double dxi = grad::cross_dxi(y[slot], xi, total[p * kGradDraws + col], inv_ngal);
    if (a.xi == nullptr)
      y[slot] = dxi;
    else if (draw < a.n_draws)
      a.dxi[(draw * NP + (p - 1)) * n_r + r] = dxi;
  }
  __syncthreads();
  for (int item = t; item < n_r * kGradDraws; item += kGradThreads) {
    const int r = item / kGradDraws;
    const double xi = grad::cross_xi(y[item], inv_ngal);   // (item % 16 == col: 256 = 16 x 16)
    if (a.xi == nullptr)
      y[item] = xi - a.chi2_data[r];
    else if (draw < a.n_draws)
      a.xi[draw * n_r + r] = xi;
  }
  if (a.xi == nullptr) {
    __syncthreads();
    grad::finish_chi2(a, y, draw0, NQ);
    grad::finish_fisher(a, y, draw0, NQ);
  }
}

}  // namespace tc
