// Joint forward kernel of several interpolators over one grid: (ngal, xi) or (ngal, chi2) of a
// batch of draws (theta, x) for ALL members in one launch, without any derivative
// (joint_interp.h: the argument block and the LDS budgets; joint_interp.cpp fills it in).  The
// forward counterpart of grad_joint_interp_kernel in the geometry of joint_forward_kernel
// (joint_forward_kernels.hip.h), composed of its pieces: a workgroup of kJointForwardWaves waves
// carries kJointForwardDraws = 64 draws, two tiles of 32; a lane is a draw, the draws behind the
// batch's last repeat it.
//   1  once per workgroup: the spline weights of the 64 draws on every axis (spline.h, as
//      predict_cross_fused_kernel forms them) into LDS; c_k of grid node k is their product;
//   2  the classes of halo tables in member 0's walk order, the occupations of a class ONCE for
//      all members (draw_params, occ_bin_zheng07 against the class's quadrature constants and n_h)
//      into the LDS densities dens[bin][64], the class's number density ngal_v, and
//      ngal += c_k ngal_v per node k of the class;
//      rows form (a member is mode auto): every bin of the class stays in LDS.  Per member in
//        list order:
//        mode auto   a PASS is (member, pair of r sub-tiles, part of the triangle, tile of 32
//                    draws), numbered through the list and dealt to the waves (wave, wave + 8,
//                    ...) as in joint_forward_kernel; the wave runs its pass on the member's table
//                    at every node of the class (fused_quad_pass over fused_walk.h) and adds
//                    (c_k / ngal_v^2) F into its part's slab of `sums`: the slabs ARE the
//                    accumulators;
//        mode cross  ONE fma chain per (node, row, draw) over the bins in library order, the rows
//                    in groups of kChains dealt to the waves behind the last pass;
//                    (c_k / ngal_v) x the chain's sum goes to part 0 of the row;
//      slab form (every member mode cross): the bins in slabs of kJointInterpForwardSlab, the
//        occupations once per slab; a chain is cut at the slab's end and c_k x its sum goes into
//        the class's products y (N, 64); ngal_v is complete behind the last slab:
//        sums += y / ngal_v once per class;
//   3  per row the parts in part order into the results tile (N, 65), then the end of
//      joint_forward_kernel: tile_write_xi, or chi2 = delta^T P delta.
// Order guarantees: ONE form per joint, chosen from the members' modes alone; a draw's results
// depend on the draw alone; a slot of `sums` (or y) belongs to one pass (one row group) whatever
// the class or node, so one wave adds into it in walk order and the arithmetic of a row does not
// depend on the wave that runs it; a wave sums the same bins of a class in both forms, so ngal
// depends on member 0's walk and on nothing else.
#pragma once

#include "joint_forward_kernels.hip.h"
#include "joint_interp.h"
#include "spline.h"

namespace tc {

namespace jif {

constexpr int kChains = 4;     // rows of one member a wave carries through one walk of the bins

// c_k of the grid node `node` for the lane's draw.
__device__ __forceinline__ double node_coef(const JointInterpForwardArgs& a, const double* weights,
                                            const int32_t* node, int col) {
  double c = 1.0;
  for (int e = 0; e < a.n_dim; ++e) c *= weights[(a.weight_row[e] + node[e]) * kLanes + col];
  return c;
}

// The occupations of the bins bin0 .. bin0 + count of class v into dens[0 .. count)[64], the bins
// strided over the waves; the wave's sums of the centrals and the satellites go on.
template <int NGAUSS, bool ASSEMBIAS, bool MODULATE>
__device__ __forceinline__ void class_occupations(const JointInterpForwardArgs& a,
                                                  const double* table, const fm::Consts& kc,
                                                  const DrawParams& dp, int v, int n_gauss,
                                                  int bin0, int count, double* dens, int lane,
                                                  int wave, double& sum_cen, double& sum_sat) {
  constexpr int W = kJointForwardWaves, DL = kJointForwardDraws;
  sc_f64 log_m = (sc_f64)a.class_log_m[v];
  sc_f64 mass = (sc_f64)a.class_m[v];
  sc_f64 weight = (sc_f64)a.class_weight[v];
  sc_f64 weight_sum = weight + a.n_bins * n_gauss;   // (get_quadrature: the bins' sums)
  sc_f64 n_h = (sc_f64)a.class_n_h[v];
  sc_f64 percentile = ASSEMBIAS ? (sc_f64)a.class_percentile[v] : nullptr;
  const double f1 = (1.0 - a.split) / a.split, f2 = a.split / (1.0 - a.split);
  for (int li = wave; li < count; li += W) {
    const int g = bin0 + li;
    const bool central = g < a.n_central;
    const bool above = ASSEMBIAS ? percentile[g] > a.split : false;
    const double acc = occ_bin_zheng07<NGAUSS, ASSEMBIAS, MODULATE>(
        table, kc, g, n_gauss, central, above, log_m, mass, weight, weight_sum, dp, f1, f2);
    const double value = acc * n_h[g];
    dens[li * DL + lane] = value;
    if (central) sum_cen += value; else sum_sat += value;
  }
}

// The class's number density from the waves' sums, in wave order.
__device__ __forceinline__ double class_ngal(double (*red)[kJointForwardWaves][kLanes], int lane) {
  double n_cen = 0.0, n_sat = 0.0;
#pragma unroll
  for (int w = 0; w < kJointForwardWaves; ++w) {
    n_cen += red[0][w][lane];
    n_sat += red[1][w][lane];
  }
  return n_cen + n_sat;
}

// C chains: rows r0 .. r0 + C of the (n_bins, n_r) matrix of one member at one node against the
// densities of the bins bin0 .. bin0 + count in dens[0 .. count)[64]; one LDS read feeds C fmas.
template <int C>
__device__ __forceinline__ void cross_chains(const void* matrix, int n_r, int r0, int bin0,
                                             int count, const double* dens, int lane,
                                             double (&sum)[C]) {
  sc_f64 m = (sc_f64)matrix + (size_t)bin0 * n_r + r0;
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = 0.0;
  for (int li = 0; li < count; ++li) {
    const double d = dens[li * kJointForwardDraws + lane];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = fma(m[li * n_r + c], d, sum[c]);
  }
}

// The groups of up to kChains consecutive rows of the mode-cross members, numbered through the
// list: group `g` is rows r0 .. r0 + count of member m; false behind the last group.
__device__ __forceinline__ bool cross_group(const JointInterpForwardArgs& a, int g, int& m,
                                            int& r0, int& count) {
  for (m = 0; m < a.n_members; ++m) {
    if (a.mode[m] != TC_MODE_CROSS) continue;
    const int groups = (a.n_rows[m] + kChains - 1) / kChains;
    if (g < groups) {
      r0 = g * kChains;
      count = a.n_rows[m] - r0 < kChains ? a.n_rows[m] - r0 : kChains;
      return true;
    }
    g -= groups;
  }
  return false;
}

// The chains of one group at one node, and `add(c, sum)` for every row of the group in row order.
template <class Add>
__device__ __forceinline__ void cross_group_chains(const void* matrix, int n_r, int r0, int rows,
                                                   int bin0, int count, const double* dens,
                                                   int lane, Add&& add) {
  if (rows == 4) {
    double sum[4];
    cross_chains<4>(matrix, n_r, r0, bin0, count, dens, lane, sum);
#pragma unroll
    for (int c = 0; c < 4; ++c) add(c, sum[c]);
  } else if (rows == 3) {
    double sum[3];
    cross_chains<3>(matrix, n_r, r0, bin0, count, dens, lane, sum);
#pragma unroll
    for (int c = 0; c < 3; ++c) add(c, sum[c]);
  } else if (rows == 2) {
    double sum[2];
    cross_chains<2>(matrix, n_r, r0, bin0, count, dens, lane, sum);
#pragma unroll
    for (int c = 0; c < 2; ++c) add(c, sum[c]);
  } else {
    double sum[1];
    cross_chains<1>(matrix, n_r, r0, bin0, count, dens, lane, sum);
    add(0, sum[0]);
  }
}

}  // namespace jif

template <int NGAUSS, bool ASSEMBIAS, bool MODULATE, int FORM>
__global__ __launch_bounds__(64 * kJointForwardWaves) void joint_interp_forward_kernel(
    const JointInterpForwardArgs a) {
  constexpr int W = kJointForwardWaves, DL = kJointForwardDraws;
  constexpr int PARTS = joint_forward_parts(W);
  constexpr bool ROWS = FORM == kJointInterpRows;
  extern __shared__ __attribute__((aligned(16))) double joint_interp_forward_lds[];
  const int n_total = a.n_r;
  const int tile_doubles = (n_total * (kLanes + 1) + 1) / 2 * 2;
  const int dens_doubles = (ROWS ? a.dens_rows : kJointInterpForwardSlab) * DL;
  const int region_b = dens_doubles > tile_doubles ? dens_doubles : tile_doubles;
  const int operand_doubles = n_total * (n_total + 1);
  const int region_a = fm::kTableDoubles > operand_doubles ? fm::kTableDoubles : operand_doubles;
  double* dens = joint_interp_forward_lds;                // later the results tile
  double* table = dens + region_b;                        // later data | precision
  double(*red)[W][kLanes] = (double(*)[W][kLanes])(table + region_a);
  // rows form: (PARTS, N, 64); slab form: the class's products y (N, 64), then (N, 64)
  double* sums = table + region_a + 2 * W * kLanes;
  double* weights = sums + (size_t)(ROWS ? PARTS : 2) * n_total * kLanes;   // (rows, 64)
  double* cls = weights + (size_t)a.n_weight_rows * kLanes;   // 1 / ngal_v, 1 / ngal_v^2
  const fm::Consts kc = fm::make_consts();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_gauss = NGAUSS > 0 ? NGAUSS : a.n_gauss;
  const int n_dim = a.n_dim;

  stage_math_table(table, a.math_table);
  for (int idx = threadIdx.x; idx < (ROWS ? PARTS : 2) * n_total * kLanes; idx += blockDim.x)
    sums[idx] = 0.0;
  if (ROWS)
    for (int idx = a.n_bins * DL + threadIdx.x; idx < a.dens_rows * DL; idx += blockDim.x)
      dens[idx] = 0.0;

  // ---- 1. the spline weights of the lane's draw ----
  const int64_t col = (int64_t)blockIdx.x * DL;
  const int64_t b0 = col + lane;
  const int64_t b = b0 < a.n_draws ? b0 : a.n_draws - 1;
  for (int d = 0; d < n_dim; ++d) {
    const int n = a.n_axis[d];
    const double x = a.x[b * n_dim + d];
    const double* m = a.a + a.a_offset[d] +
                      (int64_t)spline_segment(n, a.xp + a.axis_offset[d], x) * 4 * n;
    const double x2 = x * x, x3 = x2 * x;
    for (int j = wave; j < n; j += W)
      weights[(a.weight_row[d] + j) * kLanes + lane] = spline_node_weight(n, m, j, x, x2, x3);
  }
  __syncthreads();

  // ---- 2. the classes ----
  DrawParams dp = draw_params<ASSEMBIAS>(table, kc, a.theta + b * a.n_theta);
  series_setup<MODULATE>(dp, false, false);
  double ngal = 0.0;
  const int c = lane & 15, kq = lane >> 4;
  const int n_jobs = a.job_begin[a.n_members];
  for (int v = 0; v < a.n_classes; ++v) {
    const int s_begin = a.class_begin[v], s_end = a.class_begin[v + 1];
    if (ROWS) {
      __syncthreads();   // (the class before is done with the densities, red and cls)
      double sum_cen = 0.0, sum_sat = 0.0;
      jif::class_occupations<NGAUSS, ASSEMBIAS, MODULATE>(a, table, kc, dp, v, n_gauss, 0,
                                                          a.n_bins, dens, lane, wave, sum_cen,
                                                          sum_sat);
      red[0][wave][lane] = sum_cen;
      red[1][wave][lane] = sum_sat;
      __syncthreads();
      const double ngal_v = jif::class_ngal(red, lane);
      for (int s = s_begin; s < s_end; ++s)
        ngal = fma(jif::node_coef(a, weights, a.walk_node + (size_t)s * n_dim, lane), ngal_v, ngal);
      if (wave == 0) {
        cls[lane] = 1.0 / ngal_v;
        cls[kLanes + lane] = 1.0 / (ngal_v * ngal_v);
      }
      __syncthreads();
      // mode auto: pass (pair p, part, tile) of member m, at every node of the class
      for (int job = wave; job < n_jobs; job += W) {
        int m = 0;
        while (job >= a.job_begin[m + 1]) ++m;
        const int local = job - a.job_begin[m];
        const int p = local / (2 * PARTS), part = local / 2 % PARTS, sub = local % 2;
        const int n_u = a.n_u[m], up = (n_u + 1) / 2;
        const int d0 = sub * kQuadTile + 2 * c;      // the lane's two draws of the tile
        const double* dens_b = dens + (a.j_row0 + kq) * DL + d0;
        const double* dens_e = dens + a.i_row0 * DL + d0;
        const FusedPart walk = {a.part_rb0[part], a.part_cb0[part], a.part_count[part], 1, a.n_cb,
                                (unsigned)a.unit_base};
        const unsigned off_a = lane * 16 + p * 1024;
        for (int s = s_begin; s < s_end; ++s) {
          const int32_t* node = a.walk_node + (size_t)s * n_dim;
          const __amdgpu_buffer_rsrc_t rs_t = __builtin_amdgcn_make_buffer_rsrc(
              (void*)a.matrices[m][s], 0, a.table_bytes[m], kBufferFlags);
          double F[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
          if (2 * p + 1 < n_u)
            fused_quad_pass<2, DL>(rs_t, off_a, up * 1024u, dens_b, dens_e, walk, F);
          else
            fused_quad_pass<1, DL>(rs_t, off_a, up * 1024u, dens_b, dens_e, walk, F);
          const double scale0 = jif::node_coef(a, weights, node, d0) * cls[kLanes + d0];
          const double scale1 = jif::node_coef(a, weights, node, d0 + 1) * cls[kLanes + d0 + 1];
          // r = 4 (2 p + u) + l / 16, draws 2 c and 2 c + 1 of the tile
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int r = 4 * (2 * p + u) + kq;
            if (r < a.n_rows[m]) {
              f64x2* slot = (f64x2*)(sums + ((size_t)part * n_total + a.r_offset[m] + r) * kLanes +
                                     d0);
              f64x2 value = *slot;
              value.x = fma(scale0, F[u][0], value.x);
              value.y = fma(scale1, F[u][1], value.y);
              *slot = value;
            }
          }
        }
      }
      // mode cross: group g of the cross members' rows, at every node of the class
      const double inv_ngal = cls[lane];
      for (int g = (wave + W - n_jobs % W) % W;; g += W) {
        int m, r0, rows;
        if (!jif::cross_group(a, g, m, r0, rows)) break;
        const int n_r = a.n_rows[m];
        double* slot = sums + (size_t)(a.r_offset[m] + r0) * kLanes + lane;
        for (int s = s_begin; s < s_end; ++s) {
          const double scale =
              jif::node_coef(a, weights, a.walk_node + (size_t)s * n_dim, lane) * inv_ngal;
          jif::cross_group_chains(a.matrices[m][s], n_r, r0, rows, 0, a.n_bins, dens, lane,
                                  [&](int k, double sum) {
                                    slot[k * kLanes] = fma(scale, sum, slot[k * kLanes]);
                                  });
        }
      }
    } else {
      // slab form: the group's rows of y and of the accumulators belong to its wave
      double* y = sums;
      double* total = sums + (size_t)n_total * kLanes;
      for (int g = wave;; g += W) {
        int m, r0, rows;
        if (!jif::cross_group(a, g, m, r0, rows)) break;
        for (int k = 0; k < rows; ++k) y[(size_t)(a.r_offset[m] + r0 + k) * kLanes + lane] = 0.0;
      }
      double sum_cen = 0.0, sum_sat = 0.0;
      for (int slab0 = 0; slab0 < a.n_bins; slab0 += kJointInterpForwardSlab) {
        const int count = a.n_bins - slab0 < kJointInterpForwardSlab ? a.n_bins - slab0
                                                                     : kJointInterpForwardSlab;
        __syncthreads();   // (the slab before is done with the densities)
        jif::class_occupations<NGAUSS, ASSEMBIAS, MODULATE>(a, table, kc, dp, v, n_gauss, slab0,
                                                            count, dens, lane, wave, sum_cen,
                                                            sum_sat);
        __syncthreads();
        for (int g = wave;; g += W) {
          int m, r0, rows;
          if (!jif::cross_group(a, g, m, r0, rows)) break;
          const int n_r = a.n_rows[m];
          double* slot = y + (size_t)(a.r_offset[m] + r0) * kLanes + lane;
          for (int s = s_begin; s < s_end; ++s) {
            const double coef = jif::node_coef(a, weights, a.walk_node + (size_t)s * n_dim, lane);
            jif::cross_group_chains(a.matrices[m][s], n_r, r0, rows, slab0, count, dens, lane,
                                    [&](int k, double sum) {
                                      slot[k * kLanes] = fma(coef, sum, slot[k * kLanes]);
                                    });
          }
        }
      }
      red[0][wave][lane] = sum_cen;
      red[1][wave][lane] = sum_sat;
      __syncthreads();
      const double ngal_v = jif::class_ngal(red, lane);
      for (int s = s_begin; s < s_end; ++s)
        ngal = fma(jif::node_coef(a, weights, a.walk_node + (size_t)s * n_dim, lane), ngal_v, ngal);
      const double inv_ngal = 1.0 / ngal_v;
      for (int g = wave;; g += W) {
        int m, r0, rows;
        if (!jif::cross_group(a, g, m, r0, rows)) break;
        for (int k = 0; k < rows; ++k) {
          const size_t at = (size_t)(a.r_offset[m] + r0 + k) * kLanes + lane;
          total[at] = fma(y[at], inv_ngal, total[at]);
        }
      }
      __syncthreads();   // (red is read: the next class may write it)
    }
  }
  if (wave == 0 && b0 < a.n_draws) a.ngal[b0] = ngal;
  __syncthreads();       // the densities and the math table are dead: the results take their place

  // ---- 3. the parts of every row, the results ----
  if (a.chi2 != nullptr)
    for (int idx = threadIdx.x; idx < operand_doubles; idx += blockDim.x)
      table[idx] = a.chi2_data[idx];
  double(*tile)[kLanes + 1] = (double(*)[kLanes + 1])dens;
  for (int m = 0; m < a.n_members; ++m) {
    const bool is_auto = a.mode[m] == TC_MODE_AUTO;
    for (int rr = wave; rr < a.n_rows[m]; rr += W) {
      const int row = a.r_offset[m] + rr;
      // (slab form: the accumulators lie behind the class's products)
      const double* first = sums + (size_t)(ROWS ? row : n_total + row) * kLanes + lane;
      double sum = first[0];
      if (ROWS && is_auto) {
#pragma unroll
        for (int part = 1; part < PARTS; ++part) sum += first[(size_t)part * n_total * kLanes];
      }
      tile[row][lane] = sum;
    }
  }
  __syncthreads();
  joint_forward_results(tile, table, red[0], n_total, col, a.n_draws, a.xi, a.chi2);
}

}  // namespace tc
