// Steps that several kernels of kernels.hip.h share, one copy each:
//   stage_math_table  the math table into LDS: predict_cross_fused_kernel, single_draw_body,
//                     resident_ensemble_kernel;
//   tile_write_xi     the transposed write-out of a results tile: the two mode-cross one-launch
//                     kernels and finalize_body;
//   finalize_body     finalize_kernel and finalize_quad_kernel.
// A results tile is (rows, kLanes + 1) doubles, draw d of row r at [r * (kLanes + 1) + d].
// Every helper is inlined into its caller.  Which kernels keep which of these steps written out,
// and the register counts behind that: profiles/epilogue_notes.md.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fastmath.h"
#include "kernel_args.h"

namespace tc {

// The math table (fastmath.h) into LDS, 16-byte words, thread t of `threads` the words t,
// t + threads, ...; the caller's barrier follows.
__device__ __forceinline__ void stage_math_table(double* dst, const double* src,
                                                 int thread = threadIdx.x,
                                                 int threads = blockDim.x) {
  typedef double __attribute__((ext_vector_type(2))) double2v;
  const double2v* from = (const double2v*)src;
  double2v* to = (double2v*)dst;
  for (int i = thread; i < fm::kTableDoubles / 2; i += threads) to[i] = from[i];
}

// Rows [row_offset, row_offset + rows) of the first n_valid of the tile's `draws` draws to
// dst[d * stride + row]: `dst` is where draw 0 begins, `stride` its length in doubles.
__device__ __forceinline__ void tile_write_xi(const double* tile, int rows, int draws,
                                              int64_t n_valid, double* dst, int stride,
                                              int row_offset) {
  for (int idx = threadIdx.x; idx < rows * draws; idx += blockDim.x) {
    const int d = idx / rows, rr = idx % rows;
    if (d < n_valid) dst[d * stride + row_offset + rr] = tile[rr * (kLanes + 1) + d];
  }
}

// The two finalisation kernels: the number density from its parts into the norm, then the rows
// of this block kFinalizeRows at a time -- `sum(row, part, parts)`: part `part` of `parts` equal
// ranges of a row's slabs, added in slab order; few rows: several waves per row, combined in
// fixed order --, `normalise(sum, norm, poisoned)`, the results tile, and its write-out or,
// LIKELIHOOD, the likelihood of the tile (one pass, one row block: the host sees to that).
// Separated by galaxy type the reference forms every term / sum first and masks afterwards
// (tabcorr.py:653-681): with a non-finite sum some term is inf / inf = NaN and NaN x False = NaN
// reaches every component -- `poisoned`.
template <bool LIKELIHOOD, typename Args, typename Sum, typename Normalise>
__device__ __forceinline__ void finalize_body(const Args& a, Sum sum_slabs, Normalise normalise) {
  __shared__ double tile[kFinalizeRows][kLanes + 1];
  __shared__ double part_sum[16][kLanes];
  __shared__ double norm_inv[kLanes];
  // the likelihood: the data vector and the weight matrix, staged once per workgroup
  __shared__ double chi2_lds[LIKELIHOOD ? kFinalizeRows * (kFinalizeRows + 1) : 1];
  if constexpr (LIKELIHOOD) {
    if (a.chi2 != nullptr) {
      const int count = a.n_r * (a.n_r + 1);
      for (int idx = threadIdx.x; idx < count; idx += blockDim.x) chi2_lds[idx] = a.chi2_data[idx];
    }
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t col = (int64_t)blockIdx.x * kLanes;
  const int64_t n_valid = a.n_draws - col < kLanes ? a.n_draws - col : kLanes;

  if (wave == 0 && a.ngal_part == nullptr) norm_inv[lane] = 1.0;
  if (wave == 0 && a.ngal_part != nullptr) {
    double n_cen = 0.0, n_sat = 0.0;
    for (int p = 0; p < a.n_ngal_parts; ++p) {
      n_cen += a.ngal_part[((int64_t)p * 2 + 0) * a.ldb + col + lane];
      n_sat += a.ngal_part[((int64_t)p * 2 + 1) * a.ldb + col + lane];
    }
    const double total = n_cen + n_sat;
    norm_inv[lane] = a.mode == 0 ? total * total : total;
    if (lane < n_valid && blockIdx.y == 0) {
      if (a.n_comp == 1) {
        a.ngal[col + lane] = total;
      } else {
        a.ngal[2 * (col + lane)] = n_cen;
        a.ngal[2 * (col + lane) + 1] = n_sat;
      }
    }
  }
  __syncthreads();
  const double norm = norm_inv[lane];
  const bool poisoned = a.n_comp > 1 && !(fabs(norm) <= 1.79769313486231570815e308);

  const int n_rows = a.n_comp * a.n_r;
  const int n_waves = blockDim.x >> 6;
  // rows of this block (grid.y row blocks; one for large batches)
  const int rows_per_block = (n_rows + gridDim.y - 1) / gridDim.y;
  const int row_begin = blockIdx.y * rows_per_block;
  const int row_end = row_begin + rows_per_block < n_rows ? row_begin + rows_per_block : n_rows;
  for (int row0 = row_begin; row0 < row_end; row0 += kFinalizeRows) {
    const int rows = row_end - row0 < kFinalizeRows ? row_end - row0 : kFinalizeRows;
    if (rows * 2 <= n_waves) {
      // few rows (small batches, split over row blocks; an un-batched interpolator call
      // leaves ~1000 slabs per row): several waves per row, each over a contiguous range
      // of slabs, combined in fixed order
      const int parts = n_waves / rows;
      const int rr = wave / parts, part = wave % parts;
      if (rr < rows) part_sum[wave][lane] = sum_slabs(row0 + rr, part, parts);
      __syncthreads();
      if (wave < rows) {
        double sum = 0.0;
        for (int p = 0; p < parts; ++p) sum += part_sum[wave * parts + p][lane];
        tile[wave][lane] = normalise(sum, norm, poisoned);
      }
    } else {
      for (int rr = wave; rr < rows; rr += n_waves)
        tile[rr][lane] = normalise(sum_slabs(row0 + rr, 0, 1), norm, poisoned);
    }
    __syncthreads();
    if constexpr (LIKELIHOOD) {
      if (a.chi2 != nullptr) {
        // (every row of the draws is in `tile` now)  chi2 = delta^T P delta of the lane's draw:
        // wave w sums the rows i = w, w + n_waves, ... of delta_i (P delta)_i (the matrix word is
        // a broadcast), wave 0 adds the waves' sums in wave order -- as the one-launch kernels
        const double* data = chi2_lds;
        const double* matrix = chi2_lds + rows;
        double part = 0.0;
        for (int i = wave; i < rows; i += n_waves) {
          double inner = 0.0;
          for (int j = 0; j < rows; ++j)
            inner = fma(matrix[i * rows + j], tile[j][lane] - data[j], inner);
          part = fma(tile[i][lane] - data[i], inner, part);
        }
        part_sum[wave][lane] = part;
        __syncthreads();
        if (wave == 0 && lane < n_valid) {
          double total = 0.0;
          for (int w = 0; w < n_waves; ++w) total += part_sum[w][lane];
          a.chi2[col + lane] = total;
        }
        __syncthreads();
        continue;
      }
    }
    tile_write_xi(&tile[0][0], rows, kLanes, n_valid, a.xi + col * (int64_t)n_rows, n_rows, row0);
    __syncthreads();
  }
}

}  // namespace tc
