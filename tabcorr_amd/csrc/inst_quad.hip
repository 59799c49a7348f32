// Kernels of the three-kernel path (occupations, contraction, finalisation), the segment
// kernels, the interpolator's coefficients and the likelihood: their launches, in a translation
// unit of their own.
#define TC_UNIT_QUAD
#include "dispatch.h"
#include "internal.h"
#include "kernels.hip.h"

namespace tc {
namespace host {

// The occupation kernel of the three-kernel path for these flags (instances: Zheng07 family
// with ten or any number of nodes, per bin or -- ten nodes -- per group of bins, each as an
// (assembias, modulate) square; Leauthaud11, modulate or not).
int launch_occupation(const tc::OccArgs& oa, unsigned flags, int n_gauss, bool grouped,
                      int64_t grid_blocks, hipStream_t stream) {
  const dim3 grid((unsigned)grid_blocks), block(tc::kOccWaves * 64);
  const bool assembias = (flags & TC_FLAG_ASSEMBIAS) != 0;
  const bool modulate = (flags & TC_FLAG_MODULATE_WITH_CENOCC) != 0;
  auto zheng07 = [&](auto ng, auto gr) {
    return with_bools(
        [&](auto ab, auto mo) {
          hipLaunchKernelGGL((tc::occ_zheng07_kernel<ng(), ab(), mo(), gr()>), grid, block, 0,
                             stream, oa);
          return TC_OK;
        },
        assembias, modulate);
  };
  if (flags & TC_FLAG_LEAUTHAUD11)
    with_bools(
        [&](auto mo) {
          hipLaunchKernelGGL(tc::occ_leauthaud11_kernel<mo()>, grid, block, 0, stream, oa);
          return TC_OK;
        },
        modulate);
  else if (grouped)
    zheng07(int_c<10>{}, std::true_type{});
  else if (n_gauss == 10)
    zheng07(int_c<10>{}, std::false_type{});
  else
    zheng07(int_c<0>{}, std::false_type{});
  TC_HIP(hipGetLastError());
  return TC_OK;
}

// Instances: contract_quad_kernel<1 .. 5, interp>, contract_quad_f32_kernel<1 .. 4, interp>.
int launch_contract_quad(int n_u, int dtype, bool interp, const tc::QuadArgs& args, int lds_bytes,
                         hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  const dim3 grid((unsigned)((args.n_waves + tc::kQuadWavesPerBlock - 1) /
                             tc::kQuadWavesPerBlock));
  const dim3 block(64 * tc::kQuadWavesPerBlock);
  if (args.n_waves == 0) return TC_OK;
  const bool f32 = dtype == TC_DTYPE_F32;
  auto none = [&] {
    return f32 ? fail(TC_ERR_UNSUPPORTED, "no float32 kernel for %d r sub-tiles", n_u)
               : fail(TC_ERR_UNSUPPORTED, "no kernel for %d r sub-tiles", n_u);
  };
  return with_int<1, 2, 3, 4, 5>(
      n_u,
      [&](auto n) {
        return with_bools(
            [&](auto single, auto in) {
              if constexpr (single() && n() == 5) {
                return none();
              } else {
                if constexpr (single())
                  hipExtLaunchKernelGGL((tc::contract_quad_f32_kernel<n(), in()>), grid, block,
                                        lds_bytes, stream, start, stop, 0, args);
                else
                  hipExtLaunchKernelGGL((tc::contract_quad_kernel<n(), in()>), grid, block,
                                        lds_bytes, stream, start, stop, 0, args);
                TC_HIP(hipGetLastError());
                return TC_OK;
              }
            },
            f32, interp);
      },
      none);
}

int launch_finalize_quad(const tc::FinalizeQuadArgs& args, const Tuning& tuning,
                         hipStream_t stream, bool f32) {
  // geometry as launch_finalize: one block per 64 draws, small batches split the rows
  const int64_t n_tiles = args.ldb / 64;
  // (fused likelihood: 16 waves share the rows of the quadratic form -- next to a
  // contraction every vector instruction of a wave waits for a matrix instruction)
  const int threads = tuning.finalize_threads > 0 ? tuning.finalize_threads
                      : n_tiles < 128 || args.chi2 != nullptr ? 1024 : 256;
  const int n_rows = args.n_comp * args.n_r;
  // (many rows -- hundreds of r values -- are split over row blocks of at least 16 rows until
  // the grid has ~2048 blocks: one block per draw tile walked 760 rows serially, 2.4 ms)
  const int row_blocks =
      args.chi2 != nullptr
          ? 1   // (the fused likelihood needs every row of a draw in one workgroup)
          : std::min(n_rows, tuning.finalize_row_blocks > 0
                                 ? tuning.finalize_row_blocks
                                 : n_tiles < 128
                                       ? (int)std::max<int64_t>(1, 512 / n_tiles)
                                       : (int)std::max<int64_t>(
                                             1, std::min<int64_t>(n_rows / 16, 2048 / n_tiles)));
  if (f32)
    hipLaunchKernelGGL((tc::finalize_quad_kernel<float, tc::kQuadTileF32>),
                       dim3((unsigned)n_tiles, (unsigned)row_blocks), dim3(threads), 0, stream,
                       args);
  else
    hipLaunchKernelGGL((tc::finalize_quad_kernel<double, tc::kQuadTile>),
                       dim3((unsigned)n_tiles, (unsigned)row_blocks), dim3(threads), 0, stream,
                       args);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

// Instances: contract_mfma_kernel<r tile, several tables> for r tiles of 4, 8, ..., 32.
int launch_contract_rt(int rt, int device, dim3 grid, dim3 block, int lds, hipStream_t stream,
                       const tc::ContractArgs& args, hipEvent_t start, hipEvent_t stop) {
  return with_int<4, 8, 12, 16, 20, 24, 28, 32>(
      rt,
      [&](auto n) {
        return with_bools(
            [&](auto tables) {
              const auto kernel = tc::contract_mfma_kernel<n(), tables()>;
              if (lds > 64 * 1024) {
                const int status = ensure_lds_limit((const void*)kernel, device, lds);
                if (status != TC_OK) return status;
              }
              hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, start, stop, 0, args);
              TC_HIP(hipGetLastError());
              return TC_OK;
            },
            args.n_tables > 0);
      },
      [&] { return fail(TC_ERR_UNSUPPORTED, "no kernel for r tile %d", rt); });
}

// float32 variant (one kernel for every r tile: always 32 wide)
int launch_contract_f32(int device, dim3 grid, dim3 block, int lds, hipStream_t stream,
                        const tc::ContractArgs& args, hipEvent_t start, hipEvent_t stop) {
  return with_bools(
      [&](auto tables) {
        const auto kernel = tc::contract_f32_kernel<tables()>;
        if (lds > 64 * 1024) {
          const int status = ensure_lds_limit((const void*)kernel, device, lds);
          if (status != TC_OK) return status;
        }
        hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, start, stop, 0, args);
        TC_HIP(hipGetLastError());
        return TC_OK;
      },
      args.n_tables > 0);
}

int launch_finalize(const FinalizeArgs& args, const Tuning& tuning, hipStream_t stream) {
  // one block per draw tile; a wave sums one (component, r) row at a time over the slabs,
  // so small batches (few blocks, latency-bound) get 16 waves per block instead of 4
  // and split the rows over several blocks (up to ~512 blocks in all)
  const int64_t n_tiles = args.ldb / 64;
  const int threads =
      tuning.finalize_threads > 0 ? tuning.finalize_threads : n_tiles < 128 ? 1024 : 256;
  const int n_rows = args.n_comp * args.n_r;
  const int row_blocks = std::min(
      n_rows, tuning.finalize_row_blocks > 0
                  ? tuning.finalize_row_blocks
                  : n_tiles < 128 ? (int)std::max<int64_t>(1, 512 / n_tiles) : 1);
  hipLaunchKernelGGL(tc::finalize_kernel, dim3((unsigned)n_tiles, (unsigned)row_blocks),
                     dim3(threads), 0, stream, args);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

int launch_interp_coef(const InterpArgs& args, hipStream_t stream) {
  if (args.n_draws <= 16 && args.n_tables <= tc::kCoefSmallTables)
    hipLaunchKernelGGL(tc::interp_coef_small_kernel, dim3((unsigned)args.n_draws), dim3(64),
                       0, stream, args);
  else
    hipLaunchKernelGGL(tc::interp_coef_kernel, dim3((unsigned)(args.ldb / 64)), dim3(64), 0,
                       stream, args);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

int launch_chi2(const double* xi, int64_t n_draws, int n_r, const double* data,
                const double* precision, double* chi2, hipStream_t stream) {
  // draws per workgroup: 8 unless their deviations would not fit the LDS budget
  const size_t row = (size_t)n_r * sizeof(double);
  TC_CHECK(n_r >= 1 && row <= (size_t)tc::kChi2LdsBytes, "chi2: too many r bins");
  const int per_block =
      (int)std::min<size_t>(tc::kChi2DrawsPerBlock, (size_t)tc::kChi2LdsBytes / row);
  const size_t lds =
      per_block * row + (n_r <= tc::kChi2LdsMatrix ? (size_t)n_r * row : (size_t)0);
  hipLaunchKernelGGL(tc::chi2_kernel, dim3((unsigned)((n_draws + per_block - 1) / per_block)),
                     dim3(32 * per_block), lds, stream, xi, n_draws, n_r, data, precision,
                     chi2);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

int launch_occ_from_array_kernel(const double* occupation_device, int64_t n_draws, int64_t ldb,
                                 int n_bins, int n_central, const double* n_h,
                                 const int32_t* perm, double* nbuf, double* ngal2, float* nbuf32,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(tc::occ_from_array_kernel, dim3((unsigned)((ldb + 255) / 256)),
                     dim3(256), 0, stream, occupation_device, n_draws, ldb, n_bins, n_central,
                     n_h, perm, nbuf, ngal2, nbuf32);
  TC_HIP(hipGetLastError());
  return TC_OK;
}

}  // namespace host
}  // namespace tc

// ---- TEST INFRASTRUCTURE (include/tabcorr_amd_testing.h: tc_debug_fastmath_device) ------------
//
// The table-driven functions of fastmath.h and series::sat::reciprocal as the DEVICE compiles
// them (frexp_mant / frexp_exp / ubfe in log2, the hardware reciprocal with two Newton steps,
// the device's ldexp and FMA contraction), with the table staged in LDS as occ_zheng07_kernel
// stages it.  Never called by the product.
namespace tc {

__global__ __launch_bounds__(256) void debug_fastmath_kernel(int kind, int64_t n,
                                                             const double* math_table,
                                                             const double* x, double* y) {
  __shared__ __attribute__((aligned(16))) double table[fm::kTableDoubles];
  const fm::Consts kc = fm::make_consts();
  {
    typedef double __attribute__((ext_vector_type(2))) double2v;
    const double2v* src = (const double2v*)math_table;
    double2v* dst = (double2v*)table;
    for (int i = threadIdx.x; i < fm::kTableDoubles / 2; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = x[i];
    double out = 0.0, gauss = 0.0;
    switch (kind) {
      case 0: out = fm::erf_fast(table, kc, v); break;
      case 1: out = fm::log2_fast(table, kc, v); break;
      case 2: out = fm::exp2_fast(table, kc, v); break;
      case 3: out = fm::exp10_fast(table, kc, v); break;
      case 4: out = fm::erf_gauss_fast(table, kc, v, &gauss); break;
      case 5:
        (void)fm::erf_gauss_fast(table, kc, v, &gauss);
        out = gauss;
        break;
      case 6: out = fm::log_fast(table, kc, v); break;
      case 7:
        (void)fm::erf_gauss_fast(table, kc, v, &gauss);
        if (fabs(v) >= 6.0) gauss = 1.1283791670955125739 * exp(-v * v);
        out = fm::half_erfc_from_gauss(fabs(v), gauss);
        break;
      case 8: out = series::sat::reciprocal(v); break;
      default: out = fm::exp2_fast(table, kc, v, false); break;      // 9: keep == false
    }
    y[i] = out;
  }
}

}  // namespace tc

extern "C" int tc_debug_fastmath_device(int kind, int64_t n, const double* x, double* y) {
  using tc::host::fail;
  TC_CHECK(kind >= 0 && kind <= 9 && n >= 0 && (n == 0 || (x && y)), "invalid arguments");
  if (n == 0) return TC_OK;
  std::vector<double> table(tc::fm::kTableDoubles);
  tc::fm::build_tables(table.data());
  const size_t bytes = (size_t)n * sizeof(double), table_bytes = table.size() * sizeof(double);
  void *d_table = nullptr, *d_x = nullptr, *d_y = nullptr;
  auto run = [&]() -> int {
    TC_HIP(hipMalloc(&d_table, table_bytes));
    TC_HIP(hipMalloc(&d_x, bytes));
    TC_HIP(hipMalloc(&d_y, bytes));
    TC_HIP(hipMemcpy(d_table, table.data(), table_bytes, hipMemcpyHostToDevice));
    TC_HIP(hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(tc::debug_fastmath_kernel, dim3(blocks), dim3(256), 0, nullptr, kind, n,
                       (const double*)d_table, (const double*)d_x, (double*)d_y);
    TC_HIP(hipGetLastError());
    TC_HIP(hipDeviceSynchronize());
    TC_HIP(hipMemcpy(y, d_y, bytes, hipMemcpyDeviceToHost));
    return TC_OK;
  };
  const int status = run();
  for (void* p : {d_table, d_x, d_y})
    if (p != nullptr) (void)hipFree(p);
  return status;
}
