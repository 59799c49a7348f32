// Table handle of the C ABI (include/tabcorr_amd.h): upload and re-layout of one
// tabulated correlation matrix, the batched predict / chi2 / occupation entry points,
// and the measurement hooks bench.py uses.
#include <cmath>

#include "internal.h"

using namespace tc::host;

extern "C" {

int tc_table_create(int mode, int n_bins, int n_r, int64_t n_pairs,
                    const void* tpcf_matrix, int matrix_dtype, const double* n_h,
                    const double* log_min, const double* log_max,
                    const double* percentile, const double* dist_index,
                    const uint8_t* is_central, int compute_dtype, tc_table** out) {
  TC_CHECK(out != nullptr, "table output pointer is NULL");
  *out = nullptr;
  TC_CHECK(mode == TC_MODE_AUTO || mode == TC_MODE_CROSS, "invalid mode %d", mode);
  TC_CHECK(n_bins >= 1 && n_bins < (1 << 20), "invalid number of bins %d", n_bins);
  TC_CHECK(n_r >= 1, "invalid number of correlation function bins %d", n_r);
  const int64_t expect =
      mode == TC_MODE_AUTO ? (int64_t)n_bins * (n_bins + 1) / 2 : n_bins;
  TC_CHECK(n_pairs == expect,
           "tpcf_matrix has %lld columns but %d bins in mode '%s' need %lld",
           (long long)n_pairs, n_bins, mode == TC_MODE_AUTO ? "auto" : "cross",
           (long long)expect);
  TC_CHECK(n_pairs < (1LL << 31), "too many pair columns");
  TC_CHECK(tpcf_matrix && n_h && log_min && log_max && percentile && is_central,
           "NULL input array");
  TC_CHECK(matrix_dtype == TC_DTYPE_F64 || matrix_dtype == TC_DTYPE_F32,
           "invalid matrix dtype");
  TC_CHECK(compute_dtype == TC_DTYPE_F64 || compute_dtype == TC_DTYPE_F32,
           "invalid compute dtype");
  TC_CHECK(compute_dtype != TC_DTYPE_F32 || n_bins < 65535,
           "too many bins for the float32 variant");

  // (tc_table_destroy releases whatever exists when a later step fails)
  struct Destroy {
    void operator()(tc_table* table) const { tc_table_destroy(table); }
  };
  std::unique_ptr<tc_table, Destroy> t(new tc_table);
  TC_HIP(hipGetDevice(&t->device));
  {
    hipDeviceProp_t prop;
    TC_HIP(hipGetDeviceProperties(&prop, t->device));
    t->n_cus = std::max(1, prop.multiProcessorCount);
    // MI355X: 8 accelerator complexes (XCDs) of 32 CUs; a compute partition exposes fewer
    t->n_xcds = std::max(1, t->n_cus / 32);
  }
  t->tuning.load();
  t->mode = mode;
  t->n_bins = n_bins;
  t->n_r = n_r;
  t->n_pairs = n_pairs;
  t->compute_dtype = compute_dtype;
  t->legacy = dist_index == nullptr;
  // r tiling: at most 32 accumulators per lane, a multiple of 4 so that a block
  // of at most 4 entries fills whole 128-byte lines (float64); tiles of exactly 32 r
  // values and blocks of 8 entries for the float32 MFMA kernel.
  const int max_rt = 32;
  t->n_rtiles = (n_r + max_rt - 1) / max_rt;
  if (compute_dtype == TC_DTYPE_F32) {
    t->rt = tc::kF32Tile;
    tc::build_plan(mode, n_bins, is_central, tc::kF32Block,
                   env_int("TC_ROW_BUDGET_F32", 128), t->plan);   // (developer builds)
  } else {
    int rt = (n_r + t->n_rtiles - 1) / t->n_rtiles;
    t->rt = (rt + 3) / 4 * 4;
    // LDS rows a workgroup may stage: half the bins (one triangle or one column block
    // of the cen-sat rectangle) plus a few rows, within 28..66 KB
    const int budget = std::max(56, std::min(128, n_bins / 2 + 6));
    tc::build_plan(mode, n_bins, is_central, tc::kF64Block,
                   env_int("TC_ROW_BUDGET", budget), t->plan);
  }

  for (int g = 0; g < n_bins; ++g) {
    const int src = t->plan.perm[g];
    t->n_h.push_back(n_h[src]);
    t->log_min.push_back(log_min[src]);
    t->log_max.push_back(log_max[src]);
    t->percentile.push_back(percentile[src]);
    t->dist_index.push_back(dist_index ? dist_index[src] : -1.0);
  }

  const int rt = t->rt;
  const int64_t n_positions = t->plan.n_positions;
  const size_t count = (size_t)t->n_rtiles * n_positions * rt;
  auto source = [&](int r, int64_t column) {
    return matrix_dtype == TC_DTYPE_F64
               ? ((const double*)tpcf_matrix)[(size_t)r * n_pairs + column]
               : (double)((const float*)tpcf_matrix)[(size_t)r * n_pairs + column];
  };
  std::vector<double> tmp64;
  std::vector<float> tmp32;
  std::vector<int32_t> pos_ij;
  if (compute_dtype == TC_DTYPE_F64) {
    // Re-laid-out matrix, per r tile and position, with the pair prefactor
    // (tabcorr.py:638-642) folded in (a multiplication by 2 is exact) and zero
    // rows at the padding positions.
    t->table_bytes = count * sizeof(double);
    tmp64.assign(count, 0.0);
    for (int r = 0; r < n_r; ++r) {
      const int tile = r / rt, rr = r % rt;
      for (int64_t q = 0; q < n_positions; ++q) {
        const int64_t column = t->plan.column[q];
        if (column < 0) continue;
        // blocks of 8 positions (two steps of 4) as [r sub-tile of 4][position in step]
        // [r in sub-tile][step] (kernels.hip.h)
        const size_t index = ((size_t)tile * n_positions + q / 8 * 8) * rt +
                             (((rr / 4) * 16 + (q % 4) * 4 + rr % 4) * 2 + (q / 4) % 2);
        tmp64[index] = source(r, column) * t->plan.prefactor[q];
      }
    }
    // LDS row offsets per pair of steps and position in step: (i, j of step 0, i, j of
    // step 1) * 512 bytes
    pos_ij.assign((size_t)n_positions * 2, 0);
    for (int64_t q = 0; q < n_positions; ++q) {
      const size_t slot = ((size_t)(q / 8) * 4 + q % 4) * 4 + ((q / 4) % 2) * 2;
      pos_ij[slot] = std::max(t->plan.pos_i[q], 0) * 512;
      pos_ij[slot + 1] = t->plan.pos_j[q] * 512;
    }
  } else {
    // float32 MFMA layout: [r tile][block of 8 positions][k][r][k-step] (kernels.hip.h)
    t->table_bytes = count * sizeof(float);
    tmp32.assign(count, 0.0f);
    for (int r = 0; r < n_r; ++r) {
      const int tile = r / rt, rr = r % rt;
      for (int64_t q = 0; q < n_positions; ++q) {
        const int64_t column = t->plan.column[q];
        if (column < 0) continue;
        const int64_t block = q / 8;
        const int p = (int)(q % 8) / 2, k = (int)(q % 2);
        tmp32[((size_t)tile * n_positions + block * 8) * rt + (k * 32 + rr) * 4 + p] =
            (float)(source(r, column) * t->plan.prefactor[q]);
      }
    }
    pos_ij.assign((size_t)n_positions, 0);
    for (int64_t q = 0; q < n_positions; ++q) {
      const int64_t block = q / 8;
      const int p = (int)(q % 8) / 2, k = (int)(q % 2);
      const int i = t->plan.pos_i[q] < 0 ? 0 : t->plan.pos_i[q];
      pos_ij[(size_t)block * 8 + k * 4 + p] = (i << 16) | t->plan.pos_j[q];
    }
  }
  if (mode == TC_MODE_CROSS && compute_dtype == TC_DTYPE_F64 &&
      (int64_t)n_r + 1 <= tc::kCrossMaxRows) {
    t->cross_host.resize((size_t)n_bins * n_r);
    for (int g = 0; g < n_bins; ++g)
      for (int r = 0; r < n_r; ++r)
        t->cross_host[(size_t)g * n_r + r] = source(r, t->plan.perm[g]);
  }
  // (streams of the lanes in use; tc_table_set_option "lanes" creates further ones)
  t->n_lanes = std::max(1, std::min(t->tuning.lanes, (int)tc_table::kMaxLanes));
  {
    hipStream_t streams[tc_table::kMaxLanes] = {};
    const int created = create_lane_streams(t->n_lanes, streams);
    for (int l = 0; l < t->n_lanes; ++l) t->lanes[l].stream = streams[l];
    if (created != TC_OK) return created;
    for (int l = 0; l < t->n_lanes; ++l)
      TC_HIP(hipEventCreateWithFlags(&t->lanes[l].finished, hipEventDisableTiming));
  }
  t->stream = t->lanes[0].stream;
  TC_HIP(hipEventCreate(&t->ev_begin));
  TC_HIP(hipEventCreate(&t->ev_end));
  int status = compute_dtype == TC_DTYPE_F64 ? upload(tmp64, &t->d_table)
                                             : upload(tmp32, &t->d_table);
  if (status == TC_OK && compute_dtype == TC_DTYPE_F32)
    status = upload(pos_ij, &t->d_pos_ij);
  if (status == TC_OK && compute_dtype == TC_DTYPE_F64)
    status = upload(pos_ij, &t->d_pos_off);
  if (status == TC_OK) status = upload(t->n_h, &t->d_n_h);
  if (status == TC_OK) status = upload(t->percentile, &t->d_percentile);
  if (status == TC_OK) status = upload(t->plan.perm, &t->d_perm);
  tc::find_node_groups(n_bins, t->plan.n_central, t->log_min.data(), t->log_max.data(),
                       t->node_groups);
  t->grouped = t->node_groups.largest > 1;
  if (status == TC_OK) status = upload(t->node_groups.begin, &t->d_group_begin);
  if (status == TC_OK) status = upload(t->node_groups.member, &t->d_group_member);
  {
    std::vector<double> n_h_m, percentile_m;
    for (int32_t g : t->node_groups.member) {
      n_h_m.push_back(t->n_h[g]);
      percentile_m.push_back(t->percentile[g]);
    }
    if (status == TC_OK) status = upload(n_h_m, &t->d_group_n_h);
    if (status == TC_OK) status = upload(percentile_m, &t->d_group_percentile);
  }
  if (status == TC_OK) {
    std::vector<double> math_table(tc::fm::kTableDoubles);
    tc::fm::build_tables(math_table.data());
    status = upload(math_table, &t->d_math_table);
  }
  // The quadratic-form kernel serves mode auto in float64 up to 256 MB of matrix.  While the
  // matrix fits an L2 (cfg2 0.8 MB, cfg3 3.2 MB) the shares walk it once per tile of 32 draws;
  // larger ones are walked r tile by r tile by all waves (hostmath.h: kQuadRtileMajor),
  // interpolators table by table, and matrices far beyond the L2s (BASELINE configs[4] in
  // float64: 38 r tiles of 4 MB) unit-synchronously: the waves of an XCD read the same units at
  // the same time (kQuadUnitSync: 4.40 ms per 10^4 draws against 4.76 for the segment kernel,
  // whose workgroups share their slice through LDS, and 7.0-7.3 in the other orders).
  const tc::QuadTiling quad_tiling = tc::quad_tiling(n_r);
  const double quad_blocks = (n_bins / 4.0 + 1.0) * (n_bins / 4.0 + 2.0) / 2.0;
  const double quad_bytes =
      quad_blocks * ((quad_tiling.n_u + 1) / 2) * 1024.0 * quad_tiling.n_rtiles;
  // float32: r tiles of 16 values, 1 KB per unit; an r tile's slice must stay in an L2
  // (r-tile-major order): up to 3 MB per r tile, i.e. about 300 bins
  const tc::QuadTiling quad_tiling_f32 = tc::quad_tiling_f32(n_r);
  const bool quad_f32 = compute_dtype == TC_DTYPE_F32 && quad_blocks * 1024.0 <= 3.0 * 1024 * 1024;
  if (status == TC_OK && mode == TC_MODE_AUTO &&
      ((compute_dtype == TC_DTYPE_F64 && quad_bytes <= 256.0 * 1024 * 1024) || quad_f32)) {
    // quadratic-form kernel: the matrix by galaxy type and, when the centrals do not fill
    // whole 4 x 4 blocks, the unpadded triangle for the total prediction
    t->quad = true;
    t->quad_tiling = quad_f32 ? quad_tiling_f32 : quad_tiling;
    status = build_quad_table(t.get(), true, tpcf_matrix, matrix_dtype, &t->quad_by_type);
    const int n_central = t->plan.n_central;
    // (... and for every float64 table with a single r tile: predict_fused_kernel walks the
    // whole triangle as one component)
    // (only where that kernel can ever take the table -- hostmath.cpp: choose_fused_form --: up to
    // 20 r values, up to 248 bins; a second copy of the matrix otherwise serves nobody)
    const bool fusable = !quad_f32 && quad_tiling.n_rtiles == 1 && n_r <= 20 && n_bins <= 248;
    if (status == TC_OK && ((n_central % 4 != 0 && n_central < n_bins) || fusable))
      status = build_quad_table(t.get(), false, tpcf_matrix, matrix_dtype, &t->quad_total);
  }
  if (status != TC_OK) return status;
  *out = t.release();
  return TC_OK;
}

int tc_table_destroy(tc_table* t) {
  if (t == nullptr) return TC_OK;
  (void)hipSetDevice(t->device);
  (void)resident_stop(t);
  if (t->resident.stream) (void)hipStreamDestroy(t->resident.stream);
  t->resident.mailbox.release();
  t->resident.ens_mailbox.release();
  t->resident.ens_out.release();
  t->resident.ens_device.release();
  t->resident.ens_aperture.release();
  t->resident.single_aperture.release();
  t->resident.ws.buffer.release();
  for (tc_table::Lane& lane : t->lanes)
    if (lane.stream) (void)hipStreamSynchronize(lane.stream);
  for (void* p : {t->d_table, t->d_n_h, t->d_percentile, t->d_perm, t->d_math_table,
                  t->d_pos_ij, t->d_pos_off, t->d_group_begin, t->d_group_member,
                  t->d_group_n_h, t->d_group_percentile})
    if (p) (void)hipFree(p);
  for (auto& kv : t->quadrature)
    for (void* p : {kv.second.log_m, kv.second.m, kv.second.weight, kv.second.group_log_m,
                    kv.second.group_m, kv.second.group_weight, kv.second.series,
                    kv.second.series_thr, kv.second.group_series, kv.second.group_series_thr,
                    kv.second.sat_series, kv.second.sat_series_thr, kv.second.group_sat_series,
                    kv.second.group_sat_series_thr, kv.second.group_records, kv.second.sat_records, kv.second.cen_records})
      if (p) (void)hipFree(p);
  for (auto& kv : t->chunkings)
    for (void* p : {kv.second->chunks, kv.second->groups})
      if (p) (void)hipFree(p);
  t->quad_by_type.release();
  t->quad_total.release();
  t->cross_fused.release();
  t->cross_fused_wide.release();
  t->grad.release();
  for (DeviceBuffer* b : {&t->theta, &t->out_ngal, &t->out_xi, &t->occupation,
                          &t->trace, &t->wave_trace, &t->chi2.buffer})
    b->release();
  for (tc_table::Lane& lane : t->lanes) {
    lane.nbuf.release();
    lane.ngal2.release();
    lane.partial.release();
    lane.xi.release();
    lane.nbuf32.release();
    lane.in_theta.release();
    lane.out.release();
    lane.cross_counters.release();
    if (lane.finished) (void)hipEventDestroy(lane.finished);
  }
  t->tickets.release();
  t->h_in.release();
  t->h_out.release();
  t->single_ws.buffer.release();
  for (auto& ev : t->kernel_events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  for (hipEvent_t event : t->chunk_events) (void)hipEventDestroy(event);
  if (t->ev_begin) (void)hipEventDestroy(t->ev_begin);
  if (t->ev_end) (void)hipEventDestroy(t->ev_end);
  for (tc_table::Lane& lane : t->lanes)
    if (lane.stream) (void)hipStreamDestroy(lane.stream);
  delete t;
  return TC_OK;
}

int tc_table_synchronize(tc_table* t) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  for (tc_table::Lane& lane : t->lanes)
    if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
  return TC_OK;
}

int tc_table_info(const tc_table* t, int* mode, int* n_bins, int* n_r,
                  int64_t* n_pairs, int* n_components, int64_t* device_bytes) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  if (mode) *mode = t->mode;
  if (n_bins) *n_bins = t->n_bins;
  if (n_r) *n_r = t->n_r;
  if (n_pairs) *n_pairs = t->n_pairs;
  if (n_components) *n_components = t->plan.n_components;
  if (device_bytes) *device_bytes = (int64_t)t->table_bytes;
  return TC_OK;
}

}  // extern "C"

namespace {
int autotune(tc_table* t, unsigned flags);

// The built-in estimate of which form serves a batch (hostmath.cpp: choose_fused_form) was fitted on
// a handful of table shapes and is up to 1.4 x behind the best form elsewhere (VERDICT r04 item
// 5).  So a handle that sees a LOOP of pipelined or asynchronous calls measures: the
// autotune_after-th such call with one combination of flags runs option "autotune" for it.
int maybe_autotune(tc_table* t, const Call& call, int n_gauss, unsigned flags) {
  // (the chunks of a synchronous call come with their form: no measurement inside one)
  if (t->autotuning || t->tuning.autotune_after <= 0 || t->tuning.deterministic != 0 ||
      n_gauss != 10 || t->tuning.fused != 1 ||
      call.fused_min_draws != 0 || call.fused_draws != 0 || t->tuning.fused_waves != 0)
    return TC_OK;
  const bool pipelined = call.async || (!call.pinned && t->tuning.pipeline && t->n_lanes > 1);
  // (only where the one-launch forms can serve the table at all)
  if (!pipelined || !t->quad || t->compute_dtype != TC_DTYPE_F64 || t->mode != TC_MODE_AUTO ||
      t->quad_tiling.n_rtiles != 1 || t->n_r > 20 || call.chain || t->tuning.trace ||
      call.chi2_out != nullptr)
    return TC_OK;
  const unsigned key = flags & (TC_FLAG_SEPARATE_GAL_TYPE | TC_FLAG_MODULATE_WITH_CENOCC |
                                TC_FLAG_ASSEMBIAS | TC_FLAG_LEAUTHAUD11);
  if (t->autotuned.count(key) != 0) return TC_OK;
  if (++t->pipelined_calls[key] < t->tuning.autotune_after) return TC_OK;
  t->pipelined_calls[key] = 0;
  // (the measurement makes device-pointer calls of its own, on the lanes of the rotation)
  t->autotuning = true;
  const int status = autotune(t, key);
  t->autotuning = false;
  if (status != TC_OK) {
    // (a table the measurement cannot serve: keep the estimate, do not try again)
    t->tuning.autotune_after = 0;
    (void)tc_table_synchronize(t);
  }
  return TC_OK;
}

// A prediction of n_draws > 0 draws on device pointers as `call` describes it (the arguments
// are checked): what tc_predict_zheng07_batch_device does, and every host-array and
// asynchronous entry point underneath.  *chi2_written: the form that ran wrote the call's
// likelihood (call.chi2_out) itself and left xi alone.
int predict_device(tc_table* t, const Call& call, const double* theta_device, int n_theta,
                   int64_t n_draws, int n_gauss, unsigned flags, double* ngal_device,
                   double* xi_device, bool* chi2_written = nullptr) {
  TC_HIP(hipSetDevice(t->device));
  int status = TC_OK;
  if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  const bool separate = (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0;
  const int n_comp = separate ? t->plan.n_components : 1;
  // a loop of pipelined / asynchronous calls: its autotune_after-th call measures which form
  // serves which batch size on this table (about half a second, once per combination of flags)
  if ((status = maybe_autotune(t, call, n_gauss, flags)) != TC_OK) return status;
  t->cur = call.lane;
  tc_table::Lane& lane = t->lanes[call.lane];
  const int64_t slab = max_slab(t);
  for (int64_t begin = 0; begin < n_draws; begin += slab) {
    const int64_t n = std::min(slab, n_draws - begin);
    const int64_t ldb = (n + 63) / 64 * 64;
    if (t->mode == TC_MODE_CROSS && !t->cross_host.empty() && t->tuning.fused != 0) {
      // mode cross: one launch per batch where it pays (launch.hip)
      tc_table* self = t;
      const CrossFused& cf = *choose_cross_fused(&self, 1, &t->cross_fused, &t->cross_fused_wide,
                                                 n, flags, &status);
      if (status != TC_OK) return status;
      if (cross_fused_eligible(t, call, cf, n, n_gauss, flags)) {
        status = run_cross_fused(t, call, cf, nullptr, theta_device + begin * n_theta,
                                 n_theta, n, flags, ngal_device + begin * (separate ? 2 : 1),
                                 xi_device + begin * n_comp * t->n_r, lane.stream,
                                 &lane.partial, &lane.cross_counters, chi2_written);
        if (status != TC_OK) return status;
        t->prev = call.pinned ? -1 : call.lane;
        continue;
      }
    }
    const tc::FusedForm form = tc::choose_fused_form(fused_query(t, call, n, n_gauss, flags));
    if (form.waves != 0) {
      status = run_fused(t, call, form, theta_device + begin * n_theta, n_theta, n, n_gauss,
                         flags, ngal_device + begin * (separate ? 2 : 1),
                         xi_device + begin * n_comp * t->n_r, chi2_written);
      if (status != TC_OK) return status;
      continue;
    }
    status = run_occupation(t, call, theta_device + begin * n_theta, n_theta, n, ldb,
                            n_gauss, flags, nullptr);
    if (status != TC_OK) return status;
    status = run_contraction(t, call, n, ldb, flags,
                             ngal_device + begin * (separate ? 2 : 1),
                             xi_device + begin * n_comp * t->n_r, chi2_written);
    if (status != TC_OK) return status;
  }
  return TC_OK;
}
}  // namespace

extern "C" {

int tc_predict_zheng07_batch_device(tc_table* t, const double* theta_device,
                                    int n_theta, int64_t n_draws, int n_gauss,
                                    unsigned flags, double* ngal_device,
                                    double* xi_device) {
  int status = check_predict_args(t, theta_device, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(ngal_device && xi_device, "output pointer is NULL");
  return predict_device(t, make_call(t, /*pinned=*/false), theta_device, n_theta, n_draws,
                        n_gauss, flags, ngal_device, xi_device);
}

}  // extern "C"

namespace tc {
namespace host {

// Host -> device copy of a small input through the pinned staging buffer.
int copy_in(PinnedBuffer* stage, void* device, const void* host, size_t bytes,
            hipStream_t stream) {
  Range range("upload");
  if (bytes <= stage_limit() && stage->reserve(bytes) == TC_OK) {
    memcpy(stage->ptr, host, bytes);
    host = stage->ptr;
  }
  TC_HIP(hipMemcpyAsync(device, host, bytes, hipMemcpyHostToDevice, stream));
  return TC_OK;
}

// Device -> host copy of [ngal | xi], synchronising the stream.
int copy_out(PinnedBuffer* stage, double* ngal, size_t ngal_count, const void* d_ngal,
             double* xi, size_t xi_count, const void* d_xi, hipStream_t stream) {
  Range range("download");
  const size_t bytes = (ngal_count + xi_count) * sizeof(double);
  if (bytes <= stage_limit() && stage->reserve(bytes) == TC_OK) {
    double* h = (double*)stage->ptr;
    TC_HIP(hipMemcpyAsync(h, d_ngal, ngal_count * 8, hipMemcpyDeviceToHost, stream));
    TC_HIP(hipMemcpyAsync(h + ngal_count, d_xi, xi_count * 8, hipMemcpyDeviceToHost,
                          stream));
    TC_HIP(hipStreamSynchronize(stream));
    memcpy(ngal, h, ngal_count * 8);
    parallel_copy(xi, h + ngal_count, xi_count * 8);
    return TC_OK;
  }
  TC_HIP(hipMemcpyAsync(ngal, d_ngal, ngal_count * 8, hipMemcpyDeviceToHost, stream));
  TC_HIP(hipMemcpyAsync(xi, d_xi, xi_count * 8, hipMemcpyDeviceToHost, stream));
  TC_HIP(hipStreamSynchronize(stream));
  return TC_OK;
}

}  // namespace host
}  // namespace tc

namespace {
long long monotonic_ns() {
  timespec now{};
  clock_gettime(CLOCK_MONOTONIC, &now);
  return (long long)now.tv_sec * 1000000000LL + now.tv_nsec;
}

// Should this un-batched call go to the resident kernel although nobody asked for it?  From the
// auto_streak_min-th call on that follows its predecessor within auto_gap_us, unless the mode
// is backing off.
bool resident_auto_wants(tc_table* t) {
  tc_table::Resident& r = t->resident;
  const long long now = monotonic_ns();
  const bool close = r.auto_last_ns != 0 && now - r.auto_last_ns < (long long)r.auto_gap_us * 1000;
  r.auto_streak = close ? std::min(r.auto_streak + 1, 1 << 20) : 0;
  if (r.auto_backoff > 0) {
    --r.auto_backoff;
    return false;
  }
  // (a neighbour's resident kernel is running: this process is in a loop of un-batched calls,
  // and a launch of this handle might queue behind that kernel -- launch.hip)
  if (other_resident_running(t)) return true;
  return r.auto_streak >= r.auto_streak_min;
}

// Bookkeeping behind a call the automatic mode served: a window of 32 calls of which more than
// a quarter found the kernel gone ends the mode for auto_backoff_calls calls.
void resident_auto_served(tc_table* t, bool relaunched) {
  tc_table::Resident& r = t->resident;
  r.auto_last_ns = monotonic_ns();
  r.auto_relaunches += relaunched ? 1 : 0;
  if (++r.auto_window < 32) return;
  if (r.auto_relaunches > 8) {
    r.auto_backoff = r.auto_backoff_calls;
    r.auto_streak = 0;
    (void)resident_stop(t);
  }
  r.auto_window = r.auto_relaunches = 0;
}

// Nobody asked for the resident kernel: whatever went wrong with it (it keeps leaving before it
// answers, its mailbox or aperture cannot be allocated, ...) is not the caller's business.  Stop
// it, stay away from it for a while -- for good after three such failures -- and let the caller
// serve THIS call by a launch.
void resident_auto_failed(tc_table* t) {
  (void)resident_stop(t);
  (void)hipGetLastError();
  tc_table::Resident& r = t->resident;
  r.auto_backoff = r.auto_backoff_calls;
  r.auto_streak = r.auto_window = r.auto_relaunches = 0;
  if (++r.auto_failures >= 3) r.auto_mode = false;
}
}  // namespace

extern "C" {

int tc_predict_zheng07_many(tc_table* t, const double* theta, int n_theta, int n_walkers,
                            int n_gauss, unsigned flags, double* ngal, double* xi) {
  int status = check_predict_args(t, theta, n_theta, n_walkers, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_walkers == 0) return TC_OK;
  TC_CHECK(ngal && xi, "output pointer is NULL");
  // (option "deterministic" = 2: the batched path's one-launch form, whatever the batch size)
  if (batch_invariant_form(t, n_gauss, flags))
    return tc_predict_zheng07_batch(t, theta, n_theta, n_walkers, n_gauss, flags, ngal, xi);
  if (n_walkers > kSingleMaxWalkers || !single_draw_eligible(t, 1, n_gauss, flags)) {
    // (separated by galaxy type, several r tiles, float32 tables, the Leauthaud11 family, more
    // walkers than one launch takes: the batched path serves them)
    TC_CHECK(n_walkers > many_walkers_limit() || !single_draw_eligible(t, 1, n_gauss, flags),
             "internal: un-batched routing");
    return tc_predict_zheng07_batch(t, theta, n_theta, n_walkers, n_gauss, flags, ngal, xi);
  }
  TC_HIP(hipSetDevice(t->device));
  if (n_walkers == 1 && t->resident.enabled && resident_eligible(t, n_gauss))
    return resident_predict(t, theta, n_theta, n_gauss, flags, ngal, xi);
  // the resident kernel by itself for loops of un-batched calls (internal.h: Resident::auto_*)
  const bool auto_candidate = n_walkers == 1 && t->resident.auto_mode && !t->resident.enabled &&
                              resident_eligible(t, n_gauss);
  if (auto_candidate && resident_auto_wants(t)) {
    const unsigned long long before = t->resident.relaunches;
    status = resident_predict(t, theta, n_theta, n_gauss, flags, ngal, xi);
    if (status == TC_OK) {
      resident_auto_served(t, t->resident.relaunches != before);
      return status;
    }
    resident_auto_failed(t);     // (and serve this call by a launch)
  }
  if (t->resident.enabled && ensemble_eligible(t, n_walkers, n_gauss, flags)) {
    status = ensemble_predict(t, theta, n_theta, n_walkers, n_gauss, flags, ngal, xi);
    if (status != TC_ERR_UNSUPPORTED) return status;     // (else: the launched path below)
  }
  if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  status = launch_single_draw(t, theta, n_theta, n_walkers, n_gauss, flags, &t->single_ws,
                              t->stream);
  if (status != TC_OK) return status;
  status = wait_single_done(&t->single_ws, t->stream, t->tuning.poll_done != 0);
  if (status != TC_OK) return status;
  for (int w = 0; w < n_walkers; ++w)
    combine_single_draw(t, t->single_ws, w, ngal + w, xi + (size_t)w * t->n_r);
  if (auto_candidate) t->resident.auto_last_ns = monotonic_ns();
  return TC_OK;
}

// One draw against SEVERAL tables -- the reference's documented step evaluates two:
// halotab_wp.predict(model), then halotab_ds.predict(model) (docs/guides/overview.rst:86-92,
// tests/test_database.py:17-18).  Every table's call is posted first -- the parameters into the
// mailbox of its resident kernel, or one launch of single_draw_kernel on the table's own stream
// -- and only then are the answers waited for, in table order: the tables' round trips overlap
// (two tables: 18.6 -> ~11 us per pair with the resident kernels, 33 -> ~20 us with launches).
// Which path serves a table is decided as in tc_predict_zheng07_many, table by table, and the
// results are those calls' bit for bit.
int tc_predict_zheng07_joint(tc_table* const* tables, int n_tables, const double* theta,
                             int n_theta, int n_gauss, unsigned flags, double* ngal,
                             double* const* xi) {
  constexpr int kMaxJoint = 16;
  TC_CHECK(tables != nullptr && n_tables >= 1 && n_tables <= kMaxJoint,
           "n_tables must be in [1, %d]", kMaxJoint);
  TC_CHECK(ngal != nullptr && xi != nullptr, "output pointer is NULL");
  enum Route { kGeneric, kResident, kLaunched };
  Route route[kMaxJoint];
  bool automatic[kMaxJoint];
  unsigned long long relaunches[kMaxJoint];
  for (int k = 0; k < n_tables; ++k) {
    tc_table* t = tables[k];
    int status = check_predict_args(t, theta, n_theta, 1, n_gauss, flags);
    if (status != TC_OK) return status;
    TC_CHECK(xi[k] != nullptr, "output pointer is NULL");
    for (int j = 0; j < k; ++j) TC_CHECK(tables[j] != t, "a table appears twice");
    route[k] = kGeneric;
    automatic[k] = false;
    if (batch_invariant_form(t, n_gauss, flags) || !single_draw_eligible(t, 1, n_gauss, flags))
      continue;
    TC_HIP(hipSetDevice(t->device));
    tc_table::Resident& r = t->resident;
    const bool eligible = resident_eligible(t, n_gauss);
    const bool candidate = r.auto_mode && !r.enabled && eligible;
    if (r.enabled && eligible) {
      route[k] = kResident;
    } else if (candidate && resident_auto_wants(t)) {
      route[k] = kResident;
      automatic[k] = true;
    } else {
      route[k] = kLaunched;
      automatic[k] = candidate;
    }
  }
  // post
  int first_error = TC_OK;
  for (int k = 0; k < n_tables; ++k) {
    tc_table* t = tables[k];
    if (route[k] == kGeneric) continue;
    TC_HIP(hipSetDevice(t->device));
    if (route[k] == kResident) {
      relaunches[k] = t->resident.relaunches;
      int status = resident_post(t, theta, n_theta, n_gauss, flags);
      if (status == TC_OK) continue;
      if (!automatic[k]) {
        first_error = status;
        n_tables = k;             // (collect what was posted, then report)
        break;
      }
      resident_auto_failed(t);    // (tc_predict_zheng07_many's fallback)
      route[k] = kLaunched;
    }
    int status = TC_OK;
    if (t->resident.running) status = resident_stop(t);
    if (status == TC_OK)
      status = launch_single_draw(t, theta, n_theta, 1, n_gauss, flags, &t->single_ws, t->stream);
    if (status != TC_OK) {
      first_error = status;
      n_tables = k;
      break;
    }
  }
  // collect, in table order
  for (int k = 0; k < n_tables; ++k) {
    tc_table* t = tables[k];
    TC_HIP(hipSetDevice(t->device));
    int status = TC_OK;
    if (route[k] == kGeneric) {
      status = tc_predict_zheng07_many(t, theta, n_theta, 1, n_gauss, flags, ngal + k, xi[k]);
    } else if (route[k] == kResident) {
      status = resident_collect(t, theta, n_theta, n_gauss, flags, ngal + k, xi[k]);
      if (status == TC_OK && automatic[k])
        resident_auto_served(t, t->resident.relaunches != relaunches[k]);
      if (status != TC_OK && automatic[k]) {
        resident_auto_failed(t);  // (as above: serve this table by a launch)
        status = launch_single_draw(t, theta, n_theta, 1, n_gauss, flags, &t->single_ws,
                                    t->stream);
        if (status == TC_OK)
          status = wait_single_done(&t->single_ws, t->stream, t->tuning.poll_done != 0);
        if (status == TC_OK) combine_single_draw(t, t->single_ws, 0, ngal + k, xi[k]);
      }
    } else {
      status = wait_single_done(&t->single_ws, t->stream, t->tuning.poll_done != 0);
      if (status == TC_OK) combine_single_draw(t, t->single_ws, 0, ngal + k, xi[k]);
      if (automatic[k]) t->resident.auto_last_ns = monotonic_ns();
    }
    if (status != TC_OK && first_error == TC_OK) first_error = status;
  }
  return first_error;
}

// ---- forward calls (predict_call.h: PredictRequest, forward_chunked, forward_zero_copy) -------

namespace {
int predict_async(tc_table* t, const PredictRequest& request, const double* data,
                  const double* precision, int64_t* ticket_out, const Call* chunk,
                  hipEvent_t wait_for = nullptr, hipEvent_t kernels_done = nullptr);

// A table as forward_chunked and forward_zero_copy see it: the handle (its staging areas h_in and
// h_out, its tickets, its pinned lane's stream), the Call every chunk carries, the events between
// the chunks of a staggered plan (NULL: never staggered), the asynchronous path, the wait for
// everything queued, and the launches on the pinned lane.
struct TableForward {
  static constexpr bool kThreadedCopyOut = true;
  tc_table* t;
  tc_table* handle() const { return t; }
  // Every chunk takes the one-launch form with sync_form draws per workgroup wherever it serves
  // the table at all: a draw's result there does not depend on the number of chunks
  // (tests/test_gpu_async.py); elsewhere chunks differ from one piece by rounding.
  Call hints(const PredictRequest& request, const tc::SyncChunkPlan& plan) const {
    Call hints = probe_call(t);
    hints.async = true;                      // (as the chunks will run)
    hints.chain = false;
    // (the latency form for every chunk when the whole call fits one round of 40-draw workgroups:
    // the chunks' launches then fill the chip together)
    hints.sync_spread = request.n_draws >= t->tuning.fused_spread_min &&
                        (request.n_draws + 39) / 40 + plan.n_chunks <= (int64_t)t->n_cus;
    hints.sync_spread = hints.sync_spread &&
        tc::choose_fused_form(fused_query(t, hints, request.n_draws, request.n_gauss,
                                          request.flags)).draws == 40;
    if (hints.sync_spread) {
      hints.fused_draws = 40;
    } else if (t->tuning.sync_form != 0 && hints.fused_draws == 0 && t->tuning.fused == 1 &&
               t->tuning.deterministic < 2) {
      hints.fused_draws = t->tuning.sync_form;
      if (hints.fused_min_draws == 0) hints.fused_min_draws = 1;
    }
    return hints;
  }
  std::vector<hipEvent_t>* chunk_events() const { return &t->chunk_events; }
  int enqueue(const PredictRequest& part, const Call& hints, hipEvent_t wait_for,
              hipEvent_t kernels_done, int64_t* ticket) const {
    return predict_async(t, part, nullptr, nullptr, ticket, &hints, wait_for, kernels_done);
  }
  int synchronize() const { return tc_table_synchronize(t); }
  // (a likelihood: operands on the device, xi to t->out_xi; one slab's finalisation may write it)
  int run(const PredictRequest& s) const {
    Call call = make_call(t, /*pinned=*/true);
    call.chi2_data = s.likelihood ? t->chi2.device() : nullptr;
    call.chi2_out = s.likelihood && s.n_draws <= max_slab(t) ? s.second : nullptr;
    bool written = !s.likelihood;
    double* xi = s.likelihood ? (double*)t->out_xi.ptr : s.second;
    int status = predict_device(t, call, s.theta, s.n_theta, s.n_draws, s.n_gauss, s.flags, s.ngal,
                                xi, s.likelihood ? &written : nullptr);
    if (status == TC_OK && !written)
      status = launch_chi2(xi, s.n_draws, t->n_r, call.chi2_data, call.chi2_data + t->n_r,
                           s.second, t->stream);
    return status;
  }
};
}  // namespace

int tc_predict_zheng07_batch(tc_table* t, const double* theta, int n_theta,
                             int64_t n_draws, int n_gauss, unsigned flags,
                             double* ngal, double* xi) {
  int status = check_predict_args(t, theta, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(ngal && xi, "output pointer is NULL");
  TC_HIP(hipSetDevice(t->device));
  const PredictRequest request =
      forward_request(t, theta, n_theta, 0, nullptr, n_draws, n_gauss, flags, ngal, xi, false);
  // (option "deterministic" = 2: neither of the un-batched kernels -- their sums are cut
  // differently from the batched forms')
  const bool invariant = batch_invariant_form(t, n_gauss, flags);
  if (!invariant && t->resident.enabled && ensemble_eligible(t, n_draws, n_gauss, flags)) {
    // an ensemble of up to 256 walkers with option "resident": no launch at all (unless its
    // workgroups do not all find a place on the chip: the launched path below)
    status = ensemble_predict(t, theta, n_theta, (int)n_draws, n_gauss, flags, ngal, xi);
    if (status != TC_ERR_UNSUPPORTED) return status;
  }
  if (!invariant && n_draws <= many_walkers_limit() &&
      single_draw_eligible(t, 1, n_gauss, flags)) {
    // one draw -- or a handful (an ensemble sampler's proposals): ONE launch, the device-side
    // combination replaced by a few hundred additions here (kernels.hip.h: single_draw_kernel)
    return tc_predict_zheng07_many(t, theta, n_theta, (int)n_draws, n_gauss, flags, ngal, xi);
  }
  // small and medium calls (an MCMC step, a few thousand walkers): straight on page-locked staging
  const TableForward forward{t};
  if (zero_copy_serves(forward, request)) return forward_zero_copy(forward, request);
  const tc::SyncChunkPlan plan = plan_forward_chunks(t, t->n_lanes, t->chain, false, request);
  if (plan.n_chunks > 0) return forward_chunked(forward, request, plan);
  status = t->theta.reserve(request.theta_bytes(), t->stream);
  if (status == TC_OK) status = t->out_ngal.reserve(request.ngal_count() * 8, t->stream);
  if (status == TC_OK) status = t->out_xi.reserve(request.second_count() * 8, t->stream);
  if (status != TC_OK) return status;
  status = copy_in(&t->h_in, t->theta.ptr, theta, request.theta_bytes(), t->stream);
  if (status != TC_OK) return status;
  status = forward.run(request.on((const double*)t->theta.ptr, nullptr, (double*)t->out_ngal.ptr,
                                  (double*)t->out_xi.ptr));
  if (status != TC_OK) return status;
  return copy_out(&t->h_out, ngal, request.ngal_count(), t->out_ngal.ptr, xi,
                  request.second_count(), t->out_xi.ptr, t->stream);
}

namespace {

// What the operand cache of a table waits for before new values go up: every lane's stream.
int drain_lanes(tc_table* t) {
  for (tc_table::Lane& lane : t->lanes)
    if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
  return TC_OK;
}

// The data vector and the precision matrix of a likelihood on the device (internal.h:
// Chi2Operands).
int upload_operands(tc_table* t, const double* data, const double* precision) {
  return t->chi2.upload(t->n_r, data, precision, t->stream, [t] { return drain_lanes(t); });
}

// A likelihood of 0 < n_draws <= max_slab(t) draws on device pointers as `call` describes it
// (the arguments are checked): tc_chi2_zheng07_batch_device and its asynchronous twin.
int chi2_on_device(tc_table* t, Call call, const double* theta_device, int n_theta, int64_t n_draws,
                int n_gauss, unsigned flags, const double* data, const double* precision,
                double* ngal_device, double* chi2_device) {
  TC_HIP(hipSetDevice(t->device));
  int status = TC_OK;
  if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  status = upload_operands(t, data, precision);
  if (status != TC_OK) return status;
  // xi stays in a workspace of the lane the call runs on; the lane's `finished` event is
  // re-recorded behind the chi2 kernel, so the next call on this lane (whose finalisation
  // waits for that event through the chain of lanes) cannot overwrite it early
  tc_table::Lane& lane = t->lanes[call.lane];
  status = lane.xi.reserve((size_t)n_draws * t->n_r * 8, lane.stream);
  if (status != TC_OK) return status;
  call.chi2_data = t->chi2.device();
  call.chi2_out = chi2_device;
  bool written = false;
  status = predict_device(t, call, theta_device, n_theta, n_draws, n_gauss, flags, ngal_device,
                          (double*)lane.xi.ptr, &written);
  if (status != TC_OK) return status;
  if (written) return TC_OK;            // (the finalisation kernel wrote chi2 itself)
  status = launch_chi2((const double*)lane.xi.ptr, n_draws, t->n_r, call.chi2_data,
                       call.chi2_data + t->n_r, chi2_device, lane.stream);
  if (status != TC_OK) return status;
  if (!call.pinned && call.chain) TC_HIP(hipEventRecord(lane.finished, lane.stream));
  return TC_OK;
}

}  // namespace

int tc_chi2_zheng07_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                 int64_t n_draws, int n_gauss, unsigned flags,
                                 const double* data, const double* precision,
                                 double* ngal_device, double* chi2_device) {
  int status = check_predict_args(t, theta_device, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  TC_CHECK(!(flags & TC_FLAG_SEPARATE_GAL_TYPE),
           "chi2 is defined for the total correlation function only");
  if (n_draws == 0) return TC_OK;
  TC_CHECK(data && precision && ngal_device && chi2_device, "NULL pointer");
  TC_CHECK(n_draws <= max_slab(t), "at most %lld draws per call",
           (long long)max_slab(t));
  return chi2_on_device(t, make_call(t, /*pinned=*/false), theta_device, n_theta, n_draws, n_gauss,
                     flags, data, precision, ngal_device, chi2_device);
}

int tc_chi2_zheng07_batch(tc_table* t, const double* theta, int n_theta,
                          int64_t n_draws, int n_gauss, unsigned flags,
                          const double* data, const double* precision, double* ngal,
                          double* chi2) {
  int status = check_predict_args(t, theta, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  TC_CHECK(!(flags & TC_FLAG_SEPARATE_GAL_TYPE),
           "chi2 is defined for the total correlation function only");
  if (n_draws == 0) return TC_OK;
  TC_CHECK(data && precision && ngal && chi2, "NULL pointer");
  TC_HIP(hipSetDevice(t->device));
  const PredictRequest request =
      forward_request(t, theta, n_theta, 0, nullptr, n_draws, n_gauss, flags, ngal, chi2, true);
  status = t->out_xi.reserve((size_t)n_draws * t->n_r * 8, t->stream);   // (run()'s workspace)
  if (status == TC_OK) status = upload_operands(t, data, precision);
  if (status != TC_OK) return status;
  // small calls: draws read from and results written to page-locked host memory directly
  const TableForward forward{t};
  if (zero_copy_serves(forward, request)) return forward_zero_copy(forward, request);
  status = t->theta.reserve(request.theta_bytes(), t->stream);
  if (status == TC_OK) status = t->out_ngal.reserve(request.out_bytes(), t->stream);
  if (status != TC_OK) return status;
  status = copy_in(&t->h_in, t->theta.ptr, theta, request.theta_bytes(), t->stream);
  if (status != TC_OK) return status;
  double* d_ngal = (double*)t->out_ngal.ptr;
  double* d_chi2 = d_ngal + request.ngal_count();
  status = forward.run(request.on((const double*)t->theta.ptr, nullptr, d_ngal, d_chi2));
  if (status != TC_OK) return status;
  return copy_out(&t->h_out, ngal, request.ngal_count(), d_ngal, chi2, request.second_count(),
                  d_chi2, t->stream);
}

// ---- gradients (grad_call.h: grad_entry; launch.hip: run_grad) ----------------------------

namespace {

// What the derivative entries of a table share (grad_call.h: grad_entry, vjp_entry).
struct TableHandle {
  tc_table* t;
  int device_id() const { return t->device; }
  Chi2Operands& operands() const { return t->chi2; }
  int upload_chi2(const Chi2Host& host) const {
    return upload_operands(t, host.data, host.precision);
  }
};

// A table as grad_entry sees it.
struct TableGrad : TableHandle {
  int check(const GradRequest& request, int n_theta, bool likelihood) const {
    return check_grad_args(t, request, n_theta, likelihood, /*fit=*/true);
  }
  const char* null_message(bool likelihood) const {
    return likelihood ? "NULL pointer" : "output pointer is NULL";
  }
  GradStaging staging() const {
    return {&t->theta, nullptr, &t->out_ngal, &t->out_xi, t->stream};
  }
  // (grad_slabs: the table's resident kernel stops, the lane is the table's next, t->prev says
  // who may chain to it)
  int device(GradLane lane, const GradRequest& request) const {
    return grad_slabs(t, lane, request.n_draws, [&](int64_t begin, int64_t n, hipStream_t stream) {
      return run_grad(t, request.slab(begin, n), stream);
    });
  }
};

// The request of a table entry point of the family `n_params`, in the order of the C arguments.
GradRequest table_request(const tc_table* t, int n_params, const double* theta, int64_t n_draws,
                          int n_gauss, unsigned flags, double* ngal, double* value,
                          double* dngal, double* dvalue, double* fisher) {
  GradRequest request{};
  request.n_params = n_params;
  request.n_gauss = n_gauss;
  request.flags = flags;
  request.n_draws = n_draws;
  request.n_r = t ? t->n_r : 0;
  request.theta = theta;
  request.ngal = ngal;
  request.dngal = dngal;
  request.value = value;
  request.dvalue = dvalue;
  request.fisher = fisher;
  return request;
}

}  // namespace

int tc_predict_grad_zheng07_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                         int64_t n_draws, int n_gauss, unsigned flags,
                                         double* ngal_device, double* xi_device,
                                         double* dngal_device, double* dxi_device) {
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParams, theta_device, n_draws, n_gauss, flags,
                                  ngal_device, xi_device, dngal_device, dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_predict_grad_zheng07_batch(tc_table* t, const double* theta, int n_theta,
                                  int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                                  double* xi, double* dngal, double* dxi) {
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParams, theta, n_draws, n_gauss, flags, ngal, xi,
                                  dngal, dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_chi2_grad_zheng07_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                      int64_t n_draws, int n_gauss, unsigned flags,
                                      const double* data, const double* precision,
                                      double* ngal_device, double* chi2_device,
                                      double* dngal_device, double* dchi2_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParams, theta_device, n_draws, n_gauss, flags,
                                  ngal_device, chi2_device, dngal_device, dchi2_device, nullptr),
                    n_theta, &operands, false);
}

int tc_chi2_grad_zheng07_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                               int n_gauss, unsigned flags, const double* data,
                               const double* precision, double* ngal, double* chi2,
                               double* dngal, double* dchi2) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParams, theta, n_draws, n_gauss, flags, ngal, chi2,
                                  dngal, dchi2, nullptr),
                    n_theta, &operands, false);
}

int tc_chi2_fisher_zheng07_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                        int64_t n_draws, int n_gauss, unsigned flags,
                                        const double* data, const double* precision,
                                        double* ngal_device, double* chi2_device,
                                        double* dngal_device, double* dchi2_device,
                                        double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParams, theta_device, n_draws, n_gauss, flags,
                                  ngal_device, chi2_device, dngal_device, dchi2_device,
                                  fisher_device),
                    n_theta, &operands, true);
}

int tc_chi2_fisher_zheng07_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                                 int n_gauss, unsigned flags, const double* data,
                                 const double* precision, double* ngal, double* chi2,
                                 double* dngal, double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParams, theta, n_draws, n_gauss, flags, ngal, chi2,
                                  dngal, dchi2, fisher),
                    n_theta, &operands, true);
}

// ---- gradients of the model decorated with assembly bias (seven columns, the strengths last)
// and of the Leauthaud11 family (fourteen theta columns, eleven differentiated: grad.h:
// kGradParamsLeauthaud11); `fisher` may be NULL ----

int tc_predict_grad_assembias_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                        int64_t n_draws, int n_gauss, unsigned flags,
                                        double* ngal_device, double* xi_device,
                                        double* dngal_device, double* dxi_device) {
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParamsAssembias, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  xi_device, dngal_device, dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_predict_grad_assembias_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                                 int n_gauss, unsigned flags, double* ngal, double* xi,
                                 double* dngal, double* dxi) {
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParamsAssembias, theta, n_draws, n_gauss, flags, ngal, xi, dngal,
                                  dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_chi2_grad_assembias_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                     int64_t n_draws, int n_gauss, unsigned flags,
                                     const double* data, const double* precision,
                                     double* ngal_device, double* chi2_device,
                                     double* dngal_device, double* dchi2_device,
                                     double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParamsAssembias, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  chi2_device, dngal_device, dchi2_device, fisher_device),
                    n_theta, &operands, false);
}

int tc_chi2_grad_assembias_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                              int n_gauss, unsigned flags, const double* data,
                              const double* precision, double* ngal, double* chi2, double* dngal,
                              double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParamsAssembias, theta, n_draws, n_gauss, flags, ngal, chi2, dngal,
                                  dchi2, fisher),
                    n_theta, &operands, false);
}

int tc_predict_grad_leauthaud11_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                        int64_t n_draws, int n_gauss, unsigned flags,
                                        double* ngal_device, double* xi_device,
                                        double* dngal_device, double* dxi_device) {
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParamsLeauthaud11, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  xi_device, dngal_device, dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_predict_grad_leauthaud11_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                                 int n_gauss, unsigned flags, double* ngal, double* xi,
                                 double* dngal, double* dxi) {
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParamsLeauthaud11, theta, n_draws, n_gauss, flags, ngal, xi, dngal,
                                  dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_chi2_grad_leauthaud11_batch_device(tc_table* t, const double* theta_device, int n_theta,
                                     int64_t n_draws, int n_gauss, unsigned flags,
                                     const double* data, const double* precision,
                                     double* ngal_device, double* chi2_device,
                                     double* dngal_device, double* dchi2_device,
                                     double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kDevice,
                    table_request(t, tc::kGradParamsLeauthaud11, theta_device, n_draws, n_gauss, flags, ngal_device,
                                  chi2_device, dngal_device, dchi2_device, fisher_device),
                    n_theta, &operands, false);
}

int tc_chi2_grad_leauthaud11_batch(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                              int n_gauss, unsigned flags, const double* data,
                              const double* precision, double* ngal, double* chi2, double* dngal,
                              double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(TableGrad{t}, GradRoute::kHost,
                    table_request(t, tc::kGradParamsLeauthaud11, theta, n_draws, n_gauss, flags, ngal, chi2, dngal,
                                  dchi2, fisher),
                    n_theta, &operands, false);
}

// ---- occupation VJP (grad_call.h: vjp_entry; launch.hip: run_vjp) -------------------------

namespace {

// A table as vjp_entry sees it: no forward-only form, every adjoint array is required.
struct TableVjp : TableHandle {
  int check(int64_t n_draws, unsigned flags) const { return check_vjp_args(t, n_draws, flags); }
  VjpRule rule() const { return {false, false, {nullptr, nullptr}}; }
  VjpStaging staging() const {
    return {&t->occupation, &t->out_ngal, &t->out_xi, t->stream, max_slab(t)};
  }
  // (grad_slabs, as TableGrad: one launch of the table's kernel per slab)
  int device(GradLane lane, const VjpRequest& request) const {
    return grad_slabs(t, lane, request.n_draws, [&](int64_t begin, int64_t n, hipStream_t stream) {
      return run_vjp(t, request.slab(begin, n), stream);
    });
  }
};

// The request of a table's entry point at the occupation seam, in the order of the C arguments.
VjpRequest vjp_request(const tc_table* t, const double* occupation, int64_t n_draws,
                       const double* g_ngal, const double* g_xi, double* ngal, double* xi,
                       double* chi2, double* g_occupation) {
  return VjpRequest{n_draws, t ? t->n_bins : 0, t ? t->n_r : 0, occupation, g_ngal, g_xi,
                    nullptr, ngal, xi, chi2, g_occupation, 1, 0, nullptr, nullptr, nullptr};
}

}  // namespace

int tc_predict_occupation_vjp_batch_device(tc_table* t, const double* occupation_device,
                                           int64_t n_draws, unsigned flags,
                                           const double* g_ngal_device, const double* g_xi_device,
                                           double* ngal_device, double* xi_device,
                                           double* g_occupation_device) {
  return vjp_entry(TableVjp{t}, GradRoute::kDevice, flags,
                   vjp_request(t, occupation_device, n_draws, g_ngal_device, g_xi_device,
                               ngal_device, xi_device, nullptr, g_occupation_device),
                   nullptr);
}

int tc_predict_occupation_vjp_batch(tc_table* t, const double* occupation, int64_t n_draws,
                                    unsigned flags, const double* g_ngal, const double* g_xi,
                                    double* ngal, double* xi, double* g_occupation) {
  return vjp_entry(TableVjp{t}, GradRoute::kHost, flags,
                   vjp_request(t, occupation, n_draws, g_ngal, g_xi, ngal, xi, nullptr,
                               g_occupation),
                   nullptr);
}

int tc_chi2_occupation_grad_batch_device(tc_table* t, const double* occupation_device,
                                         int64_t n_draws, unsigned flags, const double* data,
                                         const double* precision, double* ngal_device,
                                         double* chi2_device, double* dchi2_docc_device) {
  const Chi2Host operands{data, precision};
  return vjp_entry(TableVjp{t}, GradRoute::kDevice, flags,
                   vjp_request(t, occupation_device, n_draws, nullptr, nullptr, ngal_device,
                               nullptr, chi2_device, dchi2_docc_device),
                   &operands);
}

int tc_chi2_occupation_grad_batch(tc_table* t, const double* occupation, int64_t n_draws,
                                  unsigned flags, const double* data, const double* precision,
                                  double* ngal, double* chi2, double* dchi2_docc) {
  const Chi2Host operands{data, precision};
  return vjp_entry(TableVjp{t}, GradRoute::kHost, flags,
                   vjp_request(t, occupation, n_draws, nullptr, nullptr, ngal, nullptr, chi2,
                               dchi2_docc),
                   &operands);
}

namespace {

// Asynchronous host-to-host prediction or likelihood on the handle's next lane: everything
// (upload, three kernels, download, the ticket's event) is queued on that lane's stream, so lanes
// overlap each other's copies and kernels and nothing orders one ticket against another.
// `chunk` (or NULL): the call is a chunk of a synchronous call (forward_chunked) and this is what
// every chunk carries; the buffers are then the library's own page-locked staging areas.
// wait_for / kernels_done (the chunks of a staggered plan): the call's kernels start behind
// `wait_for`, and `kernels_done` is recorded between its kernels and its download -- the chunks'
// kernels run one after the other, each with the chip to itself, while the previous results travel.
int predict_async(tc_table* t, const PredictRequest& r, const double* data,
                  const double* precision, int64_t* ticket_out, const Call* chunk,
                  hipEvent_t wait_for, hipEvent_t kernels_done) {
  int status = check_predict_args(t, r.theta, r.n_theta, r.n_draws, r.n_gauss, r.flags);
  if (status != TC_OK) return status;
  const int64_t n_draws = r.n_draws;
  const bool chi2 = r.likelihood;
  TC_CHECK(ticket_out != nullptr, "ticket is NULL");
  TC_CHECK(n_draws == 0 || (r.ngal && r.second), "output pointer is NULL");
  TC_CHECK(!(chi2 && r.separate()), "chi2 is defined for the total correlation function only");
  TC_CHECK(!chi2 || (data && precision), "NULL pointer");
  TC_CHECK(!chi2 || n_draws <= max_slab(t), "at most %lld draws per call",
           (long long)max_slab(t));
  const size_t ngal_count = r.ngal_count(), second_count = r.second_count();
  const size_t theta_bytes = r.theta_bytes();
  void *theta_seen = (void*)r.theta, *ngal_seen = r.ngal, *second_seen = r.second;
  const bool staging = chunk != nullptr;
  TC_CHECK(staging || n_draws == 0 || (is_pinned(r.theta, theta_bytes, &theta_seen) &&
                                       is_pinned(r.ngal, ngal_count * 8, &ngal_seen) &&
                                       is_pinned(r.second, second_count * 8, &second_seen)),
           "asynchronous calls need page-locked buffers (tc_host_alloc / tc_host_register)");
  TC_HIP(hipSetDevice(t->device));
  if (t->resident.running) {
    const int stopped = resident_stop(t);
    if (stopped != TC_OK) return stopped;
  }
  // (the finalisations of asynchronous calls are never chained: each has its ticket)
  Call call = chunk != nullptr ? *chunk : probe_call(t);
  call.lane = next_lane(false, t->tuning.pipeline != 0, t->n_lanes, &t->device_calls);
  call.async = true;
  call.chain = false;
  tc_table::Lane& lane = t->lanes[call.lane];
  if (n_draws > 0) {
    // Which arrays the kernels address in the caller's page-locked memory themselves and
    // which travel by copy command: see Tuning::async_direct_in / async_direct_out.
    // (the chunks of a synchronous call: the kernels store up to 1 MB per array themselves -- 10^4
    // draws of 19 r values in two chunks 128 us against 151; larger chunks by the copy engines)
    const int mode = staging ? t->tuning.sync_direct_out : t->tuning.async_direct_out;
    const size_t direct_bytes = staging ? kSyncDirectOutBytes : kDirectOutBytes;
    auto direct = [mode, direct_bytes](void* seen, size_t count) {
      return seen != nullptr && (mode == 1 || (mode == 2 && count * 8 <= direct_bytes));
    };
    const bool direct_in = t->tuning.async_direct_in && theta_seen != nullptr;
    const bool direct_ngal = direct(ngal_seen, ngal_count);
    const bool direct_second = direct(second_seen, second_count);
    if (!direct_in) status = lane.in_theta.reserve(theta_bytes, lane.stream);
    if (status == TC_OK && !(direct_ngal && direct_second))
      status = lane.out.reserve((ngal_count + second_count) * 8, lane.stream);
    if (status != TC_OK) return status;
    const double* d_theta = direct_in ? (const double*)theta_seen
                                      : (const double*)lane.in_theta.ptr;
    double* d_ngal = direct_ngal ? (double*)ngal_seen : (double*)lane.out.ptr;
    double* d_second = direct_second ? (double*)second_seen
                                     : (double*)lane.out.ptr + ngal_count;
    if (!direct_in) {
      Range range("upload");
      TC_HIP(hipMemcpyAsync(lane.in_theta.ptr, r.theta, theta_bytes, hipMemcpyHostToDevice,
                            lane.stream));
    }
    if (wait_for != nullptr) TC_HIP(hipStreamWaitEvent(lane.stream, wait_for, 0));
    status = chi2 ? chi2_on_device(t, call, d_theta, r.n_theta, n_draws, r.n_gauss, r.flags, data,
                                   precision, d_ngal, d_second)
                  : predict_device(t, call, d_theta, r.n_theta, n_draws, r.n_gauss, r.flags,
                                   d_ngal, d_second);
    if (status != TC_OK) return status;
    if (kernels_done != nullptr) TC_HIP(hipEventRecord(kernels_done, lane.stream));
    Range range("download");
    if (!direct_ngal && !direct_second && r.second == r.ngal + ngal_count) {
      // (adjacent in the caller's memory as in the staging buffer: one command)
      TC_HIP(hipMemcpyAsync(r.ngal, d_ngal, (ngal_count + second_count) * 8,
                            hipMemcpyDeviceToHost, lane.stream));
    } else {
      if (!direct_ngal)
        TC_HIP(hipMemcpyAsync(r.ngal, d_ngal, ngal_count * 8, hipMemcpyDeviceToHost,
                              lane.stream));
      if (!direct_second)
        TC_HIP(hipMemcpyAsync(r.second, d_second, second_count * 8, hipMemcpyDeviceToHost,
                              lane.stream));
    }
  }
  return t->tickets.issue(lane.stream, ticket_out);
}

}  // namespace

int tc_predict_zheng07_batch_async(tc_table* t, const double* theta, int n_theta,
                                   int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                                   double* xi, int64_t* ticket) {
  return predict_async(t, forward_request(t, theta, n_theta, 0, nullptr, n_draws, n_gauss, flags,
                                          ngal, xi, false),
                       nullptr, nullptr, ticket, nullptr);
}

int tc_chi2_zheng07_batch_async(tc_table* t, const double* theta, int n_theta, int64_t n_draws,
                                int n_gauss, unsigned flags, const double* data,
                                const double* precision, double* ngal, double* chi2,
                                int64_t* ticket) {
  return predict_async(t, forward_request(t, theta, n_theta, 0, nullptr, n_draws, n_gauss, flags,
                                          ngal, chi2, true),
                       data, precision, ticket, nullptr);
}

int tc_table_wait(tc_table* t, int64_t ticket) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  return t->tickets.wait(ticket, [t] { return tc_table_synchronize(t); });
}

int tc_table_query(tc_table* t, int64_t ticket, int* done) {
  TC_CHECK(t != nullptr && done != nullptr, "NULL argument");
  static const char* const what[2] = {"hipEventQuery", "hipStreamQuery"};
  return t->tickets.query(ticket, done, t->lanes, what);
}

int tc_mean_occupation_zheng07_batch(tc_table* t, const double* theta, int n_theta,
                                     int64_t n_draws, int n_gauss, unsigned flags,
                                     double* occupation) {
  int status = check_predict_args(t, theta, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(occupation != nullptr, "output pointer is NULL");
  TC_HIP(hipSetDevice(t->device));
  if (t->resident.running) {
    const int stopped = resident_stop(t);
    if (stopped != TC_OK) return stopped;
  }
  const int64_t slab = max_slab(t);
  for (int64_t begin = 0; begin < n_draws; begin += slab) {
    const int64_t n = std::min(slab, n_draws - begin);
    const int64_t ldb = (n + 63) / 64 * 64;
    const size_t occ_bytes = (size_t)n * t->n_bins * 8;
    status = t->theta.reserve((size_t)n * n_theta * 8, t->stream);
    if (status == TC_OK) status = t->occupation.reserve(occ_bytes, t->stream);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(t->theta.ptr, theta + begin * n_theta,
                          (size_t)n * n_theta * 8, hipMemcpyHostToDevice, t->stream));
    t->cur = 0;
    status = run_occupation(t, probe_call(t), (const double*)t->theta.ptr, n_theta, n, ldb,
                            n_gauss, flags, (double*)t->occupation.ptr);
    if (status != TC_OK) return status;
    TC_HIP(hipMemcpyAsync(occupation + begin * t->n_bins, t->occupation.ptr,
                          occ_bytes, hipMemcpyDeviceToHost, t->stream));
    TC_HIP(hipStreamSynchronize(t->stream));
  }
  return TC_OK;
}

int tc_predict_occupation_batch(tc_table* t, const double* occupation,
                                int64_t n_draws, unsigned flags, double* ngal,
                                double* xi) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  TC_CHECK(n_draws >= 0, "n_draws must be non-negative");
  if (n_draws == 0) return TC_OK;
  TC_CHECK(occupation && ngal && xi, "NULL array");
  TC_HIP(hipSetDevice(t->device));
  if (t->resident.running) {
    const int stopped = resident_stop(t);
    if (stopped != TC_OK) return stopped;
  }
  const bool separate = (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0;
  const int n_comp = separate ? t->plan.n_components : 1;
  const int64_t slab = max_slab(t);
  for (int64_t begin = 0; begin < n_draws; begin += slab) {
    const int64_t n = std::min(slab, n_draws - begin);
    const int64_t ldb = (n + 63) / 64 * 64;
    const size_t occ_bytes = (size_t)n * t->n_bins * 8;
    const size_t ngal_count = (size_t)n * (separate ? 2 : 1);
    const size_t xi_count = (size_t)n * n_comp * t->n_r;
    int status = t->occupation.reserve(occ_bytes, t->stream);
    if (status == TC_OK)
      status = t->lanes[0].nbuf.reserve((size_t)t->n_bins * ldb * 8, t->stream);
    if (status == TC_OK)
      status = t->lanes[0].ngal2.reserve(2 * ldb * 8, t->stream);
    if (status == TC_OK) status = t->out_ngal.reserve(ngal_count * 8, t->stream);
    if (status == TC_OK) status = t->out_xi.reserve(xi_count * 8, t->stream);
    if (status != TC_OK) return status;
    status = copy_in(&t->h_in, t->occupation.ptr, occupation + begin * t->n_bins,
                     occ_bytes, t->stream);
    if (status != TC_OK) return status;
    status = launch_occ_from_array(t, (const double*)t->occupation.ptr, n, ldb,
                                   (double*)t->lanes[0].nbuf.ptr,
                                   (double*)t->lanes[0].ngal2.ptr, t->stream);
    if (status != TC_OK) return status;
    t->cur = 0;
    t->lanes[0].ngal_parts = 1;
    status = run_contraction(t, probe_call(t), n, ldb, flags, (double*)t->out_ngal.ptr,
                             (double*)t->out_xi.ptr);
    if (status != TC_OK) return status;
    status = copy_out(&t->h_out, ngal + begin * (separate ? 2 : 1), ngal_count,
                      t->out_ngal.ptr, xi + begin * n_comp * t->n_r, xi_count,
                      t->out_xi.ptr, t->stream);
    if (status != TC_OK) return status;
  }
  return TC_OK;
}

namespace {

// Option "autotune": which form serves a batch of n draws fastest on THIS table in the
// pipelined regime -- three kernels, one launch with 64-draw workgroups, one launch with
// 32-draw workgroups --, measured for a grid of batch sizes with draws from a wide prior box and
// kept in the handle (internal.h: AutoChoice).  `flags`: the predict flags to tune for.
int autotune(tc_table* t, unsigned flags) {
  TC_CHECK(!(flags & ~(TC_FLAG_SEPARATE_GAL_TYPE | TC_FLAG_MODULATE_WITH_CENOCC |
                       TC_FLAG_ASSEMBIAS | TC_FLAG_LEAUTHAUD11)),
           "autotune: the value is a combination of predict flags");
  TC_CHECK(!((flags & TC_FLAG_LEAUTHAUD11) && (flags & TC_FLAG_ASSEMBIAS)),
           "autotune: no assembly bias for the Leauthaud11 family");
  int status = tc_table_synchronize(t);
  if (status != TC_OK) return status;
  if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  t->autotuned.erase(flags);
  const bool separate = (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0;
  const bool leauthaud = (flags & TC_FLAG_LEAUTHAUD11) != 0;
  const int n_theta = leauthaud ? 14 : (flags & TC_FLAG_ASSEMBIAS) ? 7 : 5;
  const int n_comp = separate ? t->plan.n_components : 1;
  const int64_t n_max = AutoChoice::size(AutoChoice::kSizes - 1);
  // draws: uniform in the box of tabcorr_amd.synthetic.zheng07_draws (/ the defaults of the
  // Leauthaud11 model with a little scatter), a fixed multiplicative generator
  std::vector<double> theta((size_t)n_max * n_theta);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto uniform = [&state]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) * (1.0 / 9007199254740992.0);
  };
  static const double lo[7] = {11.5, 0.1, 11.0, 12.5, 0.7, -1.0, -1.0};
  static const double hi[7] = {13.5, 0.8, 13.0, 14.5, 1.4, 1.0, 1.0};
  static const double leauthaud_mid[14] = {10.72, 12.35, 0.43, 0.56, 1.54, 0.2,  1.0,
                                           10.62, 0.859, 1.47, -0.13, 10.5, 0.7, 0.72};
  for (int64_t b = 0; b < n_max; ++b)
    for (int i = 0; i < n_theta; ++i)
      theta[(size_t)b * n_theta + i] =
          leauthaud ? leauthaud_mid[i] * (i < 12 ? 1.0 + 0.02 * (uniform() - 0.5) : 1.0)
                    : lo[i] + (hi[i] - lo[i]) * uniform();
  DeviceBuffer d_theta, d_ngal, d_xi;
  struct Release {
    DeviceBuffer *a, *b, *c;
    ~Release() {
      a->release();
      b->release();
      c->release();
    }
  } release{&d_theta, &d_ngal, &d_xi};
  status = d_theta.reserve(theta.size() * 8, t->stream);
  if (status == TC_OK) status = d_ngal.reserve((size_t)n_max * 2 * 8, t->stream);
  if (status == TC_OK) status = d_xi.reserve((size_t)n_max * n_comp * t->n_r * 8, t->stream);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpy(d_theta.ptr, theta.data(), theta.size() * 8, hipMemcpyHostToDevice));

  const Tuning saved = t->tuning;
  struct Restore {
    tc_table* t;
    Tuning saved;
    ~Restore() { t->tuning = saved; }
  } restore{t, saved};
  t->tuning.fused_min_draws = 1;
  t->tuning.fused_max_draws = 1 << 30;
  auto time_form = [&](int64_t n, float* us) -> int {
    auto call = [&]() {
      return tc_predict_zheng07_batch_device(t, (const double*)d_theta.ptr, n_theta, n, 10, flags,
                                             (double*)d_ngal.ptr, (double*)d_xi.ptr);
    };
    int st = TC_OK;
    for (int k = 0; k < 4 && st == TC_OK; ++k) st = call();          // warm (schedules, lanes)
    if (st == TC_OK) st = tc_table_synchronize(t);
    if (st != TC_OK) return st;
    // at least 8 ms and 8 calls, at most 400
    int calls = 8;
    double seconds = 0.0;
    for (;;) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; k < calls && st == TC_OK; ++k) st = call();
      if (st == TC_OK) st = tc_table_synchronize(t);
      if (st != TC_OK) return st;
      seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (seconds >= 8e-3 || calls >= 400) break;
      calls = (int)std::min<double>(400.0, std::max<double>(calls * 2.0,
                                                            calls * 1e-2 / std::max(seconds, 1e-6)));
    }
    *us = (float)(seconds / calls * 1e6);
    return TC_OK;
  };
  AutoChoice choice;
  for (int i = 0; i < AutoChoice::kSizes; ++i) {
    const int64_t n = AutoChoice::size(i);
    t->tuning.fused = 0;
    status = time_form(n, &choice.us[i][0]);
    if (status != TC_OK) return status;
    choice.form[i] = 0;
    float best = choice.us[i][0];
    const int shapes[2] = {64, 32};
    for (int k = 0; k < 2; ++k) {
      t->tuning.fused = 2;
      t->tuning.fused_draws = shapes[k];
      choice.us[i][1 + k] = 0.0f;
      // (the shape asked for is the one that would run?)
      if (tc::choose_fused_form(fused_query(t, probe_call(t), n, 10, flags)).draws != shapes[k])
        continue;
      status = time_form(n, &choice.us[i][1 + k]);
      if (status != TC_OK) return status;
      // (a one-launch form must win by 2 %: ties go to the three kernels)
      if (choice.us[i][1 + k] < 0.98f * best) {
        best = choice.us[i][1 + k];
        choice.form[i] = shapes[k];
      }
    }
  }
  t->autotuned[flags] = choice;
  return TC_OK;
}

}  // namespace

int tc_table_autotune_result(const tc_table* t, unsigned flags, int capacity, int* count,
                             int64_t* sizes, int* forms, float* us) {
  TC_CHECK(t != nullptr && count && sizes && forms && us, "NULL argument");
  *count = 0;
  auto it = t->autotuned.find(flags);
  TC_CHECK(it != t->autotuned.end(), "no autotune result for these flags");
  TC_CHECK(capacity >= AutoChoice::kSizes, "capacity below %d", (int)AutoChoice::kSizes);
  for (int i = 0; i < AutoChoice::kSizes; ++i) {
    sizes[i] = AutoChoice::size(i);
    forms[i] = it->second.form[i];
    for (int k = 0; k < 3; ++k) us[3 * i + k] = it->second.us[i][k];
  }
  *count = AutoChoice::kSizes;
  return TC_OK;
}

int tc_table_resident_stats(const tc_table* t, int64_t* launches, int64_t* relaunches,
                            int64_t* failures, int* running) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  const tc_table::Resident& r = t->resident;
  if (launches) *launches = (int64_t)r.launch_id;
  if (relaunches) *relaunches = (int64_t)r.relaunches;
  if (failures) *failures = (int64_t)r.auto_failures;
  if (running) *running = r.running ? (r.ensemble ? 2 : 1) : 0;
  return TC_OK;
}

int tc_table_batch_invariant(tc_table* t, int n_gauss, unsigned flags, int* out) {
  TC_CHECK(t != nullptr && out != nullptr, "NULL argument");
  TC_HIP(hipSetDevice(t->device));
  *out = batch_invariant_form(t, n_gauss, flags) ? 1 : 0;
  return TC_OK;
}

int tc_table_set_option(tc_table* t, const char* name, int value) {
  TC_CHECK(t != nullptr && name != nullptr, "NULL argument");
  // (streams and events created below, and the resident kernel stopped, belong to the table's
  // device whatever device is current in the calling thread)
  TC_HIP(hipSetDevice(t->device));
  const std::string key(name);
  if (key == "pipeline") {
    t->tuning.pipeline = value != 0;
  } else if (key == "deterministic") {
    // 0 (default): the fastest form per call -- chosen from the table, the flags, the entry
    // point and the batch size, never from timing (no self-measurement unless "autotune_after"
    // or "autotune" ask for it); 1: the same, and the measured dispatch is refused; 2:
    // batch-invariant -- ONE kernel form per (table, flags) for every entry point and batch
    // size (internal.h: Tuning::deterministic)
    TC_CHECK(value >= 0 && value <= 2, "deterministic must be 0, 1 or 2");
    int status = resident_stop(t);
    if (status != TC_OK) return status;
    for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
    t->tuning.deterministic = value;
    if (value != 0) {
      t->autotuned.clear();
      t->tuning.autotune_after = 0;
    }
  } else if (key == "autotune_after") {
    TC_CHECK(value == 0 || t->tuning.deterministic == 0,
             "autotune_after: the measured dispatch is not available while \"deterministic\" is set");
    // the N-th pipelined / asynchronous call with one combination of predict flags measures the
    // forms by itself (option "autotune": ~0.5 s, once); 0: never
    TC_CHECK(value >= 0, "autotune_after must be non-negative");
    t->tuning.autotune_after = value;
  } else if (key == "autotune") {
    // value = the predict flags to tune for (TC_FLAG_*; n_gauss_prim = 10), or -1: forget
    // every measured choice (back to the formula of hostmath.cpp: choose_fused_form)
    if (value < 0) {
      t->autotuned.clear();
      return TC_OK;
    }
    TC_CHECK(t->tuning.deterministic == 0,
             "autotune: the measured dispatch is not available while \"deterministic\" is set");
    return autotune(t, (unsigned)value);
  } else if (key == "resident_min_walkers") {
    // smallest ensemble the resident ensemble kernel takes (default 24; smaller ones go through
    // one launch of single_draw_kernel, which is faster for them)
    TC_CHECK(value >= 2 && value <= 256, "resident_min_walkers must be in [2, 256]");
    t->resident.min_walkers = value;
  } else if (key == "resident_wait_us") {
    // how long a workgroup of the resident ensemble kernel waits for another one inside a call
    // before it gives up (default 20 000; tests use 1 to exercise that path)
    TC_CHECK(value >= 1 && value <= 1000000, "resident_wait_us must be in [1, 1000000]");
    const int status = resident_stop(t);
    if (status != TC_OK) return status;
    t->resident.wait_us = value;
  } else if (key == "resident_aperture") {
    // 1 (default): the resident ensemble kernel's mailbox lies in device memory (large-BAR
    // systems; the host writes it through the PCIe aperture); 0: in page-locked host memory
    TC_CHECK(value == 0 || value == 1, "resident_aperture must be 0 or 1");
    const int status = resident_stop(t);
    if (status != TC_OK) return status;
    t->tuning.resident_aperture = value;
    t->resident.ens_grid = 0;          // (the buffers are chosen again at the next call)
    t->resident.single_aperture_decided = false;
  } else if (key == "cross_min_draws") {
    TC_CHECK(value >= 1, "cross_min_draws must be positive");
    t->tuning.cross_min_draws = value;
  } else if (key == "cross_defer") {
    // developer A/B: 0 = predict_cross_fused_kernel runs every lane's node loop in place
    t->tuning.cross_defer = value != 0;
  } else if (key == "fused_defer") {
    // developer A/B: 0 = predict_fused_kernel runs the satellites' node loops in place
    TC_CHECK(value >= 0 && value <= 2, "fused_defer must be 0, 1 or 2");
    t->tuning.fused_defer = value;
  } else if (key == "fused_skip") {
    // A/B and tests: 0 = predict_fused_kernel's matrix phase issues every product (same bits)
    TC_CHECK(value >= 0 && value <= 3, "fused_skip must be 0 .. 3");
    t->tuning.fused_skip = value;
  } else if (key == "fused_share") {
    // A/B and tests: the last r pass of the skipping instances with U = 3 or 5 as items of a
    // queue in LDS (same bits): 0 every wave its own, 1 eight items, 2 sixteen (one per group)
    TC_CHECK(value >= 0 && value <= 2, "fused_share must be 0, 1 or 2");
    t->tuning.fused_share = value;
  } else if (key == "fused_sat_cap") {
    TC_CHECK(value >= 0 && value <= 6, "fused_sat_cap must be in [0, 6]");
    t->tuning.fused_sat_cap = value;
  } else if (key == "cross_wide_min_draws") {
    // mode cross, tables of up to 16 rows: undecorated batches of this many draws take the
    // 32-row chunk form (launch.hip: choose_cross_fused); 0: never
    TC_CHECK(value >= 0, "cross_wide_min_draws must not be negative");
    t->tuning.cross_wide_min_draws = value;
  } else if (key == "cross_target") {
    // developer A/B: workgroups a launch of predict_cross_small_kernel should have at least
    TC_CHECK(value >= 1 && value <= 4096, "cross_target must be in [1, 4096]");
    t->tuning.cross_target = value;
  } else if (key == "series") {
    // bit 0: the node sum of an undecorated central bin by its moment expansion (csrc/series.h)
    // for every draw that allows it; bit 1: the binomial expansion of the satellite bins well
    // above a draw's M0; 0: always the node loops.  Per draw either way (a draw's bits do not
    // depend on its neighbours in the batch).
    TC_CHECK(value >= -1 && value <= 3, "series must be -1 .. 3");
    t->tuning.series = value;
  } else if (key == "grouped") {
    // 1 (default): bins that share their quadrature nodes -- the secondary-percentile bins of a
    // mass bin -- have the nodes' occupations evaluated once per group (kernels.hip.h:
    // occ_group_zheng07); 0: every bin by itself (A/B and tests: rounding-level differences
    // only in the sums over bins, none per bin)
    t->grouped = value != 0 && t->node_groups.largest > 1;
  } else if (key == "lanes") {
    TC_CHECK(value >= 1 && value <= (int)tc_table::kMaxLanes, "lanes must be in [1, %d]",
             (int)tc_table::kMaxLanes);
    for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
    for (int l = 0; l < value; ++l) {
      if (t->lanes[l].stream != nullptr) continue;
      TC_HIP(hipStreamCreateWithFlags(&t->lanes[l].stream, hipStreamNonBlocking));
      TC_HIP(hipEventCreateWithFlags(&t->lanes[l].finished, hipEventDisableTiming));
    }
    t->tuning.lanes = t->n_lanes = value;
    t->prev = -1;
  } else if (key == "ordered") {
    // 0 (default): every call only orders its own kernels (results land in the buffers the
    // caller passed; tc_table_synchronize and tc_comm_gather wait for every lane);
    // 1: the finalisations of consecutive device-pointer calls are chained by events, so
    // that a consumer waiting for the LAST call finds the earlier ones complete as well
    for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
    t->chain = value != 0;
    t->prev = -1;
  } else if (key == "sync_chunks") {
    // synchronous host calls (tc_predict_zheng07_batch, ...): 0 (default) cut batches of 2048
    // draws and more into up to 8 chunks whose uploads, kernels, downloads and host copies
    // overlap; N >= 1: N chunks for every batch (1: the same machinery, one piece); -1: the
    // serial path of rounds 1-4 (upload, kernels alone on one lane, download, copy)
    TC_CHECK(value >= -1 && value <= 64, "sync_chunks must be in [-1, 64]");
    t->tuning.sync_chunks = value;
  } else if (key == "sync_stagger") {
    // synchronous host calls with 16 MB of results and more run their chunks' kernels one after
    // the other, the chunks shrinking geometrically to this many per cent of the first
    // (default 10; 0: equal chunks on all lanes as for small results; plan_sync_chunks)
    TC_CHECK(value >= 0 && value <= 100, "sync_stagger must be in [0, 100]");
    t->tuning.sync_stagger = value;
  } else if (key == "sync_form") {
    TC_CHECK(value == 0 || value == 32 || value == 64, "sync_form must be 0, 32 or 64");
    t->tuning.sync_form = value;
  } else if (key == "sync_direct_out") {
    TC_CHECK(value >= 0 && value <= 2, "sync_direct_out must be 0, 1 or 2");
    t->tuning.sync_direct_out = value;
  } else if (key == "async_direct_in" || key == "async_direct_out") {
    // asynchronous host calls: 1 = the kernels read the draws from / write the results to
    // the caller's page-locked buffers themselves; 0 = copy commands on the lane's stream
    // (async_direct_out 2: only the number densities directly, xi by copy command)
    (key == "async_direct_in" ? t->tuning.async_direct_in : t->tuning.async_direct_out) =
        value;
  } else if (key == "fused") {
    // 0: always the three-kernel path; 1 (default): one launch per batch
    // (predict_fused_kernel) for pipelined device-pointer and asynchronous calls of
    // "fused_min_draws" .. "fused_max_draws" draws that it covers; 2: for every such call, also
    // those that run alone
    TC_CHECK(value >= 0 && value <= 2, "fused must be 0, 1 or 2");
    t->tuning.fused = value;
  } else if (key == "fused_min_draws" || key == "fused_max_draws") {
    TC_CHECK(value >= (key == "fused_min_draws" ? 0 : 1), "%s must be positive", name);
    (key == "fused_min_draws" ? t->tuning.fused_min_draws : t->tuning.fused_max_draws) = value;
  } else if (key == "resident") {
    // 1: un-batched calls (one draw, total correlation function, Zheng07 family) are served by
    // ONE resident launch that takes them from a mailbox in page-locked memory (launch.hip:
    // resident_predict); it leaves when idle for "resident_idle_us" and before any other kind
    // of call on this handle.  0 (default): one launch per call.
    // 2 (default): by itself for loops of un-batched calls -- from the eighth call on that
    // follows its predecessor within 300 us, with an idle time of 250 us, backing off when the
    // caller's pauses or device-wide synchronisations keep ending the launch.
    TC_CHECK(value >= 0 && value <= 2, "resident must be 0, 1 or 2");
    t->resident.enabled = value == 1;
    t->resident.auto_mode = value == 2;
    t->resident.auto_streak = t->resident.auto_backoff = 0;
    t->resident.auto_window = t->resident.auto_relaunches = 0;
    t->resident.auto_failures = 0;
    t->resident.ens_disabled = false;
    t->resident.ens_failures = 0;
    if (value != 1) return resident_stop(t);
  } else if (key == "resident_inject_failures") {
    // test hook: the next `value` calls that reach the resident single-draw kernel fail as if
    // the kernel kept leaving (the automatic mode must then serve them by launches)
    TC_CHECK(value >= 0, "resident_inject_failures must not be negative");
    t->resident.inject_failures = value;
  } else if (key == "resident_auto_idle_us") {
    TC_CHECK(value >= 10 && value <= 100000, "resident_auto_idle_us must be in [10, 100000]");
    const int status = resident_stop(t);
    if (status != TC_OK) return status;
    t->resident.auto_idle_us = value;
  } else if (key == "resident_poll_waves") {
    TC_CHECK(value >= 1 && value <= 4, "resident_poll_waves must be in [1, 4]");
    const int status = resident_stop(t);
    if (status != TC_OK) return status;
    t->resident.poll_waves = value;
  } else if (key == "resident_idle_us") {
    TC_CHECK(value >= 10 && value <= 1000000, "resident_idle_us must be in [10, 1000000]");
    const int status = resident_stop(t);
    if (status != TC_OK) return status;
    t->resident.idle_us = value;
  } else if (key == "fused_draws") {
    // (40: the latency form -- hostmath.cpp: choose_fused_form -- for every batch it serves)
    TC_CHECK(value == 0 || value == 32 || value == 40 || value == 64,
             "fused_draws must be 0, 32, 40 or 64");
    t->tuning.fused_draws = value;
  } else if (key == "fused_spread") {
    // 1 (default): calls that have the chip to themselves (host arrays, one lane, pipeline
    // off) take the latency form of the one-launch kernel where it serves them; 0: never
    t->tuning.fused_spread = value != 0;
  } else if (key == "fused_spread_min") {
    TC_CHECK(value >= 1, "fused_spread_min must be positive");
    t->tuning.fused_spread_min = value;
  } else if (key == "fused_spread_rounds") {
    TC_CHECK(value >= 1 && value <= 64, "fused_spread_rounds must be in [1, 64]");
    t->tuning.fused_spread_rounds = value;
  } else if (key == "fused_waves") {
    TC_CHECK(value == 0 || value == 8 || value == 16, "fused_waves must be 0, 8 or 16");
    t->tuning.fused_waves = value;
  } else if (key == "prio_fused") {
    t->tuning.prio_fused = value & 3;
  } else if (key == "prio_fused_occ") {
    t->tuning.prio_fused_occ = value & 3;
  } else if (key == "prio_fused_out") {
    t->tuning.prio_fused_out = value & 3;
  } else if (key == "single_draw") {
    t->tuning.single_draw = value != 0;
  } else if (key == "many_blocks") {
    TC_CHECK(value >= 2 && value <= 4096, "many_blocks must be in [2, 4096]");
    t->tuning.many_blocks = value;
  } else if (key == "single_round") {
    // (first table of an interpolator) 1: its un-batched call is sized so that all tables'
    // workgroups are on the chip at once; 0: one pass over the positions per workgroup
    t->tuning.single_round = value != 0;
  } else if (key == "poll_done") {
    // un-batched calls: 1 (default) poll the kernel's completion words in page-locked host
    // memory, 0 wait with hipStreamSynchronize
    t->tuning.poll_done = value != 0;
  } else if (key == "trace") {
    t->tuning.trace = value;
  } else if (key == "occ_splits" || key == "occ_per_cu" || key == "finalize_threads" ||
             key == "finalize_row_blocks") {
    // developer A/B: launch geometry of the occupation / finalisation kernels (0: chosen)
    TC_CHECK(value >= 0 && value <= 4096, "invalid value");
    (key == "occ_splits" ? t->tuning.occ_splits
     : key == "occ_per_cu" ? t->tuning.occ_per_cu
     : key == "finalize_threads" ? t->tuning.finalize_threads
                                 : t->tuning.finalize_row_blocks) = value;
  } else if (key == "prio_occ" || key == "prio_contract" || key == "prio_finalize") {
    // developer A/B: wave priorities (0..3) of the three kernels
    TC_CHECK(value >= 0 && value <= 3, "priorities are 0..3");
    (key == "prio_occ" ? t->tuning.prio_occ
                       : key == "prio_contract" ? t->tuning.prio_contract
                                                : t->tuning.prio_finalize) = value;
  } else if (key == "quad_merge" || key == "quad_waves" || key == "quad_order") {
    // developer A/B of the quadratic-form schedule: schedules are rebuilt on demand
    for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
    if (key == "quad_merge") t->tuning.quad_merge = value != 0;
    else if (key == "quad_order") t->tuning.quad_order = value;
    else t->tuning.quad_waves = t->tuning.quad_waves_f32 = value;
    for (tc::host::QuadTable* q : {&t->quad_by_type, &t->quad_total}) q->drop_schedules();
  } else {
    return fail(TC_ERR_INVALID, "unknown option '%s'", name);
  }
  return TC_OK;
}

int tc_table_timer_begin(tc_table* t, int profile_kernels) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  TC_HIP(hipSetDevice(t->device));
  t->profile_kernels = profile_kernels != 0;
  t->profile_every = profile_kernels > 1 ? profile_kernels : 1;
  t->profile_launches = 0;
  t->kernel_events_used = 0;
  TC_HIP(hipEventRecord(t->ev_begin, t->stream));
  return TC_OK;
}

int tc_table_timer_end(tc_table* t, float* elapsed_ms) {
  TC_CHECK(t != nullptr && elapsed_ms != nullptr, "NULL argument");
  for (int l = 1; l < tc_table::kMaxLanes; ++l)
    if (t->lanes[l].stream) TC_HIP(hipStreamSynchronize(t->lanes[l].stream));
  TC_HIP(hipEventRecord(t->ev_end, t->stream));
  TC_HIP(hipEventSynchronize(t->ev_end));
  TC_HIP(hipEventElapsedTime(elapsed_ms, t->ev_begin, t->ev_end));
  t->profile_kernels = false;
  return TC_OK;
}

int tc_table_kernel_time(tc_table* t, int* n_launches, float* mean_ms) {
  TC_CHECK(t != nullptr && n_launches && mean_ms, "NULL argument");
  double total = 0.0;
  for (size_t i = 0; i < t->kernel_events_used; ++i) {
    float ms = 0.0f;
    TC_HIP(hipEventSynchronize(t->kernel_events[i].second));
    TC_HIP(hipEventElapsedTime(&ms, t->kernel_events[i].first,
                               t->kernel_events[i].second));
    total += ms;
  }
  *n_launches = (int)t->kernel_events_used;
  *mean_ms = t->kernel_events_used ? (float)(total / t->kernel_events_used) : 0.0f;
  return TC_OK;
}

int tc_debug_trace(tc_table* t, uint64_t* out, int64_t capacity, int64_t* n_blocks) {
  TC_CHECK(t != nullptr && n_blocks != nullptr, "NULL argument");
  *n_blocks = (int64_t)t->trace_blocks;
  if (out == nullptr || t->trace.ptr == nullptr) return TC_OK;
  for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
  const int64_t n = std::min<int64_t>(capacity, (int64_t)t->trace_blocks);
  TC_HIP(hipMemcpy(out, t->trace.ptr, (size_t)n * 6 * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  return TC_OK;
}

int tc_debug_wave_trace(tc_table* t, uint64_t* out, int64_t capacity, int64_t* n_waves) {
  TC_CHECK(t != nullptr && n_waves != nullptr, "NULL argument");
  *n_waves = (int64_t)t->wave_trace_count;
  if (out == nullptr || t->wave_trace.ptr == nullptr) return TC_OK;
  for (tc_table::Lane& lane : t->lanes)
      if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
  const int64_t n = std::min<int64_t>(capacity, (int64_t)t->wave_trace_count);
  TC_HIP(hipMemcpy(out, t->wave_trace.ptr, (size_t)n * 6 * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  return TC_OK;
}

int tc_debug_resident_ticks(tc_table* t, uint64_t* out, int64_t capacity, int64_t* n_blocks) {
  TC_CHECK(t != nullptr && n_blocks != nullptr, "NULL argument");
  *n_blocks = t->resident.mailbox.ptr != nullptr ? t->resident.blocks : 0;
  if (out == nullptr || t->resident.mailbox.ptr == nullptr) return TC_OK;
  const unsigned long long* words = (const unsigned long long*)t->resident.mailbox.ptr;
  for (int64_t b = 0; b < std::min<int64_t>(capacity, *n_blocks); ++b)
    out[b] = words[16 + kSingleMaxBlocks + b];
  return TC_OK;
}

// Phase stamps of workgroup 0 in the last call of the resident ensemble kernel (developer
// builds; 100 MHz ticks: call seen, occupation stored, the group's occupations seen, densities
// in LDS, quarters summed, partial sums stored, [6] shader cycles of the quarter sums, call
// finished), then three host times of
// that call in ns: published, every row combined (from its begin), time spent on the rows.
int tc_debug_ensemble_stamps(tc_table* t, uint64_t* out) {
  TC_CHECK(t != nullptr && out != nullptr, "NULL argument");
  TC_CHECK(t->resident.ens_mailbox.ptr != nullptr, "no ensemble call has been made");
  const unsigned long long* words = (const unsigned long long*)t->resident.ens_mailbox.ptr;
  const size_t offset = 8 + (size_t)tc::kEnsembleMaxWalkers * 8 + t->resident.ens_grid;
  for (int i = 0; i < 8; ++i) out[i] = words[offset + i];
  for (int i = 0; i < 3; ++i) out[8 + i] = t->resident.ens_host_ns[i];
  return TC_OK;
}

int tc_table_last_launch(const tc_table* t, int* n_workgroups, int* waves,
                         int* n_splits, int* lds_bytes) {
  TC_CHECK(t != nullptr, "table handle is NULL");
  if (n_workgroups) *n_workgroups = t->last_workgroups;
  if (waves) *waves = t->last_waves;
  if (n_splits) *n_splits = t->last_splits;
  if (lds_bytes) *lds_bytes = t->last_lds;
  return TC_OK;
}

}  // extern "C"
