// Interpolator handle of the C ABI (include/tabcorr_amd.h): tensor-product cubic-spline
// interpolation over a grid of tables, evaluated as one contraction over all tables
// (tabcorr/interpolator.py:136-219).
#include "internal.h"
#include "spline.h"

using namespace tc::host;

struct tc_interp {
  int device = 0;
  int n_tables = 0;
  int n_dim = 0;
  std::vector<tc_table*> tables;
  std::vector<std::vector<double>> xp;      // per dimension
  std::vector<int32_t> table_node;          // (K, D)
  std::vector<int32_t> table_class;         // (K)
  std::vector<int> class_table;             // representative table of each class
  void* d_xp = nullptr;
  void* d_a = nullptr;
  void* d_table_node = nullptr;
  void* d_table_class = nullptr;
  void* d_tables = nullptr;                 // (K) device pointers
  void* d_quad_by_type = nullptr;           // (K) matrices of the quadratic-form kernel
  void* d_quad_total = nullptr;             // (K) ... unpadded triangle, if the tables have it
  std::vector<int> axis_offset, a_offset;
  std::vector<double> a_host;               // spline matrices of all dimensions
  // un-batched calls: per n_gauss the per-class pointer arrays of single_draw_kernel
  struct SinglePointers {
    void* log_m = nullptr;
    void* m = nullptr;
    void* weight = nullptr;
    void* n_h = nullptr;
    void* percentile = nullptr;
  };
  std::map<int, SinglePointers> single_pointers;
  // gradients (grad_interp_kernels.hip.h), built at the first gradient call: the walk over the
  // tables -- class by class, inside a class in list order -- as the grid node and the gradient
  // matrix (launch.hip: build_grad_table) of every table in walk order
  struct GradWalk {
    bool built = false;
    void* class_begin = nullptr;              // (classes + 1)
    void* node = nullptr;                     // (K, D)
    void* matrices = nullptr;                 // (K) device pointers
    void* class_n_h = nullptr;                // (classes) device pointers: n_h of every class
  };
  GradWalk grad_walk;
  // Lanes (stream + workspaces), as for a table handle: consecutive device-pointer and
  // asynchronous calls alternate between them, so that the occupation / spline-weight /
  // finalisation kernels and the ramps of one call's contraction hide behind the
  // neighbour's (BASELINE configs[3], 12 500 draws: 992 -> 929 us per call).  Host-buffer
  // calls use lane 0.
  struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t finished = nullptr;            // recorded by the gather, not per call
    std::vector<DeviceBuffer> nbuf, ngal2;    // per class
    std::vector<DeviceBuffer> nbuf32;         // per class: float copies (float32 quadratic form)
    std::vector<void*> nbuf_ptrs, ngal_ptrs, nbuf32_ptrs;   // last uploaded pointer values
    void* d_nbufs = nullptr;                  // (V) device pointers
    void* d_ngal_parts = nullptr;             // (V) device pointers
    void* d_nbufs32 = nullptr;                // (V) ... float copies of the densities
    DeviceBuffer coef, partial, chi2_xi;
    DeviceBuffer cross_counters;              // mode cross, several workgroups per tile
    DeviceBuffer stage_in, stage_out;         // asynchronous host calls
  };
  static constexpr int kLanes = 4;
  Lane lanes[kLanes];
  // Lanes in use: two for the three-kernel forms (their contraction fills the chip by itself),
  // four in mode cross, where a launch of predict_cross_fused_kernel is one workgroup per 64
  // draws and only several launches in flight fill the CUs (the reference's AbacusSummit
  // interpolator, 10^4 draws per call: 143 us per call with two lanes)
  int n_lanes = 2;
  int cur = 0;                                // lane of the last call (tc_comm_gather_interp)
  uint64_t device_calls = 0;
  hipStream_t stream = nullptr;               // = lanes[0].stream
  DeviceBuffer theta, x, out_ngal, out_xi;  // host-buffer calls
  Chi2Operands chi2;                        // likelihood: data + precision
  PinnedBuffer h_in, h_out;
  SingleWorkspace single_ws;                // un-batched calls
  std::map<std::pair<int, int>, std::unique_ptr<DeviceChunking>> chunkings;
  CrossFused cross_fused, cross_fused_wide; // mode cross: one launch per batch (launch.hip)
  Tickets tickets;                          // of the asynchronous host calls (tc_interp_*_async)
};

namespace {

// Data vector and precision matrix of a likelihood on the device (internal.h: Chi2Operands):
// before new values go up, everything queued on the interpolator is waited for.
int upload_operands(tc_interp* it, const double* data, const double* precision) {
  return it->chi2.upload(it->tables[0]->n_r, data, precision, it->stream,
                         [it] { return tc_interp_synchronize(it); });
}

// One slab of an interpolated prediction as `call` describes it (internal.h: its lane is one of
// the interpolator's, its options the first table's).
int interp_predict_slab(tc_interp* it, const Call& call, const double* theta_device, int n_theta,
                        const double* x_device, int64_t n_draws, int n_gauss,
                        unsigned flags, double* ngal_device, double* xi_device,
                        bool* chi2_written) {
  tc_table* t0 = it->tables[0];
  tc_interp::Lane& L = it->lanes[call.lane];
  const bool separate = (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0;
  const int n_comp = separate ? t0->plan.n_components : 1;
  const int n_classes = (int)it->class_table.size();
  const int64_t ldb = (n_draws + 63) / 64 * 64;
  int status = TC_OK;

  // mode cross: everything in one launch where it pays (predict_cross_fused_kernel)
  if (t0->mode == TC_MODE_CROSS && !t0->cross_host.empty() && t0->tuning.fused != 0) {
    const CrossFused& cf =
        *choose_cross_fused(it->tables.data(), it->n_tables, &it->cross_fused,
                            &it->cross_fused_wide, n_draws, flags, &status);
    if (status != TC_OK) return status;
    if (cross_fused_eligible(t0, call, cf, n_draws, n_gauss, flags)) {
      tc::CrossFusedArgs ca{};
      ca.n_dim = it->n_dim;
      for (int d = 0; d < it->n_dim; ++d) {
        ca.n_axis[d] = (int)it->xp[d].size();
        ca.axis_offset[d] = it->axis_offset[d];
        ca.a_offset[d] = it->a_offset[d];
      }
      ca.xp = (const double*)it->d_xp;
      ca.a = (const double*)it->d_a;
      ca.table_node = (const int32_t*)it->d_table_node;
      ca.x = x_device;
      return run_cross_fused(t0, call, cf, &ca, theta_device, n_theta, n_draws, flags, ngal_device,
                             xi_device, L.stream, &L.partial, &L.cross_counters, chi2_written);
    }
  }

  // occupations once per class of identical halo tables (interpolator.py:181-184)
  int ngal_parts = 1;
  const bool quad_f32 = t0->quad && t0->compute_dtype == TC_DTYPE_F32;
  for (int v = 0; v < n_classes; ++v) {
    // (the shape of a class's occupation launch follows that table's own options, not the call's)
    tc_table* t = it->tables[it->class_table[v]];
    status = run_occupation(t, probe_call(t), theta_device, n_theta, n_draws, ldb, n_gauss, flags,
                            nullptr, &L.nbuf[v], &L.ngal2[v], L.stream, &ngal_parts,
                            quad_f32 ? &L.nbuf32[v] : nullptr);
    if (status != TC_OK) return status;
  }
  bool moved = false;
  for (int v = 0; v < n_classes; ++v) {
    moved = moved || L.nbuf_ptrs[v] != L.nbuf[v].ptr ||
            L.ngal_ptrs[v] != L.ngal2[v].ptr || L.nbuf32_ptrs[v] != L.nbuf32[v].ptr;
    L.nbuf_ptrs[v] = L.nbuf[v].ptr;
    L.ngal_ptrs[v] = L.ngal2[v].ptr;
    L.nbuf32_ptrs[v] = L.nbuf32[v].ptr;
  }
  if (moved) {
    TC_HIP(hipMemcpyAsync(L.d_nbufs32, L.nbuf32_ptrs.data(), n_classes * sizeof(void*),
                          hipMemcpyHostToDevice, L.stream));
    TC_HIP(hipMemcpyAsync(L.d_nbufs, L.nbuf_ptrs.data(), n_classes * sizeof(void*),
                          hipMemcpyHostToDevice, L.stream));
    TC_HIP(hipMemcpyAsync(L.d_ngal_parts, L.ngal_ptrs.data(),
                          n_classes * sizeof(void*), hipMemcpyHostToDevice, L.stream));
    TC_HIP(hipStreamSynchronize(L.stream));   // the host vectors may change later
  }

  status = L.coef.reserve((size_t)it->n_tables * ldb * sizeof(double), L.stream);
  if (status != TC_OK) return status;
  tc::InterpArgs ia{};
  ia.n_dim = it->n_dim;
  ia.n_tables = it->n_tables;
  ia.n_classes = n_classes;
  ia.mode = t0->mode;
  ia.separate = separate ? 1 : 0;
  for (int d = 0; d < it->n_dim; ++d) {
    ia.n_axis[d] = (int)it->xp[d].size();
    ia.axis_offset[d] = it->axis_offset[d];
    ia.a_offset[d] = it->a_offset[d];
  }
  ia.xp = (const double*)it->d_xp;
  ia.a = (const double*)it->d_a;
  ia.table_node = (const int32_t*)it->d_table_node;
  ia.table_class = (const int32_t*)it->d_table_class;
  ia.x = x_device;
  ia.ngal_parts = (const double* const*)L.d_ngal_parts;
  ia.n_ngal_parts = ngal_parts;
  ia.ldb = ldb;
  ia.n_draws = n_draws;
  ia.coef = (double*)L.coef.ptr;
  ia.ngal = ngal_device;
  {
    Range range("spline weights");
    status = launch_interp_coef(ia, L.stream);
  }
  if (status != TC_OK) return status;
  Range range("contraction + finalisation (all tables)");

  if (t0->quad) {
    // quadratic-form kernel: the unit space (draw tile, r tile, component, TABLE, unit) in
    // equal shares per wave; a table's spline weight scales the outer factor n_i
    const bool by_type = separate || t0->quad_total.d_table == nullptr;
    QuadTable* q = by_type ? &t0->quad_by_type : &t0->quad_total;
    const tc::QuadTiling& tiling = t0->quad_tiling;
    DeviceQuadSchedule* schedule = nullptr;
    const int tile_draws = quad_f32 ? tc::kQuadTileF32 : tc::kQuadTile;
    status = get_quad_schedule(t0, q, ldb / tile_draws, it->n_tables, separate, &schedule);
    if (status != TC_OK) return status;
    const int rt = 4 * tiling.n_u;
    status = L.partial.reserve((size_t)schedule->n_slabs * rt * tile_draws *
                                     (quad_f32 ? sizeof(float) : sizeof(double)),
                                 L.stream);
    if (status != TC_OK) return status;
    tc::QuadArgs qa{};
    qa.nbuf = nullptr;
    qa.nbufs = (const double* const*)L.d_nbufs;
    qa.nbufs32 = (const float* const*)L.d_nbufs32;
    qa.ldb = ldb;
    qa.n_bins = t0->n_bins;
    qa.table = nullptr;
    qa.tables = (const double* const*)(by_type ? it->d_quad_by_type : it->d_quad_total);
    qa.table_class = (const int32_t*)it->d_table_class;
    qa.coef = (const double*)L.coef.ptr;
    qa.rtile_bytes = (uint32_t)q->rtile_bytes;
    qa.runs = (const tc::QuadRun*)schedule->runs;
    qa.comps = (const tc::QuadCompArgs*)q->d_comps;
    qa.wave_runs = (const int32_t*)schedule->wave_runs;
    qa.wave_head = (const int32_t*)schedule->wave_head;
    qa.n_waves = schedule->n_waves;
    qa.partial = L.partial.ptr;
    qa.priority = t0->tuning.prio_contract;
    qa.merge_range = (const int32_t*)schedule->merge_range;
    qa.merges = (const int32_t*)schedule->merges;
    qa.stamps = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr;     // timed through the first table's timer
    status = next_kernel_events(t0, &k0, &k1);
    if (status != TC_OK) return status;
    status = launch_contract_quad(tiling.n_u, quad_f32 ? TC_DTYPE_F32 : TC_DTYPE_F64, true, qa,
                                  schedule->lds_bytes, L.stream, k0, k1);
    if (status != TC_OK) return status;
    t0->last_workgroups = (schedule->n_waves + tc::kQuadWavesPerBlock - 1) / tc::kQuadWavesPerBlock;
    t0->last_waves = tc::kQuadWavesPerBlock;
    t0->last_splits = schedule->n_slabs;
    t0->last_lds = schedule->lds_bytes;
    tc::FinalizeQuadArgs fq{};
    fq.partial = L.partial.ptr;
    fq.group_begin = (const int32_t*)schedule->group_begin;
    fq.ngal_part = nullptr;      // already normalised; ngal written by the coef kernel
    fq.n_ngal_parts = 0;
    fq.n_rtiles = tiling.n_rtiles;
    fq.r_per_tile = tiling.r_per_tile;
    fq.rt = rt;
    fq.groups_per_rtile = separate ? (int)q->layout.comps.size() : 1;
    fq.priority = t0->tuning.prio_finalize;
    fq.n_comp = n_comp;
    fq.n_r = t0->n_r;
    fq.mode = t0->mode;
    fq.ldb = ldb;
    fq.n_draws = n_draws;
    fq.ngal = ngal_device;
    fq.xi = xi_device;
    if (call.chi2_out != nullptr && !separate && t0->n_r <= tc::kFinalizeRows) {
      // (launch.hip, run_contraction_quad: the likelihood from the finalisation's LDS tile)
      fq.chi2_data = call.chi2_data;
      fq.chi2 = call.chi2_out;
      fq.xi = nullptr;
      *chi2_written = true;
    }
    return launch_finalize_quad(fq, t0->tuning, L.stream, quad_f32);
  }

  // decomposition: as for one table (choose_chunking), with the tables looped inside
  // the block; the tables are split over blocks only when one pass would leave the chip
  // underfilled
  const int64_t n_tiles = ldb / 64;
  DeviceChunking* c = nullptr;
  int lds = 0;
  {
    // the table handle caches the chunkings; all tables share table 0's plan
    status = choose_chunking(t0, n_draws, std::min(it->n_tables, 1000), &c, &lds);
    if (status != TC_OK) return status;
  }
  int k_splits = 1;
  {
    const int64_t blocks = n_tiles * t0->n_rtiles * (int64_t)c->host.groups.size();
    const int64_t want = t0->n_cus * (int64_t)blocks_per_cu(lds, c->host.waves_per_group,
                                                        wave_slots(t0, true));
    // about two scheduling rounds of blocks (measured optimum for 16 tiles x 20 groups x
    // 25 tables: 3 splits); every split adds a slab the finalisation has to sum
    if (blocks < want)
      k_splits = (int)std::min<int64_t>(
          it->n_tables, std::max<int64_t>(1, 2 * want / std::max<int64_t>(1, blocks)));
    if (t0->tuning.k_splits > 0) k_splits = t0->tuning.k_splits;
    k_splits = std::min(k_splits, it->n_tables);
  }
  if (lds > kMaxLdsBytes)
    return fail(TC_ERR_UNSUPPORTED, "table with %d bins needs %d bytes of LDS",
                t0->n_bins, lds);
  const int n_groups = (int)c->host.groups.size();
  const int r_stride = t0->rt * t0->n_rtiles;
  status = L.partial.reserve(
      (size_t)n_groups * k_splits * r_stride * ldb * sizeof(double), L.stream);
  if (status != TC_OK) return status;

  tc::ContractArgs ca{};
  ca.nbuf = nullptr;
  ca.ldb = ldb;
  ca.table = nullptr;
  ca.n_positions = t0->plan.n_positions;
  ca.chunks = (const tc::Chunk*)c->chunks;
  ca.groups = (const tc::Group*)c->groups;
  ca.mode = t0->mode;
  ca.n_central = t0->plan.n_central;
  ca.r_stride = r_stride;
  ca.trace = nullptr;
  ca.wave_trace = nullptr;
  ca.pos_ij = nullptr;
  ca.pos_off = (const int32_t*)t0->d_pos_off;
  ca.partial = (double*)L.partial.ptr;
  ca.n_tables = it->n_tables;
  ca.k_splits = k_splits;
  ca.tables = (const double* const*)it->d_tables;
  ca.nbufs = (const double* const*)L.d_nbufs;
  ca.table_class = (const int32_t*)it->d_table_class;
  ca.coef = (const double*)L.coef.ptr;
  ca.n_tiles = (int)n_tiles;
  ca.n_slabs = n_groups * k_splits;
  ca.xcd_map = t0->n_xcds == 8 && n_tiles >= 8;
  const int64_t padded_tiles = ca.xcd_map ? (n_tiles + 7) / 8 * 8 : n_tiles;
  dim3 grid((unsigned)(padded_tiles * n_groups * k_splits), 1,
            (unsigned)t0->n_rtiles);
  dim3 block(64 * c->host.waves_per_group);
  hipEvent_t k0 = nullptr, k1 = nullptr;       // timed through the first table's timer
  status = next_kernel_events(t0, &k0, &k1);
  if (status != TC_OK) return status;
  if (t0->compute_dtype == TC_DTYPE_F32) {
    ca.pos_ij = (const int32_t*)t0->d_pos_ij;
    status = launch_contract_f32(t0->device, grid, block, lds, L.stream, ca, k0, k1);
  } else {
    status = launch_contract_rt(t0->rt, t0->device, grid, block, lds, L.stream, ca, k0, k1);
  }
  if (status != TC_OK) return status;
  t0->last_workgroups = (int)(grid.x * grid.z);
  t0->last_waves = c->host.waves_per_group;
  t0->last_splits = n_groups * k_splits;
  t0->last_lds = lds;

  tc::FinalizeArgs fa{};
  fa.partial = (const double*)L.partial.ptr;
  fa.groups = (const tc::Group*)c->groups;
  fa.ngal_part = nullptr;      // already normalised; ngal written by the coef kernel
  fa.n_ngal_parts = 0;
  fa.n_groups = n_groups;
  fa.k_splits = k_splits;
  fa.n_comp = n_comp;
  fa.r_stride = r_stride;
  fa.n_r = t0->n_r;
  fa.mode = t0->mode;
  fa.ldb = ldb;
  fa.n_draws = n_draws;
  fa.ngal = ngal_device;
  fa.xi = xi_device;
  return launch_finalize(fa, t0->tuning, L.stream);
}

// A call of the interpolator on its next lane (internal.h: make_call), the options its first
// table's.
Call interp_call(tc_interp* it, bool pinned) {
  const tc_table* t0 = it->tables[0];
  return make_call(t0, next_lane(pinned, t0->tuning.pipeline != 0, it->n_lanes,
                                 &it->device_calls), pinned, it->n_lanes);
}

// A prediction of n_draws > 0 draws on device pointers as `call` describes it (the arguments are
// checked): tc_interp_predict_zheng07_batch_device, and the host-array and asynchronous entry
// points underneath.  *chi2_written: the launch wrote the call's likelihood itself.
int interp_predict_device(tc_interp* it, const Call& call, const double* theta_device,
                          int n_theta, const double* x_device, int64_t n_draws, int n_gauss,
                          unsigned flags, double* ngal_device, double* xi_device,
                          bool* chi2_written = nullptr) {
  TC_HIP(hipSetDevice(it->device));
  const bool separate = (flags & TC_FLAG_SEPARATE_GAL_TYPE) != 0;
  const int n_comp = separate ? it->tables[0]->plan.n_components : 1;
  it->cur = call.lane;
  return for_each_slab(n_draws, max_slab(it->tables[0]), [&](int64_t begin, int64_t n) {
    return interp_predict_slab(it, call, theta_device + begin * n_theta, n_theta,
                               x_device + begin * it->n_dim, n, n_gauss, flags,
                               ngal_device + begin * (separate ? 2 : 1),
                               xi_device + begin * n_comp * it->tables[0]->n_r, chi2_written);
  });
}

// A likelihood of n_draws > 0 draws on device pointers as `call` describes it (the arguments are
// checked): tc_interp_chi2_zheng07_batch_device and the entry points underneath.
int interp_chi2_device(tc_interp* it, Call call, const double* theta_device, int n_theta,
                       const double* x_device, int64_t n_draws, int n_gauss, unsigned flags,
                       const double* data, const double* precision, double* ngal_device,
                       double* chi2_device) {
  TC_HIP(hipSetDevice(it->device));
  tc_table* t0 = it->tables[0];
  const int n_r = t0->n_r;
  tc_interp::Lane& L = it->lanes[call.lane];
  int status = upload_operands(it, data, precision);
  if (status != TC_OK) return status;
  status = L.chi2_xi.reserve((size_t)n_draws * n_r * 8, L.stream);
  if (status != TC_OK) return status;
  call.chi2_data = it->chi2.device();
  call.chi2_out = n_draws <= max_slab(t0) ? chi2_device : nullptr;   // (one slab)
  bool written = false;
  status = interp_predict_device(it, call, theta_device, n_theta, x_device, n_draws, n_gauss,
                                 flags, ngal_device, (double*)L.chi2_xi.ptr, &written);
  if (status != TC_OK || written) return status;
  return launch_chi2((const double*)L.chi2_xi.ptr, n_draws, n_r, call.chi2_data,
                     call.chi2_data + n_r, chi2_device, L.stream);
}

}  // namespace

namespace tc {
namespace host {
hipStream_t interp_stream(tc_interp* interp) { return interp->lanes[interp->cur].stream; }
// Everything queued so far on every lane of the interpolator precedes what is queued on
// `stream` afterwards (tc_comm_gather_interp) / every lane waits for `event`
// (tc_comm_release_interp).
int interp_join_lanes(tc_interp* interp, hipStream_t stream) {
  for (tc_interp::Lane& lane : interp->lanes) {
    if (lane.stream == nullptr) continue;
    TC_HIP(hipEventRecord(lane.finished, lane.stream));
    TC_HIP(hipStreamWaitEvent(stream, lane.finished, 0));
  }
  return TC_OK;
}
int interp_lanes_wait(tc_interp* interp, hipEvent_t event) {
  for (tc_interp::Lane& lane : interp->lanes)
    if (lane.stream != nullptr) TC_HIP(hipStreamWaitEvent(lane.stream, event, 0));
  return TC_OK;
}
}  // namespace host
}  // namespace tc

extern "C" {

int tc_interp_create(tc_table* const* tables, int n_tables, int n_dim,
                     const double* points, tc_interp** out) {
  TC_CHECK(out != nullptr, "interp output pointer is NULL");
  *out = nullptr;
  TC_CHECK(tables != nullptr && points != nullptr, "NULL argument");
  TC_CHECK(n_tables >= 1 && n_dim >= 1 && n_dim <= tc::kMaxInterpDim,
           "invalid number of tables or dimensions");
  struct Destroy {
    void operator()(tc_interp* interp) const { tc_interp_destroy(interp); }
  };
  std::unique_ptr<tc_interp, Destroy> it(new tc_interp);
  TC_HIP(hipGetDevice(&it->device));
  it->n_tables = n_tables;
  it->n_dim = n_dim;
  it->tables.assign(tables, tables + n_tables);
  tc_table* t0 = tables[0];
  for (int k = 0; k < n_tables; ++k) {
    tc_table* t = tables[k];
    TC_CHECK(t != nullptr, "table %d is NULL", k);
    TC_CHECK(t->device == it->device, "table %d lives on another device", k);
    TC_CHECK(t->compute_dtype == t0->compute_dtype,
             "table %d differs from table 0 in compute dtype", k);
    TC_CHECK(t->mode == t0->mode && t->n_bins == t0->n_bins && t->n_r == t0->n_r &&
                 t->plan.perm == t0->plan.perm,
             "table %d differs from table 0 in mode, shape or gal_type layout", k);
  }
  // abscissae: sorted unique values per dimension (interpolator.py:41-43)
  int64_t grid_size = 1;
  std::vector<double> xp_all, a_all;
  for (int d = 0; d < n_dim; ++d) {
    std::vector<double> xp;
    for (int k = 0; k < n_tables; ++k) xp.push_back(points[(size_t)k * n_dim + d]);
    std::sort(xp.begin(), xp.end());
    xp.erase(std::unique(xp.begin(), xp.end()), xp.end());
    TC_CHECK((int)xp.size() <= tc::kMaxInterpAxis, "more than %d grid values in "
             "dimension %d", tc::kMaxInterpAxis, d);
    // interpolator.py:239-241
    TC_CHECK(xp.size() >= 4,
             "Cannot perform spline interpolation with less than 4 values.");
    std::vector<double> a;
    TC_CHECK(tc::spline_interpolation_matrix((int)xp.size(), xp.data(), a),
             "singular spline system in dimension %d", d);
    it->axis_offset.push_back((int)xp_all.size());
    it->a_offset.push_back((int)a_all.size());
    xp_all.insert(xp_all.end(), xp.begin(), xp.end());
    a_all.insert(a_all.end(), a.begin(), a.end());
    grid_size *= (int64_t)xp.size();
    it->xp.push_back(xp);
  }
  // the points must form the full grid, each node once (interpolator.py:45-57)
  TC_CHECK(grid_size == n_tables, "The 'param_dict_table' does not describe a grid.");
  std::vector<char> taken((size_t)grid_size, 0);
  it->table_node.resize((size_t)n_tables * n_dim);
  for (int k = 0; k < n_tables; ++k) {
    int64_t flat = 0;
    for (int d = 0; d < n_dim; ++d) {
      const std::vector<double>& xp = it->xp[d];
      const int node = (int)(std::lower_bound(xp.begin(), xp.end(),
                                              points[(size_t)k * n_dim + d]) -
                             xp.begin());
      it->table_node[(size_t)k * n_dim + d] = node;
      flat = flat * (int64_t)xp.size() + node;
    }
    TC_CHECK(!taken[flat], "The 'param_dict_table' does not describe a grid.");
    taken[flat] = 1;
  }
  // classes of identical halo tables share their occupations (interpolator.py:63-70)
  it->table_class.assign(n_tables, -1);
  for (int k = 0; k < n_tables; ++k) {
    for (size_t v = 0; v < it->class_table.size(); ++v) {
      if (same_bins(tables[k], tables[it->class_table[v]])) {
        it->table_class[k] = (int32_t)v;
        break;
      }
    }
    if (it->table_class[k] < 0) {
      it->table_class[k] = (int32_t)it->class_table.size();
      it->class_table.push_back(k);
    }
  }
  const size_t n_classes = it->class_table.size();
  for (tc_interp::Lane& lane : it->lanes) {
    lane.nbuf.resize(n_classes);
    lane.ngal2.resize(n_classes);
    lane.nbuf32.resize(n_classes);
    lane.nbuf_ptrs.assign(n_classes, nullptr);
    lane.ngal_ptrs.assign(n_classes, nullptr);
    lane.nbuf32_ptrs.assign(n_classes, nullptr);
    TC_HIP(hipEventCreateWithFlags(&lane.finished, hipEventDisableTiming));
  }
  {
    hipStream_t streams[tc_interp::kLanes] = {};
    const int created = create_lane_streams(tc_interp::kLanes, streams);
    for (int l = 0; l < tc_interp::kLanes; ++l) it->lanes[l].stream = streams[l];
    if (created != TC_OK) return created;
  }
  it->stream = it->lanes[0].stream;
  it->n_lanes = t0->mode == TC_MODE_CROSS ? tc_interp::kLanes : 2;
  std::vector<void*> table_ptrs;
  for (int k = 0; k < n_tables; ++k) table_ptrs.push_back(tables[k]->d_table);
  std::vector<void*> zeros(n_classes, nullptr);
  std::vector<void*> quad_by_type, quad_total;
  for (int k = 0; k < n_tables; ++k) {
    quad_by_type.push_back(tables[k]->quad_by_type.d_table);
    quad_total.push_back(tables[k]->quad_total.d_table);
  }
  int status = upload(xp_all, &it->d_xp);
  if (status == TC_OK) status = upload(quad_by_type, &it->d_quad_by_type);
  if (status == TC_OK) status = upload(quad_total, &it->d_quad_total);
  it->a_host = a_all;
  if (status == TC_OK) status = upload(a_all, &it->d_a);
  if (status == TC_OK) status = upload(it->table_node, &it->d_table_node);
  if (status == TC_OK) status = upload(it->table_class, &it->d_table_class);
  if (status == TC_OK) status = upload(table_ptrs, &it->d_tables);
  for (tc_interp::Lane& lane : it->lanes) {
    if (status == TC_OK) status = upload(zeros, &lane.d_nbufs);
    if (status == TC_OK) status = upload(zeros, &lane.d_nbufs32);
    if (status == TC_OK) status = upload(zeros, &lane.d_ngal_parts);
  }
  if (status != TC_OK) return status;
  *out = it.release();
  return TC_OK;
}

int tc_interp_destroy(tc_interp* it) {
  if (it == nullptr) return TC_OK;
  (void)hipSetDevice(it->device);
  for (tc_interp::Lane& lane : it->lanes)
    if (lane.stream) (void)hipStreamSynchronize(lane.stream);
  for (void* p : {it->d_xp, it->d_a, it->d_table_node, it->d_table_class, it->d_tables,
                  it->d_quad_by_type, it->d_quad_total})
    if (p) (void)hipFree(p);
  for (auto& kv : it->chunkings)
    for (void* p : {kv.second->chunks, kv.second->groups})
      if (p) (void)hipFree(p);
  for (auto& kv : it->single_pointers)
    for (void* p : {kv.second.log_m, kv.second.m, kv.second.weight, kv.second.n_h,
                    kv.second.percentile})
      if (p) (void)hipFree(p);
  for (void* p : {it->grad_walk.class_begin, it->grad_walk.node, it->grad_walk.matrices,
                  it->grad_walk.class_n_h})
    if (p) (void)hipFree(p);
  for (tc_interp::Lane& lane : it->lanes) {
    for (void* p : {lane.d_nbufs, lane.d_nbufs32, lane.d_ngal_parts})
      if (p) (void)hipFree(p);
    for (DeviceBuffer& b : lane.nbuf) b.release();
    for (DeviceBuffer& b : lane.ngal2) b.release();
    for (DeviceBuffer& b : lane.nbuf32) b.release();
    for (DeviceBuffer* b : {&lane.coef, &lane.partial, &lane.chi2_xi, &lane.stage_in,
                            &lane.stage_out, &lane.cross_counters})
      b->release();
    if (lane.finished) (void)hipEventDestroy(lane.finished);
  }
  for (DeviceBuffer* b : {&it->theta, &it->x, &it->out_ngal, &it->out_xi, &it->chi2.buffer})
    b->release();
  it->cross_fused.release();
  it->cross_fused_wide.release();
  it->h_in.release();
  it->h_out.release();
  it->single_ws.buffer.release();
  it->tickets.release();
  for (tc_interp::Lane& lane : it->lanes)
    if (lane.stream) (void)hipStreamDestroy(lane.stream);
  delete it;
  return TC_OK;
}

int tc_interp_synchronize(tc_interp* it) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  for (tc_interp::Lane& lane : it->lanes)
    if (lane.stream) TC_HIP(hipStreamSynchronize(lane.stream));
  return TC_OK;
}

int tc_interp_axis(const tc_interp* it, int dim, int* n, double* xp, int size) {
  TC_CHECK(it != nullptr && n != nullptr, "NULL argument");
  TC_CHECK(dim >= 0 && dim < it->n_dim, "invalid dimension %d", dim);
  *n = (int)it->xp[dim].size();
  if (xp != nullptr)
    for (int i = 0; i < std::min(*n, size); ++i) xp[i] = it->xp[dim][i];
  return TC_OK;
}

int tc_interp_predict_zheng07_batch_device(tc_interp* it, const double* theta_device,
                                           int n_theta, const double* x_device,
                                           int64_t n_draws, int n_gauss, unsigned flags,
                                           double* ngal_device, double* xi_device) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  int status = check_predict_args(it->tables[0], theta_device, n_theta, n_draws,
                                  n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(x_device && ngal_device && xi_device, "NULL pointer");
  return interp_predict_device(it, interp_call(it, /*pinned=*/false), theta_device, n_theta,
                               x_device, n_draws, n_gauss, flags, ngal_device, xi_device);
}

namespace {

// Per class the device pointers of its quadrature constants for n_gauss nodes, n_h and
// percentiles, as device arrays (made once per n_gauss).
int class_pointers(tc_interp* it, int n_gauss, const tc_interp::SinglePointers** out) {
  auto found = it->single_pointers.find(n_gauss);
  if (found == it->single_pointers.end()) {
    std::vector<void*> log_m, m, weight, n_h, percentile;
    for (int table : it->class_table) {
      tc_table* t = it->tables[table];
      Quadrature* q = nullptr;
      int status = get_quadrature(t, n_gauss, &q);
      if (status != TC_OK) return status;
      log_m.push_back(q->log_m);
      m.push_back(q->m);
      weight.push_back(q->weight);
      n_h.push_back(t->d_n_h);
      percentile.push_back(t->d_percentile);
    }
    tc_interp::SinglePointers p;
    int status = upload(log_m, &p.log_m);
    if (status == TC_OK) status = upload(m, &p.m);
    if (status == TC_OK) status = upload(weight, &p.weight);
    if (status == TC_OK) status = upload(n_h, &p.n_h);
    if (status == TC_OK) status = upload(percentile, &p.percentile);
    if (status != TC_OK) return status;
    found = it->single_pointers.emplace(n_gauss, p).first;
  }
  *out = &found->second;
  return TC_OK;
}

// Un-batched Interpolator.predict: ONE launch evaluates every table (single_draw_kernel
// with grid = tables x workgroups per table, each workgroup computing the occupations of
// its table's class itself), the partial sums land in page-locked host memory, and the
// host normalises each table, forms the tensor-product spline weights
// (interpolator.py:275-331) and adds the tables in list order.  No device-side
// combination, no second launch: ~25 us against ~70 us for the four-launch batched path.
int interp_predict_one(tc_interp* it, const double* theta, int n_theta, const double* x,
                       int n_gauss, unsigned flags, double* ngal, double* xi) {
  tc_table* t0 = it->tables[0];
  const tc_interp::SinglePointers* pointers = nullptr;
  int status = class_pointers(it, n_gauss, &pointers);
  if (status != TC_OK) return status;
  const tc_interp::SinglePointers& p = *pointers;
  const int rt = t0->rt, n_tables = it->n_tables;
  // One workgroup of 1024 threads per CU at a time (16 of the 24 wave slots its registers
  // allow): all tables' workgroups in ONE round where that leaves each of them at most four
  // passes over its positions -- a workgroup that waits for a CU costs more than more passes
  // (tools/archive/r03_interp_one.py, un-batched predict(model), us per call, one pass per workgroup /
  // one round: 5 x 5 tables of 100 bins 35.0 / 31.3 (325 / 250 workgroups), 6 x 6 37.5 / 31.9,
  // 4 x 4 x 4 58.8 / 41.0 (832 / 256 workgroups); 4 x 4 fits anyway: 28.8)
  int blocks = single_draw_blocks(t0);
  const int one_round = t0->n_cus / std::max(1, n_tables);
  if (t0->tuning.single_round && one_round >= 1 && one_round < blocks && 4 * one_round >= blocks)
    blocks = one_round;
  SingleWorkspace& workspace = it->single_ws;
  status = workspace.prepare(n_tables, blocks, rt, 0);
  if (status != TC_OK) return status;
  double* ws = workspace.ngal();
  tc::SingleArgs sa{};
  for (int i = 0; i < 7; ++i) sa.theta_value[i] = i < n_theta ? theta[i] : 0.0;
  sa.n_theta = n_theta;
  sa.n_bins = t0->n_bins;
  sa.n_central = t0->plan.n_central;
  sa.n_gauss = n_gauss;
  sa.flags = flags;
  sa.split = 0.5;
  sa.log_m = sa.m = sa.weight = sa.n_h = sa.percentile = nullptr;
  sa.math_table = (const double*)t0->d_math_table;
  sa.table = nullptr;
  sa.pos_off = (const int32_t*)t0->d_pos_off;
  sa.n_positions = t0->plan.n_positions;
  sa.rt = rt;
  sa.n_r = t0->n_r;
  sa.mode = t0->mode;
  sa.ngal = ws;
  sa.partial = workspace.partial();
  sa.done = workspace.done();
  sa.epoch = workspace.epoch;
  sa.tables = (const double* const*)it->d_tables;
  sa.table_class = (const int32_t*)it->d_table_class;
  sa.class_log_m = (const double* const*)p.log_m;
  sa.class_m = (const double* const*)p.m;
  sa.class_weight = (const double* const*)p.weight;
  sa.class_n_h = (const double* const*)p.n_h;
  sa.class_percentile = (const double* const*)p.percentile;
  status = launch_single_draw_tables(t0, sa, n_tables, blocks, it->stream);
  if (status != TC_OK) return status;

  // spline weights while the kernel runs
  double weight[tc::kMaxInterpDim][tc::kMaxInterpAxis];
  for (int d = 0; d < it->n_dim; ++d) {
    const std::vector<double>& xp = it->xp[d];
    const int n = (int)xp.size();
    const double xv = x[d];
    const double* m = it->a_host.data() + it->a_offset[d] +
                      (size_t)tc::spline_segment(n, xp.data(), xv) * 4 * n;
    const double x2 = xv * xv, x3 = x2 * xv;
    for (int j = 0; j < n; ++j) weight[d][j] = tc::spline_node_weight(n, m, j, xv, x2, x3);
  }
  status = wait_single_done(&workspace, it->stream, t0->tuning.poll_done != 0);
  if (status != TC_OK) return status;
  const double* partial = workspace.partial();
  double n_cen = 0.0, n_sat = 0.0;
  for (int r = 0; r < t0->n_r; ++r) xi[r] = 0.0;
  for (int k = 0; k < n_tables; ++k) {
    double c = 1.0;
    for (int d = 0; d < it->n_dim; ++d) c *= weight[d][it->table_node[(size_t)k * it->n_dim + d]];
    const double cen = ws[2 * k], sat = ws[2 * k + 1];
    const double total = cen + sat;
    const double coef = c / (t0->mode == TC_MODE_AUTO ? total * total : total);
    n_cen += c * cen;
    n_sat += c * sat;
    const double* rows = partial + (size_t)k * blocks * rt;
    for (int r = 0; r < t0->n_r; ++r) {
      double sum = 0.0;
      for (int b = 0; b < blocks; ++b) sum += rows[(size_t)b * rt + r];
      xi[r] += coef * sum;
    }
  }
  ngal[0] = n_cen + n_sat;
  return TC_OK;
}

}  // namespace

// ---- forward calls (predict_call.h: PredictRequest, forward_chunked, forward_zero_copy) -------

namespace {
int interp_async(tc_interp* it, const PredictRequest& request, const double* data,
                 const double* precision, int64_t* ticket_out, const Call* chunk);

// An interpolator as forward_chunked and forward_zero_copy see it.  Its kernels cut a draw's
// sums where the batch size puts them: chunks agree with one piece to rounding.
struct InterpForward {
  static constexpr bool kThreadedCopyOut = false;
  tc_interp* it;
  tc_interp* handle() const { return it; }
  Call hints(const PredictRequest&, const tc::SyncChunkPlan&) const { return Call(); }
  std::vector<hipEvent_t>* chunk_events() const { return nullptr; }   // (never staggered)
  int enqueue(const PredictRequest& part, const Call& hints, hipEvent_t, hipEvent_t,
              int64_t* ticket) const {
    return interp_async(it, part, nullptr, nullptr, ticket, &hints);
  }
  int synchronize() const { return tc_interp_synchronize(it); }
  int run(const PredictRequest& staged) const {
    return interp_predict_device(it, interp_call(it, /*pinned=*/true), staged.theta, staged.n_theta,
                                 staged.x, staged.n_draws, staged.n_gauss, staged.flags,
                                 staged.ngal, staged.second);
  }
};
}  // namespace

int tc_interp_predict_zheng07_batch(tc_interp* it, const double* theta, int n_theta,
                                    const double* x, int64_t n_draws, int n_gauss,
                                    unsigned flags, double* ngal, double* xi) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  int status = check_predict_args(it->tables[0], theta, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(x && ngal && xi, "NULL pointer");
  TC_HIP(hipSetDevice(it->device));
  // (option "deterministic" = 2 of the first table, mode cross: the one-launch form for every
  // batch size, one draw included)
  bool invariant = false;
  if (it->tables[0]->tuning.deterministic >= 2 && it->tables[0]->mode == TC_MODE_CROSS &&
      !it->tables[0]->cross_host.empty() && it->tables[0]->tuning.fused != 0) {
    const CrossFused& cf = *choose_cross_fused(it->tables.data(), it->n_tables, &it->cross_fused,
                                               &it->cross_fused_wide, n_draws, flags, &status);
    if (status != TC_OK) return status;
    invariant = cross_fused_eligible(it->tables[0], probe_call(it->tables[0], /*pinned=*/true), cf,
                                     n_draws, n_gauss, flags);
  }
  if (!invariant && single_draw_eligible(it->tables[0], n_draws, n_gauss, flags) &&
      (int64_t)it->n_tables * single_draw_blocks(it->tables[0]) <= 8192)
    return interp_predict_one(it, theta, n_theta, x, n_gauss, flags, ngal, xi);
  const PredictRequest request = forward_request(it->tables[0], theta, n_theta, it->n_dim, x,
                                                 n_draws, n_gauss, flags, ngal, xi, false);
  // small and medium calls: the kernels address page-locked host buffers directly
  const InterpForward forward{it};
  if (zero_copy_serves(forward, request)) return forward_zero_copy(forward, request);
  // (option "sync_chunks" of the first table; -1: the serial path below)
  const tc::SyncChunkPlan plan =
      plan_forward_chunks(it->tables[0], it->n_lanes, false, true, request);
  if (plan.n_chunks > 0) return forward_chunked(forward, request, plan);
  status = it->theta.reserve(request.theta_bytes(), it->stream);
  if (status == TC_OK) status = it->x.reserve(request.x_bytes(), it->stream);
  if (status == TC_OK) status = it->out_ngal.reserve(request.ngal_count() * 8, it->stream);
  if (status == TC_OK) status = it->out_xi.reserve(request.second_count() * 8, it->stream);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(it->theta.ptr, theta, request.theta_bytes(), hipMemcpyHostToDevice,
                        it->stream));
  TC_HIP(hipMemcpyAsync(it->x.ptr, x, request.x_bytes(), hipMemcpyHostToDevice, it->stream));
  status = forward.run(request.on((const double*)it->theta.ptr, (const double*)it->x.ptr,
                                  (double*)it->out_ngal.ptr, (double*)it->out_xi.ptr));
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(ngal, it->out_ngal.ptr, request.ngal_count() * 8, hipMemcpyDeviceToHost,
                        it->stream));
  TC_HIP(hipMemcpyAsync(xi, it->out_xi.ptr, request.second_count() * 8, hipMemcpyDeviceToHost,
                        it->stream));
  TC_HIP(hipStreamSynchronize(it->stream));
  return TC_OK;
}

int tc_interp_chi2_zheng07_batch_device(tc_interp* it, const double* theta_device,
                                        int n_theta, const double* x_device, int64_t n_draws,
                                        int n_gauss, unsigned flags, const double* data,
                                        const double* precision, double* ngal_device,
                                        double* chi2_device) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  TC_CHECK(!(flags & TC_FLAG_SEPARATE_GAL_TYPE),
           "chi2 is defined for the total correlation function only");
  if (n_draws == 0) return TC_OK;
  TC_CHECK(data && precision && ngal_device && chi2_device, "NULL pointer");
  int status = check_predict_args(it->tables[0], theta_device, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  TC_CHECK(x_device != nullptr, "NULL pointer");
  return interp_chi2_device(it, interp_call(it, /*pinned=*/false), theta_device, n_theta, x_device,
                            n_draws, n_gauss, flags, data, precision, ngal_device, chi2_device);
}

int tc_interp_chi2_zheng07_batch(tc_interp* it, const double* theta, int n_theta,
                                 const double* x, int64_t n_draws, int n_gauss,
                                 unsigned flags, const double* data, const double* precision,
                                 double* ngal, double* chi2) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  int status = check_predict_args(it->tables[0], theta, n_theta, n_draws, n_gauss, flags);
  if (status != TC_OK) return status;
  if (n_draws == 0) return TC_OK;
  TC_CHECK(x && data && precision && ngal && chi2, "NULL pointer");
  TC_HIP(hipSetDevice(it->device));
  const PredictRequest request = forward_request(it->tables[0], theta, n_theta, it->n_dim, x,
                                                 n_draws, n_gauss, flags, ngal, chi2, true);
  status = it->theta.reserve(request.theta_bytes(), it->stream);
  if (status == TC_OK) status = it->x.reserve(request.x_bytes(), it->stream);
  if (status == TC_OK) status = it->out_ngal.reserve(request.out_bytes(), it->stream);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(it->theta.ptr, theta, request.theta_bytes(), hipMemcpyHostToDevice,
                        it->stream));
  TC_HIP(hipMemcpyAsync(it->x.ptr, x, request.x_bytes(), hipMemcpyHostToDevice, it->stream));
  double* d_ngal = (double*)it->out_ngal.ptr;
  double* d_chi2 = d_ngal + request.ngal_count();
  TC_CHECK(!(flags & TC_FLAG_SEPARATE_GAL_TYPE),
           "chi2 is defined for the total correlation function only");
  status = interp_chi2_device(it, interp_call(it, /*pinned=*/true), (const double*)it->theta.ptr,
                              n_theta, (const double*)it->x.ptr, n_draws, n_gauss, flags, data,
                              precision, d_ngal, d_chi2);
  if (status != TC_OK) return status;
  TC_HIP(hipMemcpyAsync(ngal, d_ngal, request.ngal_count() * 8, hipMemcpyDeviceToHost,
                        it->stream));
  TC_HIP(hipMemcpyAsync(chi2, d_chi2, request.second_count() * 8, hipMemcpyDeviceToHost,
                        it->stream));
  TC_HIP(hipStreamSynchronize(it->stream));
  return TC_OK;
}

namespace {

int interp_async(tc_interp* it, const PredictRequest& r, const double* data,
                 const double* precision, int64_t* ticket_out, const Call* chunk) {
  int status = check_predict_args(it->tables[0], r.theta, r.n_theta, r.n_draws, r.n_gauss, r.flags);
  if (status != TC_OK) return status;
  const int64_t n_draws = r.n_draws;
  const bool chi2 = r.likelihood;
  TC_CHECK(ticket_out != nullptr, "ticket is NULL");
  TC_CHECK(n_draws == 0 || (r.x && r.ngal && r.second), "NULL pointer");
  TC_CHECK(!(chi2 && r.separate()), "chi2 is defined for the total correlation function only");
  TC_CHECK(!chi2 || (data && precision), "NULL pointer");
  const size_t ngal_count = r.ngal_count(), second_count = r.second_count();
  // (chunk: a chunk of a synchronous call -- what it carries of a Call is its cross_target -- in
  // the library's own page-locked staging areas)
  TC_CHECK(n_draws == 0 || chunk != nullptr ||
               (is_pinned(r.theta, r.theta_bytes()) && is_pinned(r.x, r.x_bytes()) &&
                is_pinned(r.ngal, ngal_count * 8) && is_pinned(r.second, second_count * 8)),
           "asynchronous calls need page-locked buffers (tc_host_alloc / tc_host_register)");
  TC_HIP(hipSetDevice(it->device));
  // everything of a call -- upload, kernels, download, the ticket's event -- on the next lane's
  // stream: the lanes overlap each other's transfers and kernels
  Call call = interp_call(it, /*pinned=*/false);
  call.cross_target = chunk != nullptr ? chunk->cross_target : 0;
  tc_interp::Lane& L = it->lanes[call.lane];
  hipStream_t last = L.stream;
  if (n_draws > 0) {
    status = L.stage_out.reserve(r.out_bytes(), L.stream);
    if (status == TC_OK) status = L.stage_in.reserve(r.in_bytes(), L.stream);
    if (status != TC_OK) return status;
    double* d_theta = (double*)L.stage_in.ptr;
    double* d_x = d_theta + n_draws * r.n_theta;
    double* d_ngal = (double*)L.stage_out.ptr;
    double* d_second = d_ngal + ngal_count;
    {
      Range range("upload");
      TC_HIP(hipMemcpyAsync(d_theta, r.theta, r.theta_bytes(), hipMemcpyHostToDevice, L.stream));
      TC_HIP(hipMemcpyAsync(d_x, r.x, r.x_bytes(), hipMemcpyHostToDevice, L.stream));
    }
    status = chi2 ? interp_chi2_device(it, call, d_theta, r.n_theta, d_x, n_draws, r.n_gauss,
                                       r.flags, data, precision, d_ngal, d_second)
                  : interp_predict_device(it, call, d_theta, r.n_theta, d_x, n_draws, r.n_gauss,
                                          r.flags, d_ngal, d_second);
    if (status != TC_OK) return status;
    Range range("download");
    TC_HIP(hipMemcpyAsync(r.ngal, d_ngal, ngal_count * 8, hipMemcpyDeviceToHost, L.stream));
    TC_HIP(hipMemcpyAsync(r.second, d_second, second_count * 8, hipMemcpyDeviceToHost, L.stream));
  }
  return it->tickets.issue(last, ticket_out);
}

}  // namespace

int tc_interp_predict_zheng07_batch_async(tc_interp* it, const double* theta, int n_theta,
                                          const double* x, int64_t n_draws, int n_gauss,
                                          unsigned flags, double* ngal, double* xi,
                                          int64_t* ticket) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  return interp_async(it, forward_request(it->tables[0], theta, n_theta, it->n_dim, x, n_draws,
                                          n_gauss, flags, ngal, xi, false),
                      nullptr, nullptr, ticket, nullptr);
}

int tc_interp_chi2_zheng07_batch_async(tc_interp* it, const double* theta, int n_theta,
                                       const double* x, int64_t n_draws, int n_gauss,
                                       unsigned flags, const double* data,
                                       const double* precision, double* ngal, double* chi2,
                                       int64_t* ticket) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  return interp_async(it, forward_request(it->tables[0], theta, n_theta, it->n_dim, x, n_draws,
                                          n_gauss, flags, ngal, chi2, true),
                      data, precision, ticket, nullptr);
}

// ---- gradients (grad_interp_kernels.hip.h) ------------------------------------------------

namespace {

size_t interp_grad_lds(const tc_interp* it, bool chi2, int n_params) {
  const tc_table* t0 = it->tables[0];
  return t0->mode == TC_MODE_AUTO
             ? tc::grad_interp_auto_lds_bytes(t0->n_bins, t0->plan.n_central, t0->n_r, it->n_dim,
                                              chi2, n_params)
             : tc::grad_interp_cross_lds_bytes(t0->n_r, it->n_dim, chi2, n_params);
}

// The walk (class_begin, node) and, with_matrices, the tables' gradient matrices in its order: a
// joint's forward calls take the walk alone and build no gradient matrix (grad_call.h).
int build_grad_walk(tc_interp* it, bool with_matrices) {
  if (it->grad_walk.built && (!with_matrices || it->grad_walk.matrices != nullptr)) return TC_OK;
  const int n_classes = (int)it->class_table.size();
  std::vector<int32_t> class_begin(1, 0), node;
  std::vector<void*> matrices, class_n_h;
  for (int v = 0; v < n_classes; ++v) {
    class_n_h.push_back(it->tables[it->class_table[v]]->d_n_h);
    for (int k = 0; k < it->n_tables; ++k) {
      if (it->table_class[k] != v) continue;
      if (with_matrices) {
        const int status = build_grad_table(it->tables[k]);
        if (status != TC_OK) return status;
        matrices.push_back(it->tables[k]->grad.d_matrix);
      }
      node.insert(node.end(), it->table_node.begin() + (size_t)k * it->n_dim,
                  it->table_node.begin() + (size_t)(k + 1) * it->n_dim);
    }
    class_begin.push_back((int32_t)(node.size() / it->n_dim));
  }
  // (into locals: a failure half-way leaves nothing behind)
  void* uploaded[4] = {nullptr, nullptr, nullptr, nullptr};
  int status = TC_OK;
  if (!it->grad_walk.built) {
    status = upload(class_begin, &uploaded[0]);
    if (status == TC_OK) status = upload(node, &uploaded[1]);
    if (status == TC_OK) status = upload(class_n_h, &uploaded[3]);
  }
  if (status == TC_OK && with_matrices) status = upload(matrices, &uploaded[2]);
  if (status != TC_OK) {
    for (void* p : uploaded)
      if (p) (void)hipFree(p);
    return status;
  }
  if (!it->grad_walk.built) {
    it->grad_walk.class_begin = uploaded[0];
    it->grad_walk.node = uploaded[1];
    it->grad_walk.class_n_h = uploaded[3];
    it->grad_walk.built = true;
  }
  if (with_matrices) it->grad_walk.matrices = uploaded[2];
  return TC_OK;
}

// The grid and the walk of the argument block (build_grad_walk has run).
void fill_interp_grid(const tc_interp* it, tc::GradInterpArgs* ga) {
  ga->n_dim = it->n_dim;
  ga->n_classes = (int)it->class_table.size();
  for (int d = 0; d < it->n_dim; ++d) {
    ga->n_axis[d] = (int)it->xp[d].size();
    ga->axis_offset[d] = it->axis_offset[d];
    ga->a_offset[d] = it->a_offset[d];
  }
  ga->xp = (const double*)it->d_xp;
  ga->a = (const double*)it->d_a;
  ga->class_begin = (const int32_t*)it->grad_walk.class_begin;
  ga->walk_node = (const int32_t*)it->grad_walk.node;
  ga->matrices = (const double* const*)it->grad_walk.matrices;
}

// What the derivative entries of an interpolator share (grad_call.h: grad_entry, vjp_entry).
struct InterpHandle {
  tc_interp* it;
  int device_id() const { return it->device; }
  Chi2Operands& operands() const { return it->chi2; }
  int upload_chi2(const Chi2Host& host) const {
    return upload_operands(it, host.data, host.precision);
  }
};

// An interpolator as grad_entry sees it.
struct InterpGrad : InterpHandle {
  // What the table entry points refuse (check_grad_args on the first table: flags, float32, the
  // shape of theta) and a grid that does not fit the LDS of a workgroup.
  int check(const GradRequest& request, int n_theta, bool likelihood) const {
    TC_CHECK(it != nullptr, "interp handle is NULL");
    const tc_table* t0 = it->tables[0];
    const int status = check_grad_args(t0, request, n_theta, likelihood, /*fit=*/true);
    if (status != TC_OK) return status;
    if (it->n_dim > tc::grad_interp_max_dim(request.n_params))
      return fail(TC_ERR_UNSUPPORTED,
                  "gradients of %d parameters: a grid of %d dimensions, beyond the %d that the "
                  "kernels' %d quantities per draw leave room for",
                  request.n_params, it->n_dim, tc::grad_interp_max_dim(request.n_params),
                  tc::kGradThreads / tc::kGradDraws);
    const size_t lds = interp_grad_lds(it, likelihood, request.n_params);
    if (lds > (size_t)kMaxLdsBytes)
      return fail(TC_ERR_UNSUPPORTED,
                  "gradients: a grid of %d dimensions over tables of %d bins and %d correlation "
                  "function bins needs %zu bytes of LDS per workgroup, beyond the %d there are",
                  it->n_dim, t0->n_bins, t0->n_r, lds, kMaxLdsBytes);
    return TC_OK;
  }
  const char* null_message(bool) const { return "NULL pointer"; }
  GradStaging staging() const { return interp_grad_staging(it); }
  // One launch per slab of draws on a lane of the interpolator's own (it->cur; no table's `prev`
  // is written: nothing chains to these launches); the resident kernels of all its tables stop.
  int device(GradLane lane, const GradRequest& request) const {
    TC_HIP(hipSetDevice(it->device));
    tc_table* t0 = it->tables[0];
    tc::GradInterpArgs ga{};
    const int status = interp_grad_args(it, request, &ga);
    if (status != TC_OK) return status;
    hipStream_t stream = interp_grad_stream(it, lane);
    const int n_params = request.n_params;
    const int lds = (int)interp_grad_lds(it, request.likelihood(), n_params);
    return for_each_slab(request.n_draws, max_slab(t0), [&](int64_t begin, int64_t n) {
      Range range("interpolator gradients (one launch)");
      const GradRequest slab = request.slab(begin, n);
      ga.table.theta = slab.theta;
      ga.x = slab.x;
      ga.table.n_draws = n;
      slab.outputs(&ga.table);
      // (timed through the first table's timer)
      return launch_grad_batch(t0, n, lds, [&](dim3 grid, hipEvent_t k0, hipEvent_t k1) {
        return launch_grad_instance(n_params, t0->mode, it->device, grid, lds, stream, k0, k1, ga);
      });
    });
  }
};

// The request of an interpolator entry point of the family `n_params`, in the order of the C
// arguments: the n_dim extra parameters are columns behind the family's.
GradRequest interp_request(const tc_interp* it, int n_params, const double* theta, const double* x,
                           int64_t n_draws, int n_gauss, unsigned flags, double* ngal,
                           double* value, double* dngal, double* dvalue, double* fisher) {
  GradRequest request{};
  request.n_params = n_params;
  request.n_extra = it ? it->n_dim : 0;
  request.n_gauss = n_gauss;
  request.flags = flags;
  request.n_draws = n_draws;
  request.n_r = it ? it->tables[0]->n_r : 0;
  request.theta = theta;
  request.x = x;
  request.ngal = ngal;
  request.dngal = dngal;
  request.value = value;
  request.dvalue = dvalue;
  request.fisher = fisher;
  return request;
}

}  // namespace

}  // extern "C"

// ---- what a joint of interpolators takes from its members (grad_call.h) ---------------------
namespace tc {
namespace host {

InterpParts interp_parts(const tc_interp* it) {
  InterpParts parts{it->device, it->n_dim, &it->tables, &it->xp, &it->table_node, {}};
  // (the order of build_grad_walk)
  for (size_t v = 0; v < it->class_table.size(); ++v)
    for (int k = 0; k < it->n_tables; ++k)
      if (it->table_class[k] == (int32_t)v) parts.walk.push_back(k);
  return parts;
}

int interp_grad_args(tc_interp* it, const GradRequest& request, tc::GradInterpArgs* out,
                     bool with_matrices) {
  tc_table* t0 = it->tables[0];
  int status = TC_OK;
  for (tc_table* t : it->tables)
    if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
  const tc_interp::SinglePointers* pointers = nullptr;
  status = class_pointers(it, request.n_gauss, &pointers);
  if (status == TC_OK) status = build_grad_walk(it, with_matrices);
  if (status != TC_OK) return status;
  tc::GradInterpArgs& ga = *out;
  fill_grad_shape(t0, request.n_gauss, request.flags, &ga.table);
  fill_interp_grid(it, &ga);
  ga.class_log_m = (const double* const*)pointers->log_m;
  ga.class_m = (const double* const*)pointers->m;
  ga.class_weight = (const double* const*)pointers->weight;
  ga.class_n_h = (const double* const*)pointers->n_h;
  ga.class_percentile = request.n_params == tc::kGradParamsAssembias
                            ? (const double* const*)pointers->percentile
                            : nullptr;
  return TC_OK;
}

GradStaging interp_grad_staging(tc_interp* it) {
  return {&it->theta, &it->x, &it->out_ngal, &it->out_xi, it->stream};
}

hipStream_t interp_grad_stream(tc_interp* it, GradLane lane) {
  it->cur = next_lane(lane == GradLane::kPinned, it->tables[0]->tuning.pipeline != 0, it->n_lanes,
                      &it->device_calls);
  return it->lanes[it->cur].stream;
}

InterpForwardParts interp_forward_parts(tc_interp* it) {
  return {&it->h_in, &it->h_out, &it->tickets, &it->theta, &it->x, &it->out_ngal, it->stream,
          it->n_lanes};
}

InterpForwardLane interp_forward_lane(tc_interp* it) {
  (void)interp_grad_stream(it, GradLane::kNext);
  tc_interp::Lane& lane = it->lanes[it->cur];
  return {lane.stream, &lane.stage_in, &lane.stage_out};
}

}  // namespace host
}  // namespace tc

extern "C" {

// ---- the plain model (`fisher` among the outputs of the tc_interp_chi2_fisher_* entries only,
// where it must not be NULL) and the model decorated with assembly bias (seven columns of theta,
// the strengths last, then the n_dim extra parameters; `fisher` may be NULL) ----

int tc_interp_predict_grad_zheng07_batch_device(tc_interp* it, const double* theta_device,
                                                int n_theta, const double* x_device,
                                                int64_t n_draws, int n_gauss, unsigned flags,
                                                double* ngal_device, double* xi_device,
                                                double* dngal_device, double* dxi_device) {
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParams, theta_device, x_device, n_draws, n_gauss,
                                   flags, ngal_device, xi_device, dngal_device, dxi_device,
                                   nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_predict_grad_zheng07_batch(tc_interp* it, const double* theta, int n_theta,
                                         const double* x, int64_t n_draws, int n_gauss,
                                         unsigned flags, double* ngal, double* xi, double* dngal,
                                         double* dxi) {
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParams, theta, x, n_draws, n_gauss, flags, ngal,
                                   xi, dngal, dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_chi2_grad_zheng07_batch_device(tc_interp* it, const double* theta_device,
                                             int n_theta, const double* x_device,
                                             int64_t n_draws, int n_gauss, unsigned flags,
                                             const double* data, const double* precision,
                                             double* ngal_device, double* chi2_device,
                                             double* dngal_device, double* dchi2_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParams, theta_device, x_device, n_draws, n_gauss,
                                   flags, ngal_device, chi2_device, dngal_device, dchi2_device,
                                   nullptr),
                    n_theta, &operands, false);
}

int tc_interp_chi2_grad_zheng07_batch(tc_interp* it, const double* theta, int n_theta,
                                      const double* x, int64_t n_draws, int n_gauss,
                                      unsigned flags, const double* data,
                                      const double* precision, double* ngal, double* chi2,
                                      double* dngal, double* dchi2) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParams, theta, x, n_draws, n_gauss, flags, ngal,
                                   chi2, dngal, dchi2, nullptr),
                    n_theta, &operands, false);
}

int tc_interp_chi2_fisher_zheng07_batch_device(tc_interp* it, const double* theta_device,
                                               int n_theta, const double* x_device,
                                               int64_t n_draws, int n_gauss, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dngal_device, double* dchi2_device,
                                               double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParams, theta_device, x_device, n_draws, n_gauss,
                                   flags, ngal_device, chi2_device, dngal_device, dchi2_device,
                                   fisher_device),
                    n_theta, &operands, true);
}

int tc_interp_chi2_fisher_zheng07_batch(tc_interp* it, const double* theta, int n_theta,
                                        const double* x, int64_t n_draws, int n_gauss,
                                        unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dngal, double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParams, theta, x, n_draws, n_gauss, flags, ngal,
                                   chi2, dngal, dchi2, fisher),
                    n_theta, &operands, true);
}

int tc_interp_predict_grad_assembias_batch_device(tc_interp* it, const double* theta_device,
                                                  int n_theta, const double* x_device,
                                                  int64_t n_draws, int n_gauss, unsigned flags,
                                                  double* ngal_device, double* xi_device,
                                                  double* dngal_device, double* dxi_device) {
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParamsAssembias, theta_device, x_device, n_draws,
                                   n_gauss, flags, ngal_device, xi_device, dngal_device,
                                   dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_predict_grad_assembias_batch(tc_interp* it, const double* theta, int n_theta,
                                           const double* x, int64_t n_draws, int n_gauss,
                                           unsigned flags, double* ngal, double* xi,
                                           double* dngal, double* dxi) {
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParamsAssembias, theta, x, n_draws, n_gauss, flags,
                                   ngal, xi, dngal, dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_chi2_grad_assembias_batch_device(tc_interp* it, const double* theta_device,
                                               int n_theta, const double* x_device,
                                               int64_t n_draws, int n_gauss, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dngal_device, double* dchi2_device,
                                               double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParamsAssembias, theta_device, x_device, n_draws,
                                   n_gauss, flags, ngal_device, chi2_device, dngal_device,
                                   dchi2_device, fisher_device),
                    n_theta, &operands, false);
}

int tc_interp_chi2_grad_assembias_batch(tc_interp* it, const double* theta, int n_theta,
                                        const double* x, int64_t n_draws, int n_gauss,
                                        unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dngal, double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParamsAssembias, theta, x, n_draws, n_gauss, flags,
                                   ngal, chi2, dngal, dchi2, fisher),
                    n_theta, &operands, false);
}

// ---- the Leauthaud11 family (fourteen columns of theta, eleven differentiated, then the n_dim
// extra parameters; `fisher` may be NULL) ----

int tc_interp_predict_grad_leauthaud11_batch_device(tc_interp* it, const double* theta_device,
                                                    int n_theta, const double* x_device,
                                                    int64_t n_draws, int n_gauss, unsigned flags,
                                                    double* ngal_device, double* xi_device,
                                                    double* dngal_device, double* dxi_device) {
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParamsLeauthaud11, theta_device, x_device, n_draws,
                                   n_gauss, flags, ngal_device, xi_device, dngal_device,
                                   dxi_device, nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_predict_grad_leauthaud11_batch(tc_interp* it, const double* theta, int n_theta,
                                             const double* x, int64_t n_draws, int n_gauss,
                                             unsigned flags, double* ngal, double* xi,
                                             double* dngal, double* dxi) {
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParamsLeauthaud11, theta, x, n_draws, n_gauss,
                                   flags, ngal, xi, dngal, dxi, nullptr),
                    n_theta, nullptr, false);
}

int tc_interp_chi2_grad_leauthaud11_batch_device(tc_interp* it, const double* theta_device,
                                                 int n_theta, const double* x_device,
                                                 int64_t n_draws, int n_gauss, unsigned flags,
                                                 const double* data, const double* precision,
                                                 double* ngal_device, double* chi2_device,
                                                 double* dngal_device, double* dchi2_device,
                                                 double* fisher_device) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kDevice,
                    interp_request(it, tc::kGradParamsLeauthaud11, theta_device, x_device, n_draws,
                                   n_gauss, flags, ngal_device, chi2_device, dngal_device,
                                   dchi2_device, fisher_device),
                    n_theta, &operands, false);
}

int tc_interp_chi2_grad_leauthaud11_batch(tc_interp* it, const double* theta, int n_theta,
                                          const double* x, int64_t n_draws, int n_gauss,
                                          unsigned flags, const double* data,
                                          const double* precision, double* ngal, double* chi2,
                                          double* dngal, double* dchi2, double* fisher) {
  const Chi2Host operands{data, precision};
  return grad_entry(InterpGrad{it}, GradRoute::kHost,
                    interp_request(it, tc::kGradParamsLeauthaud11, theta, x, n_draws, n_gauss,
                                   flags, ngal, chi2, dngal, dchi2, fisher),
                    n_theta, &operands, false);
}

// ---- the occupation seam (interp_vjp_kernels.hip.h) ---------------------------------------------

namespace {

size_t interp_vjp_lds(const tc_interp* it) {
  const tc_table* t0 = it->tables[0];
  return t0->mode == TC_MODE_AUTO
             ? tc::interp_vjp_auto_lds_bytes(t0->n_bins, t0->n_r, it->n_dim)
             : tc::interp_vjp_cross_lds_bytes(t0->n_r, it->n_dim);
}

// What the entries at the occupation seam refuse, the NULL handle first: flags, float32, a negative
// number of draws, a workgroup beyond the LDS of a CU.
int check_interp_vjp(const tc_interp* it, int64_t n_draws, unsigned flags) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  const tc_table* t0 = it->tables[0];
  if (flags & TC_FLAG_SEPARATE_GAL_TYPE)
    return fail(TC_ERR_UNSUPPORTED, "the interpolator occupation VJP is implemented for the total "
                                    "prediction only (not separate_gal_type)");
  if (flags != 0)
    return fail(TC_ERR_UNSUPPORTED, "interpolator occupation VJP: flags must be 0, got 0x%x",
                flags);
  if (t0->compute_dtype != TC_DTYPE_F64)
    return fail(TC_ERR_UNSUPPORTED,
                "the interpolator occupation VJP needs a float64 compute dtype");
  TC_CHECK(n_draws >= 0, "n_draws must be non-negative");
  const size_t lds = interp_vjp_lds(it);
  if (lds > (size_t)kMaxLdsBytes)
    return fail(TC_ERR_UNSUPPORTED,
                "interpolator occupation VJP: a grid of %d dimensions over tables of %d bins and "
                "%d correlation function bins needs %zu bytes of LDS per workgroup, beyond the %d "
                "there are",
                it->n_dim, t0->n_bins, t0->n_r, lds, kMaxLdsBytes);
  return check_grad_fit(t0, "interpolator occupation VJP", lds);
}

// An interpolator as vjp_entry sees it: x is required, and the adjoint arrays go together.
struct InterpVjp : InterpHandle {
  int check(int64_t n_draws, unsigned flags) const { return check_interp_vjp(it, n_draws, flags); }
  VjpRule rule() const {
    return {true, true,
            {"g_xi, g_occupation and g_x go together: all NULL is the forward-only form",
             "dchi2_docc, dchi2_dx and dngal_dx go together: all NULL is the forward-only form"}};
  }
  VjpStaging staging() const {
    return {&it->theta, &it->out_ngal, &it->out_xi, it->stream, max_slab(it->tables[0])};
  }
  // One launch per slab of draws on a lane of the interpolator's own (as InterpGrad), timed
  // through the first table's timer; the resident kernels of all its tables stop, the walk is built.
  int device(GradLane lane, const VjpRequest& request) const {
    tc_table* t0 = it->tables[0];
    int status = TC_OK;
    for (tc_table* t : it->tables)
      if (t->resident.running && (status = resident_stop(t)) != TC_OK) return status;
    status = build_grad_walk(it, /*with_matrices=*/true);
    if (status != TC_OK) return status;
    tc::InterpVjpArgs ia{};
    fill_interp_grid(it, &ia.interp);
    ia.interp.class_n_h = (const double* const*)it->grad_walk.class_n_h;
    ia.vjp.n_bins = t0->n_bins;
    ia.vjp.n_r = t0->n_r;
    ia.vjp.perm = (const int32_t*)t0->d_perm;
    ia.vjp.row_tiles = tc::grad_row_tiles(t0->n_bins);
    ia.vjp.k_steps = tc::grad_k_steps(t0->n_bins);
    const int lds = (int)interp_vjp_lds(it);
    hipStream_t stream = interp_grad_stream(it, lane);
    return vjp_slabs(request, max_slab(t0), [&](const VjpRequest& slab) {
      Range range("interpolator occupation VJP (one launch)");
      slab.arrays(&ia.vjp);
      ia.interp.table.n_draws = slab.n_draws;
      ia.interp.x = slab.x;
      ia.g_x = slab.g_x;
      ia.dngal_dx = slab.dngal_dx;
      return launch_grad_batch(t0, slab.n_draws, lds, [&](dim3 grid, hipEvent_t k0, hipEvent_t k1) {
        return launch_vjp_interp_instance(t0->mode, it->device, grid, lds, stream, k0, k1, ia);
      });
    });
  }
};

// The request of such an entry, in the order of the C arguments.
VjpRequest interp_vjp_request(const tc_interp* it, const double* occupation, const double* x,
                              int64_t n_draws, const double* g_ngal, const double* g_xi,
                              double* ngal, double* xi, double* chi2, double* g_occupation,
                              double* g_x, double* dngal_dx) {
  const tc_table* t0 = it ? it->tables[0] : nullptr;
  return VjpRequest{n_draws, t0 ? t0->n_bins : 0, t0 ? t0->n_r : 0, occupation, g_ngal, g_xi,
                    nullptr, ngal, xi, chi2, g_occupation, it ? (int)it->class_table.size() : 1,
                    it ? it->n_dim : 0, x, g_x, dngal_dx};
}

}  // namespace

int tc_interp_info(const tc_interp* it, int* n_tables, int* n_classes, int* table_class,
                   int* class_table) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  if (n_tables != nullptr) *n_tables = it->n_tables;
  if (n_classes != nullptr) *n_classes = (int)it->class_table.size();
  if (table_class != nullptr)
    for (int k = 0; k < it->n_tables; ++k) table_class[k] = it->table_class[k];
  if (class_table != nullptr)
    for (size_t v = 0; v < it->class_table.size(); ++v) class_table[v] = it->class_table[v];
  return TC_OK;
}

int tc_interp_predict_occupation_vjp_batch(tc_interp* it, const double* occupation,
                                           const double* x, int64_t n_draws, unsigned flags,
                                           const double* g_ngal, const double* g_xi, double* ngal,
                                           double* xi, double* g_occupation, double* g_x) {
  return vjp_entry(InterpVjp{it}, GradRoute::kHost, flags,
                   interp_vjp_request(it, occupation, x, n_draws, g_ngal, g_xi, ngal, xi,
                                      nullptr, g_occupation, g_x, nullptr),
                   nullptr);
}

int tc_interp_predict_occupation_vjp_batch_device(tc_interp* it, const double* occupation_device,
                                                  const double* x_device, int64_t n_draws,
                                                  unsigned flags, const double* g_ngal_device,
                                                  const double* g_xi_device, double* ngal_device,
                                                  double* xi_device, double* g_occupation_device,
                                                  double* g_x_device) {
  return vjp_entry(InterpVjp{it}, GradRoute::kDevice, flags,
                   interp_vjp_request(it, occupation_device, x_device, n_draws,
                                      g_ngal_device, g_xi_device, ngal_device, xi_device,
                                      nullptr, g_occupation_device, g_x_device, nullptr),
                   nullptr);
}

int tc_interp_chi2_occupation_grad_batch(tc_interp* it, const double* occupation, const double* x,
                                         int64_t n_draws, unsigned flags, const double* data,
                                         const double* precision, double* ngal, double* chi2,
                                         double* dchi2_docc, double* dchi2_dx, double* dngal_dx) {
  const Chi2Host operands{data, precision};
  return vjp_entry(InterpVjp{it}, GradRoute::kHost, flags,
                   interp_vjp_request(it, occupation, x, n_draws, nullptr, nullptr, ngal,
                                      nullptr, chi2, dchi2_docc, dchi2_dx, dngal_dx),
                   &operands);
}

int tc_interp_chi2_occupation_grad_batch_device(tc_interp* it, const double* occupation_device,
                                                const double* x_device, int64_t n_draws,
                                                unsigned flags, const double* data,
                                                const double* precision, double* ngal_device,
                                                double* chi2_device, double* dchi2_docc_device,
                                                double* dchi2_dx_device,
                                                double* dngal_dx_device) {
  const Chi2Host operands{data, precision};
  return vjp_entry(InterpVjp{it}, GradRoute::kDevice, flags,
                   interp_vjp_request(it, occupation_device, x_device, n_draws, nullptr,
                                      nullptr, ngal_device, nullptr, chi2_device,
                                      dchi2_docc_device, dchi2_dx_device, dngal_dx_device),
                   &operands);
}

int tc_debug_interp_vjp_lds_bytes(int mode, int n_bins, int n_r, int n_dim, int64_t* bytes) {
  TC_CHECK(bytes != nullptr, "bytes is NULL");
  TC_CHECK((mode == TC_MODE_AUTO || mode == TC_MODE_CROSS) && n_bins >= 1 && n_r >= 1 &&
               n_dim >= 1 && n_dim <= tc::kMaxInterpDim,
           "invalid shape");
  *bytes = (int64_t)(mode == TC_MODE_AUTO ? tc::interp_vjp_auto_lds_bytes(n_bins, n_r, n_dim)
                                          : tc::interp_vjp_cross_lds_bytes(n_r, n_dim));
  return TC_OK;
}

int tc_interp_wait(tc_interp* it, int64_t ticket) {
  TC_CHECK(it != nullptr, "interp handle is NULL");
  return it->tickets.wait(ticket, [it] { return tc_interp_synchronize(it); });
}

int tc_interp_query(tc_interp* it, int64_t ticket, int* done) {
  TC_CHECK(it != nullptr && done != nullptr, "NULL argument");
  static const char* const what[2] = {"query", "query"};
  return it->tickets.query(ticket, done, it->lanes, what);
}

}  // extern "C"
