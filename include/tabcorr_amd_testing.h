/*
 * tabcorr_amd_testing.h -- test-infrastructure and developer hooks of libtabcorr_hip.so.
 *
 * NOT part of the drop-in boundary (include/tabcorr_amd.h): nothing here is called by the
 * product's host classes.  The CPU tests (tests/test_host_cpu.py) use the tc_debug_* helpers
 * to check host-side planning code and the table-driven math without a GPU; the timeline
 * readers return data only from developer builds (-DTC_DEVELOPER_KNOBS, tools/build_dev.sh).
 */
#ifndef TABCORR_AMD_TESTING_H
#define TABCORR_AMD_TESTING_H

#include "tabcorr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host evaluation of the table-driven FP64 functions the occupation kernel uses in place
 * of the device libm (tabcorr_amd/csrc/fastmath.h): kind 0 erf, 1 log2 (x > 0 normal),
 * 2 exp2, 3 exp10, 4 erf and 5 its derivative 2/sqrt(pi) exp(-x^2) from erf_gauss_fast,
 * 6 the natural logarithm (x > 0 normal) of the gradient kernels, 7 erfc(|x|) / 2 for |x| >= 2.5
 * as the assembly-bias gradient kernels form it from the Gaussian of kind 5 (half_erfc_from_gauss;
 * from |x| = 6 on, where kind 5 is zero, from the libm Gaussian). */
int tc_debug_fastmath(int kind, int64_t n, const double* x, double* y);
/* The same functions as the DEVICE compiles them (needs a GPU): a small kernel stages the table
 * in LDS as the occupation kernel does and applies kinds 0 - 7 to x; kind 8 is the reciprocal of
 * the satellites' expansion (series.h: sat::reciprocal -- the hardware estimate and two Newton
 * steps on the device, 1.0 / x on the host), kind 9 exp2 with keep == false (exactly 0).  The
 * device text differs from the host's in log2 (frexp_mant / frexp_exp / ubfe against frexp and
 * shifts), ldexp and the contraction of a * b + c. */
int tc_debug_fastmath_device(int kind, int64_t n, const double* x, double* y);

/* The dense matrix-operand layout the gradient kernel of mode auto reads
 * (tabcorr_amd/csrc/grad.h), built from packed (n_r, n_bins (n_bins + 1) / 2) lower triangles
 * (p = i (i + 1) / 2 + j, j <= i) and read back lane by lane as the kernel addresses it:
 * dense (n_r, n_bins, n_bins) = the symmetric matrices.  Fails if a padding entry is not zero. */
int tc_debug_grad_operand(int n_bins, int n_r, const double* packed, double* dense);

/* The LDS bytes per workgroup that the launch layer asks for and refuses by
 * (tabcorr_amd/csrc/grad.h): kernel 0 grad_auto_kernel, 1 grad_cross_kernel, 2
 * grad_interp_auto_kernel, 3 grad_interp_cross_kernel; n_params 5 (plain Zheng07), 7 (decorated
 * with assembly bias) or 11 (Leauthaud11: kernels 0 and 1 only, the interpolator's budget of every
 * family is tc_debug_interp_grad_lds_bytes'); chi2: the likelihood is finished in the launch; n_dim: the interpolator's
 * axes (ignored by kernels 0 and 1, as n_bins and n_central are by 1 and 3). */
int tc_debug_grad_lds(int kernel, int n_params, int n_bins, int n_central, int n_r, int n_dim,
                      int chi2, int64_t* bytes);

/* The LDS bytes per workgroup of the interpolator's gradient kernels (tabcorr_amd/csrc/grad.h:
 * grad_interp_auto_lds_bytes, grad_interp_cross_lds_bytes) for every family: mode TC_MODE_AUTO or
 * TC_MODE_CROSS, n_params 5, 7 or 11; for 5 and 7 what tc_debug_grad_lds(2 | 3, ...) returns.  In
 * mode cross the slab holds 64 bins for 5 and 7 parameters and 32 for 11 (n_bins and n_central
 * are ignored there).  TC_ERR_UNSUPPORTED for more axes than the family serves: n_params + 1 +
 * n_dim quantities per draw must not exceed 16, which leaves 11 parameters four axes. */
int tc_debug_interp_grad_lds_bytes(int mode, int n_params, int n_bins, int n_central, int n_r,
                                   int n_dim, int chi2, int64_t* bytes);

/* The slab arithmetic of the derivative entry points (tabcorr_amd/csrc/grad_call.h:
 * GradRequest::slab): the element offsets that the slab beginning at draw `begin` adds to the
 * arrays of a call of the family n_params (5, 7 or 11) with n_extra interpolator axes and n_r
 * result rows per draw, in the prediction form or (likelihood != 0) the likelihood form with its
 * Fisher matrix -- offsets[7]: theta, x, ngal, dngal, xi or chi2, dxi or dchi2, fisher; -1 where
 * the call has no such array. */
int tc_debug_grad_slab(int n_params, int n_extra, int n_r, int likelihood, int64_t begin,
                       int64_t* offsets);

/* The chunks of a synchronous host-array prediction or likelihood (tabcorr_amd/csrc/hostmath.h:
 * plan_sync_chunks) -- no device needed -- of n_draws draws with out_bytes_per_draw bytes of
 * results per draw, second_cols of them doubles of the second array.  options: the values of
 * "sync_chunks", "sync_stagger", "pipeline" (three ints); n_lanes: the handle's lanes; call: bit 0
 * option "ordered", 1 a likelihood, 2 a float32 table, 3 an interpolator, 4 mode cross.
 * n_chunks = 0: the serial path; else chunk k holds the draws [begins[k], begins[k + 1]) (begins:
 * capacity 65), every chunk at least one; staggered: the chunks' kernels run one after the other. */
int tc_debug_sync_chunks(int64_t n_draws, int64_t out_bytes_per_draw, int64_t second_cols,
                         const int* options, int n_lanes, unsigned call, int* n_chunks,
                         int64_t* begins, int* staggered);

/* The node arithmetic of the Leauthaud11 gradient kernels (tabcorr_amd/csrc/grad_leauthaud11.h)
 * on the host, for one draw theta (14 columns) and n halo masses: log_mstar (n) the root of the
 * stellar-to-halo mass relation, n_cen (n) and dn_cen (n, 11) the centrals' occupation and its
 * derivatives with respect to the first eleven theta columns, n_sat (n) and dn_sat (n, 11) the
 * satellites' (modulate != 0: times <N_cen>, by the product rule). */
int tc_debug_leauthaud11_node_grad(const double* theta, int modulate, int64_t n,
                                   const double* mass, double* log_mstar, double* n_cen,
                                   double* dn_cen, double* n_sat, double* dn_sat);

/* The moment expansion of a central bin's node sum (tabcorr_amd/csrc/series.h) on the host,
 * next to the node loop it replaces: for one bin [log_min, log_max] with
 * prim_haloprop_dist_index `dist_index` and n_gauss nodes, and n draws (log_m_min, sigma):
 * series[i] = the expansion with the number of terms the kernel would take for a wave whose
 * smallest |sigma| is that draw's (terms[i]; 0: the expansion does not apply, series[i] is
 * then the node loop's value), nodes[i] = sum_k W_k erf_fast((log M_k - log_m_min) / sigma). */
int tc_debug_central_series(int n_gauss, double log_min, double log_max, double dist_index,
                            int64_t n, const double* log_m_min, const double* sigma,
                            double* series, double* nodes, int32_t* terms);

/* The same for a satellite bin (series.h, namespace sat): the binomial expansion of
 * sum_k W_k ((M_k - M0) / M1)^alpha around the bin's reference mass next to the node loop;
 * terms[i] from that draw's M0 (0: the expansion does not apply -- the bin is too close to M0 or
 * alpha outside [0, 4] --, series[i] is then the node loop's value). */
int tc_debug_satellite_series(int n_gauss, double log_min, double log_max, double dist_index,
                              int64_t n, const double* log_m0, const double* log_m1,
                              const double* alpha, double* series, double* nodes,
                              int32_t* terms);

/* Work decomposition used by the contraction kernel for a table with n_bins rows of which
 * the first n_central (after the library's stable sort by gal_type) are centrals, cut into
 * n_chunks wave-sized pieces.  Outputs one record per packed column, in processing order:
 * entry_pair[e] = packed column p (auto) or bin (cross), entry_chunk[e], entry_class[e]
 * (0 cen-cen / cen, 1 cen-sat, 2 sat-sat / sat).  Lets CPU tests check that the kernel's
 * traversal covers every column exactly once and only gathers density rows its workgroup
 * stages (padding positions included). */
int tc_plan_debug(int mode, int n_bins, const uint8_t* is_central, int n_chunks,
                  int64_t* n_entries, int32_t* entry_pair, int32_t* entry_chunk,
                  int32_t* entry_class);

/* Quadratic-form contraction kernel (mode auto, float64; tabcorr_amd/csrc/hostmath.h):
 * builds the schedule for a table of n_bins bins (the first n_central centrals) and checks
 * that it covers every (draw tile, r tile, component, table, unit) exactly once with
 * consecutive slabs per output group; returns its size and the smallest / largest number
 * of units any wave gets. */
int tc_debug_quad_schedule(int n_bins, int n_central, int by_type, int n_tiles, int n_rtiles,
                           int n_tables, int separate, int max_waves, int min_units,
                           int order /* 0 draw-tile-major, 1 table-major, 2 r-tile-major */,
                           int* n_waves, int* n_runs, int* n_slabs, int64_t* units_min,
                           int64_t* units_max);
/* The equal contiguous parts of a triangle of n_rb block rows that the waves of
 * predict_fused_kernel walk (hostmath.h: triangle_parts): first block row, block column and
 * number of units of each of the n_parts parts. */
int tc_debug_triangle_parts(int n_rb, int n_parts, int32_t* rb0, int32_t* cb0, int32_t* count);
/* The LDS bytes per workgroup of grad_joint_kernel (tabcorr_amd/csrc/joint.h: joint_lds_bytes)
 * for a joint of tables with n_bins bins, the first n_central centrals, and n_r_total result rows
 * in all -- no device needed; chi2: the likelihood is finished in the launch; n_params 5 or 7. */
int tc_debug_joint_lds_bytes(int n_bins, int n_central, int n_r_total, int chi2, int n_params,
                             int64_t* bytes);
/* The LDS bytes per workgroup of joint_forward_kernel (tabcorr_amd/csrc/joint.h:
 * joint_forward_lds_bytes) for tables of n_bins bins, n_r_total result rows in all and `waves`
 * waves per workgroup (the kernel's: 8) -- no device needed. */
int tc_debug_joint_forward_lds_bytes(int n_bins, int n_r_total, int waves, int64_t* bytes);
/* The LDS bytes per workgroup of vjp_joint_kernel (tabcorr_amd/csrc/joint.h: joint_vjp_lds_bytes)
 * for tables of n_bins bins, n_r_total result rows in all and n_r_auto of them those of mode-auto
 * tables -- no device needed. */
int tc_debug_joint_vjp_lds_bytes(int n_bins, int n_r_total, int n_r_auto, int64_t* bytes);
/* The LDS bytes per workgroup of vjp_interp_auto_kernel (mode 0) / vjp_interp_cross_kernel (mode
 * 1; n_bins is not read) (tabcorr_amd/csrc/vjp.h: interp_vjp_auto_lds_bytes,
 * interp_vjp_cross_lds_bytes) for an interpolator of n_dim dimensions over tables of n_bins bins
 * and n_r correlation function bins -- no device needed. */
int tc_debug_interp_vjp_lds_bytes(int mode, int n_bins, int n_r, int n_dim, int64_t* bytes);
/* What the forward entries of a joint refuse on the host, from plain numbers -- no device, no
 * handle: n_tables tables of n_bins bins with mode[k] (0 auto, 1 cross), n_r[k] correlation
 * function bins and compute_dtype[k] (TC_DTYPE_*).  TC_OK and the workgroup's LDS in *lds_bytes
 * (may be NULL), or TC_ERR_UNSUPPORTED with the entry's message: a member that is not float64, a
 * mode-auto member of more than 20 r bins, a workgroup beyond 160 KiB (*lds_bytes is set). */
int tc_debug_joint_forward_fit(int n_bins, int n_tables, const int* mode, const int* n_r,
                               const int* compute_dtype, int64_t* lds_bytes);
/* The LDS bytes per workgroup of grad_joint_interp_kernel (tabcorr_amd/csrc/joint_interp.h:
 * joint_interp_lds_bytes) -- no device needed.  form 1: the rows form (a member is mode auto) of a
 * joint over tables of n_bins bins, the first n_central centrals, with n_r_total result rows in
 * all, n_r_cross of them those of mode-cross members; form 0: the slab form (every member mode
 * cross; n_bins and n_central are not read, n_r_cross must be n_r_total).  n_dim: the grid's
 * dimensions; n_params 5 or 7. */
int tc_debug_joint_interp_lds_bytes(int form, int n_bins, int n_central, int n_r_total,
                                    int n_r_cross, int n_dim, int n_params, int64_t* bytes);
/* The LDS bytes per workgroup of joint_interp_forward_kernel (tabcorr_amd/csrc/joint_interp.h:
 * joint_interp_forward_lds_bytes) -- no device needed.  form 1: the rows form of a joint over
 * tables of n_bins bins; form 0: the slab form (n_bins is not read); n_r_total result rows in all,
 * n_weight_rows the sum of the grid axes' nodes, `waves` waves per workgroup (the kernel's: 8). */
int tc_debug_joint_interp_forward_lds_bytes(int form, int n_bins, int n_r_total,
                                            int n_weight_rows, int waves, int64_t* bytes);
/* What the forward entries of a joint of interpolators refuse on the host, from plain numbers --
 * no device, no handle: n_members members over tables of n_bins bins with mode[m] (0 auto, 1
 * cross) and n_r[m] correlation function bins, on a grid of n_dim axes of n_axis[d] nodes.  TC_OK,
 * the joint's form in *form and the workgroup's LDS in *lds_bytes (either may be NULL), or
 * TC_ERR_UNSUPPORTED with the entry's message: a mode-auto member of more than 20 r bins or more
 * than 248 bins, a workgroup beyond 160 KiB (*form and *lds_bytes are set). */
int tc_debug_joint_interp_forward_fit(int n_bins, int n_members, const int* mode, const int* n_r,
                                      int n_dim, const int* n_axis, int* form,
                                      int64_t* lds_bytes);
/* Groups of bins that share their Gauss-Legendre nodes (tabcorr_amd/csrc/hostmath.h:
 * find_node_groups; identical log_prim_haloprop_min / max and galaxy type), for n_bins bins in
 * library order of which the first n_central are centrals: group i = member[begin[i] ..
 * begin[i + 1]).  begin holds n_groups + 1 entries (capacity n_bins + 1), member n_bins. */
int tc_debug_node_groups(int n_bins, int n_central, const double* log_min,
                         const double* log_max, int32_t* begin, int32_t* member,
                         int* n_groups, int* n_central_groups);
/* Which form a batched call of mode auto takes (tabcorr_amd/csrc/hostmath.h: choose_fused_form)
 * on a float64 table of n_bins bins (the first n_central centrals) and n_r r values on a device
 * with n_cus compute units -- no device needed: waves x draws per workgroup of the one launch
 * (8 x 64, 16 x 64, 8 x 32, 8 x 40) and its dynamic LDS, or waves = draws = lds_bytes = 0: the
 * three kernels.  call: bit 0 the call runs alone on its lane (host-buffer API, one lane,
 * pipeline off), 1 asynchronous, 2 a chunk of a synchronous call that fits one round of 40-draw
 * workgroups, 3 chained finalisations (option "ordered"), 4 developer timeline, 5 the fused
 * likelihood is asked for.  options: the values of "fused", "fused_min_draws",
 * "fused_max_draws", "fused_waves", "fused_draws", "fused_spread", "fused_spread_min",
 * "fused_spread_rounds", "deterministic" (nine ints).  measured_forms (9) / measured_us (9 x 3):
 * a measured choice as tc_table_autotune_result returns it, or both NULL. */
int tc_debug_fused_form(int n_bins, int n_central, int n_r, int n_cus, int grouped,
                        int64_t n_draws, int n_gauss, unsigned flags, unsigned call,
                        const int* options, const int* measured_forms, const float* measured_us,
                        int* waves, int* draws, int* lds_bytes);
/* What the pair counter (tabcorr_amd/csrc/paircount.hip: pair_count) plans for a periodic box,
 * a reach in the plane (r_p,max or s_max) and along the line of sight (pi_max or s_max), the
 * larger of the two samples' point counts, n_bin = n_rp (labelled r_p counts), n_rp n_pi or
 * n_s n_mu bins and n_labels labels -- no device needed: cells and neighbour cells per side
 * (2, 1, or 0 for a single cell) along x, y, z (tabcorr_amd/csrc/hostmath.h: make_cell_grid),
 * the labels per block of sample 1 and of sample 2 and the number of blocks on either side
 * (plan_label_blocks), and the dynamic LDS bytes per workgroup the launch asks for.
 * n_labels == 0: the unlabelled count (blocks reported as 0).  Fails as the count itself
 * would where the bins exceed what a workgroup's LDS counters take. */
int tc_debug_pair_plan(const double* boxsize, double reach_xy, double reach_z,
                       int64_t n_points, int n_bin, int n_labels, int32_t* cells,
                       int32_t* neighbours, int32_t* labels_per_block, int32_t* n_blocks,
                       int64_t* lds_bytes);
/* TEST INFRASTRUCTURE, never called by the product: executes the kernel's table layout,
 * schedule and slab grouping on the host, lane by lane, for densities (n_bins, ldb) given
 * in the reference's bin order; out (n_draws, 1 | 3, n_r) = sum_p c_p T[r][p] n_i n_j
 * before the normalisation (tabcorr.py:641-655).  Lets CPU tests check the index logic of
 * contract_quad_kernel / finalize_quad_kernel without a GPU. */
int tc_debug_quad_emulate(int n_bins, int n_r, const double* tpcf_matrix,
                          const uint8_t* is_central, int by_type, int separate,
                          const double* densities, int64_t ldb, int64_t n_draws,
                          int max_waves, int min_units, int order, double* out);

/* Developer timeline (environment TC_TRACE=1): per workgroup of the last contraction
 * launch six words: 100 MHz timestamps at start / after staging / after the main loop /
 * at the end, HW_ID and XCC_ID.  Copies min(capacity, n_blocks) records. */
int tc_debug_trace(tc_table* table, uint64_t* out, int64_t capacity, int64_t* n_blocks);
/* Same run, per wavefront: timestamps at the start of the main loop, after 1/4, 1/2 and
 * 3/4 of its blocks and at the end, and HW_ID (wave slot / SIMD / CU). */
int tc_debug_wave_trace(tc_table* table, uint64_t* out, int64_t capacity,
                        int64_t* n_waves);
/* Resident un-batched path (option "resident"): per workgroup the 100 MHz ticks the last call
 * took from the sight of its parameters to the store of its completion word. */
int tc_debug_resident_ticks(tc_table* table, uint64_t* out, int64_t capacity, int64_t* n_blocks);
/* Resident ensemble kernel: eight words of workgroup 0 in the last call (developer builds;
 * 100 MHz stamps: call seen, occupation stored, the group's occupations seen, densities in LDS,
 * quarters summed, partial sums stored; [6] shader cycles of the quarter sums; [7] finished),
 * then three host times of that call in
 * ns (published, every row combined -- from its begin --, time spent on the rows): 11 words. */
int tc_debug_ensemble_stamps(tc_table* table, uint64_t* out);
#ifdef __cplusplus
}
#endif

#endif /* TABCORR_AMD_TESTING_H */
