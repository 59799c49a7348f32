/*
 * tabcorr_amd.h -- C ABI of libtabcorr_hip.so, the MI355X (gfx950) implementation
 * of TabCorr's predict() path.
 *
 * The reference (johannesulf/TabCorr v1.2.0) is pure Python and has no FFI layer;
 * the seam this library sits behind is the Python class surface.  Each entry point
 * below names the reference code it replaces (paths relative to the reference
 * repository root).  The library is loaded with ctypes by tabcorr_amd/_lib.py;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C symbols, opaque handles, int status return (0 = TC_OK), no exceptions
 *     cross the boundary; tc_last_error() returns a thread-local message.
 *   - all host arrays are caller-owned, C-contiguous, little-endian; outputs are
 *     caller-allocated.  The library never frees caller memory.
 *   - functions with the suffix _device take DEVICE pointers, enqueue work on the
 *     handle's stream and return without synchronising (tc_*_synchronize waits).
 *   - a handle is bound to the HIP device that was current when it was created and
 *     must be used by one host thread at a time.  An interpolator handle works THROUGH the
 *     table handles it was created from (their caches, lanes, timers and fused-likelihood
 *     state): a call on the interpolator must not run concurrently with a call on any of
 *     its tables either (the Python classes take the tables' locks with the
 *     interpolator's).  A joint handle (tc_joint) works through its tables in the same way --
 *     its launches run on the lanes of its FIRST table and read every table's matrix --: a call
 *     on the joint must not run concurrently with a call on any of its tables, and no call on
 *     it may follow the destruction of one of them.
 *   - there is no CPU fallback: every compute entry point fails with TC_ERR_HIP when
 *     no gfx950 device is usable.
 */
#ifndef TABCORR_AMD_H
#define TABCORR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TC_OK 0
#define TC_ERR_INVALID 1     /* bad argument (Python side raises ValueError) */
#define TC_ERR_HIP 2         /* HIP runtime / device failure (RuntimeError) */
#define TC_ERR_UNSUPPORTED 3 /* valid request this build cannot serve */
#define TC_ERR_RCCL 4        /* RCCL failure */

/* tabcorr/tabcorr.py:625,648 -- attrs['mode'] */
#define TC_MODE_AUTO 0
#define TC_MODE_CROSS 1

/* element type of a correlation matrix handed to tc_table_create */
#define TC_DTYPE_F64 0
#define TC_DTYPE_F32 1

/* flags of the predict entry points */
#define TC_FLAG_SEPARATE_GAL_TYPE 1u  /* predict(..., separate_gal_type=True), tabcorr.py:652-683 */
#define TC_FLAG_MODULATE_WITH_CENOCC 2u /* <N_sat> *= <N_cen> (halotools Zheng07Sats option) */
#define TC_FLAG_ASSEMBIAS 4u          /* theta carries 2 extra Heaviside assembly-bias strengths */
#define TC_FLAG_LEGACY_NO_DIST_INDEX 8u /* table without prim_haloprop_dist_index, tabcorr.py:571-574 */
/* Occupation family of the theta columns (default: Zheng et al. 2007).  With
 * TC_FLAG_LEAUTHAUD11 every entry point named *_zheng07_* evaluates the Leauthaud et al.
 * (2011) centrals / satellites on the Behroozi et al. (2010) stellar-to-halo mass relation
 * instead; theta then has 14 columns: logm0, logm1, beta, delta, gamma (the relation at the
 * model's redshift), scatter, alphasat, bsat, betasat, bcut, betacut, threshold (log10 of
 * the stellar mass threshold), the Hubble parameter inside the relation (halotools'
 * Behroozi10SmHm: 0.7) and that of the satellite terms (halotools' Leauthaud11Sats: 0.72).  TC_FLAG_MODULATE_WITH_CENOCC applies as for
 * Zheng07; TC_FLAG_ASSEMBIAS is not available for this family. */
#define TC_FLAG_LEAUTHAUD11 16u

typedef struct tc_table tc_table;
typedef struct tc_interp tc_interp;
typedef struct tc_comm tc_comm;
typedef struct tc_joint tc_joint;
typedef struct tc_joint_interp tc_joint_interp;

/* ---- runtime ---------------------------------------------------------------------- */

const char* tc_last_error(void);
/* The copies that end a synchronous host call (results from the page-locked staging area into
 * the caller's arrays) are shared with `helpers` threads of the library (default 3, 0 .. 7; 0:
 * the calling thread copies alone), which poll for the next job for `spin_us` microseconds
 * (default 100, 0 .. 100000) before they sleep: set both to 0 where every core runs a rank of
 * its own.  Process-wide; the threads are started by the first large copy, and a forked child
 * starts its own. */
int tc_set_copy_threads(int helpers, int spin_us);
int tc_device_count(int* count);
int tc_set_device(int device);
int tc_get_device(int* device);
/* HIP runtime version the library is bound to (guards against a second HIP runtime in
 * the process) and a short device description. */
int tc_runtime_version(int* version);
int tc_device_name(char* buffer, size_t size);
int tc_device_synchronize(void);

/* Device memory for callers that keep draws / results resident (bench.py, multi-GPU). */
int tc_device_malloc(void** ptr, size_t bytes);
int tc_device_free(void* ptr);
int tc_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
int tc_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);

/* Page-locked host memory for the asynchronous entry points (tc_*_async): caller-owned,
 * released with tc_host_free.  tc_host_register pins memory the caller already owns (e.g.
 * the coordinate array of an ensemble sampler) until tc_host_unregister.  The library keeps
 * a registry of these ranges; tc_host_is_pinned reports whether [ptr, ptr + bytes) lies
 * inside one (no HIP call, usable without a device). */
int tc_host_alloc(void** ptr, size_t bytes);
int tc_host_free(void* ptr);
int tc_host_register(void* ptr, size_t bytes);
int tc_host_unregister(void* ptr);
int tc_host_is_pinned(const void* ptr, size_t bytes, int* pinned);

/* ---- helpers exported for the host-side tests (pure host code, no GPU needed) ------- */

/* Gauss-Legendre nodes mapped to (0, 1) and weights, as tabcorr.py:543-546
 * (np.polynomial.legendre.leggauss(n); x = (x + 1) / 2). */
int tc_gauss_legendre(int n, double* x, double* w);

/* Packed-pair index map of tabcorr.py:770-806 / 626-639: for every packed column p the
 * row index i1, column index i2 (i2 <= i1) and prefactor (1 on the diagonal, else 2). */
int tc_pair_indices(int n_bins, int32_t* index_1, int32_t* index_2, int32_t* prefactor);

/* Not-a-knot cubic spline matrix a[(n-1)][4][n] of interpolator.py:219-272. */
int tc_spline_interpolation_matrix(int n, const double* xp, double* a);

/* Weights of one axis of that spline at x: the spline through (xp, y) is sum_j weight[j] y[j] and
 * its derivative with respect to x sum_j dweight[j] y[j]; `a` is the matrix above.  *segment (may
 * be NULL) receives the segment whose polynomial is evaluated: np.digitize(x, xp) - 1 with
 * x == xp[n - 1] in the last one, clamped to [0, n - 2] -- beyond the grid the outermost
 * polynomial continues.  Pure host code: the text the interpolator's gradient kernels run. */
int tc_spline_weights(int n, const double* xp, const double* a, double x, double* weight,
                      double* dweight, int* segment);

/* ---- one tabulated table (replaces the state of a `TabCorr` instance) ----------------
 *
 * tc_table_create uploads everything predict() needs from a TabCorr object
 * (tabcorr.py:356-368): the correlation matrix `tpcf_matrix` (R x P, row-major, P =
 * G (G + 1) / 2 packed lower triangle in mode auto, P = G in mode cross) and the
 * gal_type columns read at tabcorr.py:537-541, 568-570, 623.  It precomputes what the
 * reference caches lazily on `self` (pair indices, tabcorr.py:626-639; Gauss-Legendre
 * nodes, :543-546).  compute_dtype selects the arithmetic of the contraction: F64
 * (default, parity <= 1e-10) or F32 (table and accumulation in float, for BASELINE
 * configs[4]; stated tolerance 1e-5).  Occupations are always evaluated in F64.
 */
int tc_table_create(int mode, int n_bins, int n_r, int64_t n_pairs,
                    const void* tpcf_matrix, int matrix_dtype,
                    const double* n_h,
                    const double* log_prim_haloprop_min,
                    const double* log_prim_haloprop_max,
                    const double* sec_haloprop_percentile,
                    const double* prim_haloprop_dist_index, /* NULL: legacy table */
                    const uint8_t* is_central,              /* 1 = 'centrals' row */
                    int compute_dtype,
                    tc_table** table);
int tc_table_destroy(tc_table* table);
int tc_table_synchronize(tc_table* table);

/* Shape queries: n_bins, n_r, n_pairs, number of xi components with
 * TC_FLAG_SEPARATE_GAL_TYPE (3 auto / 2 cross), table bytes resident in HBM. */
int tc_table_info(const tc_table* table, int* mode, int* n_bins, int* n_r,
                  int64_t* n_pairs, int* n_components, int64_t* device_bytes);

/* TabCorr.mean_occupation(model) for a batch of Zheng07 parameter vectors
 * (tabcorr.py:465-578 with the halotools callbacks of :556-563 evaluated on device).
 * theta: (n_draws, n_theta) with columns logMmin, sigma_logM, logM0, logM1, alpha
 * [, A_cen, A_sat when TC_FLAG_ASSEMBIAS]; occupation out: (n_draws, n_bins). */
int tc_mean_occupation_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                                     int64_t n_draws, int n_gauss_prim, unsigned flags,
                                     double* occupation);

/* TabCorr.predict(model) for a batch of Zheng07 draws (tabcorr.py:580-683).
 * Outputs, without TC_FLAG_SEPARATE_GAL_TYPE: ngal (n_draws), xi (n_draws, n_r).
 * With it: ngal (n_draws, 2) [centrals, satellites]; xi (n_draws, n_components, n_r) in
 * the reference's dict order (centrals-centrals, centrals-satellites,
 * satellites-satellites | centrals, satellites). */
int tc_predict_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                             int64_t n_draws, int n_gauss_prim, unsigned flags,
                             double* ngal, double* xi);
int tc_predict_zheng07_batch_device(tc_table* table, const double* theta_device,
                                    int n_theta, int64_t n_draws, int n_gauss_prim,
                                    unsigned flags, double* ngal_device,
                                    double* xi_device);

/* Gaussian likelihood fused behind predict() (the step every
 * likelihood built on the reference performs on the host, README.md:7): for each draw
 * chi2 = (xi - data)^T precision (xi - data) over the n_r correlation function bins of
 * the total prediction.  Outputs ngal (n_draws) and chi2 (n_draws): one pair of doubles
 * per draw crosses PCIe instead of 1 + n_r. */
int tc_chi2_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                          int64_t n_draws, int n_gauss_prim, unsigned flags,
                          const double* data, const double* precision, double* ngal,
                          double* chi2);

/* The same with the draws and the results (ngal, chi2: n_draws doubles each) resident on
 * the device; data / precision are host arrays (uploaded when they change).  Enqueues and
 * returns; at most 2^18 draws per call.  Lets a multi-GPU run gather 16 bytes per draw
 * instead of 8 (1 + n_r). */
int tc_chi2_zheng07_batch_device(tc_table* table, const double* theta_device, int n_theta,
                                 int64_t n_draws, int n_gauss_prim, unsigned flags,
                                 const double* data, const double* precision,
                                 double* ngal_device, double* chi2_device);

/* Analytic gradients (extension beyond the reference): the prediction of a batch of Zheng07
 * draws together with its EXACT derivatives with respect to the five parameters (logMmin,
 * sigma_logM, logM0, logM1, alpha) -- the derivative of the function the library computes (the
 * Gauss-Legendre bin average of tabcorr.py:537-578 followed by tabcorr.py:623-650), not of the
 * underlying integral.  n_theta must be 5; flags: 0 or TC_FLAG_MODULATE_WITH_CENOCC.  Outputs:
 * ngal (n_draws), xi (n_draws, n_r), dngal (n_draws, 5), dxi (n_draws, 5, n_r).  One launch per
 * batch; ngal and xi agree with tc_predict_zheng07_batch to parity (1e-10 relative), not
 * necessarily to the bit.  A draw's results depend on the draw alone (batch-invariant by
 * construction, whatever the option "deterministic" says).  Where the value's formula divides
 * by zero (ngal = 0, sigma_logM = 0) the derivatives are what IEEE arithmetic gives (NaN or
 * inf).  TC_ERR_UNSUPPORTED with a message: a float32 compute dtype, TC_FLAG_SEPARATE_GAL_TYPE,
 * TC_FLAG_ASSEMBIAS, TC_FLAG_LEAUTHAUD11, tables whose rows do not fit the kernel's LDS (mode
 * auto: about 3 n_centrals + 6 n_satellites <= 1270 rows, i.e. at least 280 bins split evenly;
 * mode cross: any number of bins, n_r up to about 140). */
int tc_predict_grad_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                                  int64_t n_draws, int n_gauss_prim, unsigned flags,
                                  double* ngal, double* xi, double* dngal, double* dxi);
/* The same on device pointers: enqueues on one of the handle's lanes and returns. */
int tc_predict_grad_zheng07_batch_device(tc_table* table, const double* theta_device,
                                         int n_theta, int64_t n_draws, int n_gauss_prim,
                                         unsigned flags, double* ngal_device,
                                         double* xi_device, double* dngal_device,
                                         double* dxi_device);
/* chi2 = (xi - data)^T precision (xi - data) and dchi2 / dtheta_k = 2 (xi - data)^T P_sym
 * dxi / dtheta_k with P_sym = (precision + precision^T) / 2, finished in the same launch: ngal
 * (n_draws), chi2 (n_draws), dngal (n_draws, 5), dchi2 (n_draws, 5).  data / precision are host
 * arrays in both forms (uploaded when they change). */
int tc_chi2_grad_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                               int64_t n_draws, int n_gauss_prim, unsigned flags,
                               const double* data, const double* precision, double* ngal,
                               double* chi2, double* dngal, double* dchi2);
int tc_chi2_grad_zheng07_batch_device(tc_table* table, const double* theta_device, int n_theta,
                                      int64_t n_draws, int n_gauss_prim, unsigned flags,
                                      const double* data, const double* precision,
                                      double* ngal_device, double* chi2_device,
                                      double* dngal_device, double* dchi2_device);
/* The same with the Fisher matrix of the likelihood, from the derivatives the launch already
 * holds: with dxi_k the Jacobian column of parameter k (k, l = 0 .. 4 in the order above),
 *   fisher[k][l] = 1/2 sum_r dxi_k[r] (sum_s (precision[r][s] + precision[s][r]) dxi_l[s])
 *                = dxi_k^T P_sym dxi_l,
 * the Gauss-Newton normal matrix: 2 fisher is the Gauss-Newton Hessian of chi2.  A likelihood's
 * ngal term stays the caller's: dngal is returned next to it, and an outer product completes the
 * matrix.  fisher (n_draws, 5, 5): the full matrix, every pair k <= l computed once and stored to
 * both positions (bit-symmetric); the sums run over s ascending inside r ascending, so a draw's
 * matrix does not depend on its batch.  It does not depend on `data`.  Where the value's formula
 * divides by zero the entries are what IEEE arithmetic gives.  The other outputs are those of
 * tc_chi2_grad_zheng07_batch, bit for bit; arguments are checked and calls refused exactly as
 * there. */
int tc_chi2_fisher_zheng07_batch(tc_table* table, const double* theta, int n_theta,
                                 int64_t n_draws, int n_gauss_prim, unsigned flags,
                                 const double* data, const double* precision, double* ngal,
                                 double* chi2, double* dngal, double* dchi2, double* fisher);
int tc_chi2_fisher_zheng07_batch_device(tc_table* table, const double* theta_device, int n_theta,
                                        int64_t n_draws, int n_gauss_prim, unsigned flags,
                                        const double* data, const double* precision,
                                        double* ngal_device, double* chi2_device,
                                        double* dngal_device, double* dchi2_device,
                                        double* fisher_device);
/* The gradients of the model decorated with Heaviside assembly bias at the median split (what
 * TC_FLAG_ASSEMBIAS predicts): n_theta must be 7, the five Zheng07 parameters, then the strengths
 * of the centrals' and the satellites' assembly bias, and there are 7 wherever 5 stands above:
 * dngal (n_draws, 7), dxi (n_draws, 7, n_r), dchi2 (n_draws, 7), fisher (n_draws, 7, 7).  With c
 * the clip of a strength to [-1, 1] and s_b = +1 for a bin whose sec_haloprop_percentile lies
 * above 0.5, else -1: <N_cen>' = N + s_b c(A_cen) min(N, 1 - N) per quadrature node and <N_sat>'
 * = (1 + s_b c(A_sat)) N, N the plain occupations (with TC_FLAG_MODULATE_WITH_CENOCC the
 * satellites' N holds the PLAIN <N_cen>).  The derivative is that of the function computed: the
 * column of a strength beyond [-1, 1] is exactly zero, at +-1 it is the one facing inside, and
 * min(N, 1 - N) takes the branch N <= 1 - N at a tie.  flags: 0 or
 * TC_FLAG_MODULATE_WITH_CENOCC (the decoration is implied; TC_FLAG_ASSEMBIAS and every other
 * flag is TC_ERR_UNSUPPORTED).  Otherwise as the plain calls: one launch per batch, a draw's
 * results depend on the draw alone, float32 tables and tables beyond the LDS budget (8 for 6
 * quantities, 4 rows per central and 7 per satellite bin) are refused.  The likelihood calls take
 * a trailing `fisher`, which may be NULL: not asked for. */
int tc_predict_grad_assembias_batch(tc_table* table, const double* theta, int n_theta,
                                    int64_t n_draws, int n_gauss_prim, unsigned flags,
                                    double* ngal, double* xi, double* dngal, double* dxi);
int tc_predict_grad_assembias_batch_device(tc_table* table, const double* theta_device,
                                           int n_theta, int64_t n_draws, int n_gauss_prim,
                                           unsigned flags, double* ngal_device,
                                           double* xi_device, double* dngal_device,
                                           double* dxi_device);
int tc_chi2_grad_assembias_batch(tc_table* table, const double* theta, int n_theta,
                                 int64_t n_draws, int n_gauss_prim, unsigned flags,
                                 const double* data, const double* precision, double* ngal,
                                 double* chi2, double* dngal, double* dchi2, double* fisher);
int tc_chi2_grad_assembias_batch_device(tc_table* table, const double* theta_device, int n_theta,
                                        int64_t n_draws, int n_gauss_prim, unsigned flags,
                                        const double* data, const double* precision,
                                        double* ngal_device, double* chi2_device,
                                        double* dngal_device, double* dchi2_device,
                                        double* fisher_device);
/* The gradients of the Leauthaud et al. (2011) family (what TC_FLAG_LEAUTHAUD11 predicts): theta
 * is (n_draws, 14) as for the forward calls, n_theta must be 14, and the derivatives are those
 * with respect to the first eleven columns -- logm0, logm1, beta, delta, gamma, scatter, alphasat,
 * bsat, betasat, bcut, betacut; threshold, h and h_s are inputs --, 11 wherever 5 stands above:
 * dngal (n_draws, 11), dxi (n_draws, 11, n_r), dchi2 (n_draws, 11), fisher (n_draws, 11, 11).
 * The inverse stellar-to-halo mass relation is solved per quadrature node by Newton's method and
 * differentiated at the root by the implicit function theorem; the occupation is smooth, so the
 * derivative is exact everywhere.  flags: 0 or TC_FLAG_MODULATE_WITH_CENOCC (the family is
 * implied; TC_FLAG_LEAUTHAUD11, TC_FLAG_ASSEMBIAS and every other flag is TC_ERR_UNSUPPORTED).
 * Otherwise as the plain calls: one launch per batch, a draw's results depend on the draw alone,
 * float32 tables and tables beyond the LDS budget (12 for 6 quantities, 7 rows per central and
 * 12 per satellite bin) are refused.  The likelihood calls take a trailing `fisher`, which may
 * be NULL: not asked for. */
int tc_predict_grad_leauthaud11_batch(tc_table* table, const double* theta, int n_theta,
                                      int64_t n_draws, int n_gauss_prim, unsigned flags,
                                      double* ngal, double* xi, double* dngal, double* dxi);
int tc_predict_grad_leauthaud11_batch_device(tc_table* table, const double* theta_device,
                                             int n_theta, int64_t n_draws, int n_gauss_prim,
                                             unsigned flags, double* ngal_device,
                                             double* xi_device, double* dngal_device,
                                             double* dxi_device);
int tc_chi2_grad_leauthaud11_batch(tc_table* table, const double* theta, int n_theta,
                                   int64_t n_draws, int n_gauss_prim, unsigned flags,
                                   const double* data, const double* precision, double* ngal,
                                   double* chi2, double* dngal, double* dchi2, double* fisher);
int tc_chi2_grad_leauthaud11_batch_device(tc_table* table, const double* theta_device,
                                          int n_theta, int64_t n_draws, int n_gauss_prim,
                                          unsigned flags, const double* data,
                                          const double* precision, double* ngal_device,
                                          double* chi2_device, double* dngal_device,
                                          double* dchi2_device, double* fisher_device);

/* A handful of independent draws in ONE launch (the proposals of an ensemble sampler's step,
 * or the reference's un-batched predict(), README.md:72-75, for n_walkers = 1): every
 * workgroup evaluates the occupations of its draw itself, contracts its share of the table
 * and stores its partial sums and a completion word into page-locked host memory, which the
 * host polls -- no device-side combination, no stream synchronisation.  theta (n_walkers,
 * n_theta), ngal (n_walkers), xi (n_walkers, n_r): host arrays.  Total prediction only;
 * calls the path cannot serve (TC_FLAG_SEPARATE_GAL_TYPE, more than 64 walkers, several r
 * tiles, float32 tables, TC_FLAG_LEAUTHAUD11) are forwarded to tc_predict_zheng07_batch,
 * which in turn routes small eligible batches here. */
int tc_predict_zheng07_many(tc_table* table, const double* theta, int n_theta, int n_walkers,
                            int n_gauss_prim, unsigned flags, double* ngal, double* xi);
/* ONE draw against several tables in one call -- the reference's documented likelihood step
 * evaluates two: halotab_wp.predict(model), then halotab_ds.predict(model)
 * (docs/guides/overview.rst:86-92).  Every table's call is posted before the first answer is
 * waited for (its resident kernel's mailbox, or one launch on the table's own stream), so the
 * tables' round trips overlap; each table is served by the path tc_predict_zheng07_many would
 * take for it, with the same bits.  tables: 1 .. 16 different handles (any mix of modes and
 * shapes; all must accept the same theta and flags); ngal (n_tables); xi[k]: n_r(k) doubles. */
int tc_predict_zheng07_joint(tc_table* const* tables, int n_tables, const double* theta,
                             int n_theta, int n_gauss_prim, unsigned flags, double* ngal,
                             double* const* xi);

/* Asynchronous host-to-host form of the two calls above -- the SURVEY.md section 8d metric
 * (theta on the host -> (ngal, xi) on the host) at the device rate.  What it replaces in the
 * reference is the user's loop of predict() calls (README.md:72-75): an ensemble sampler
 * enqueues the batch of walker positions of step k + 1 while the results of step k are still
 * on their way back.
 *
 * theta, ngal, xi (chi2) must lie in page-locked memory (tc_host_alloc / tc_host_register),
 * else TC_ERR_INVALID.  The call enqueues upload -> occupation -> contraction ->
 * finalisation -> download on the next lane of the handle (stream + workspaces + staging,
 * rotating as the _device entry points do) and returns a ticket without synchronising;
 * copies run on the lane's stream, so the kernels of call k + 1 overlap the download of call
 * k.  The caller must not touch theta / ngal / xi of a ticket before tc_table_wait(ticket)
 * returned (tc_table_query: non-blocking test).  Tickets complete in any order; results of
 * a ticket land only in the buffers passed with it.  At most 64 tickets may be pending. */
int tc_predict_zheng07_batch_async(tc_table* table, const double* theta_pinned, int n_theta,
                                   int64_t n_draws, int n_gauss_prim, unsigned flags,
                                   double* ngal_pinned, double* xi_pinned, int64_t* ticket);
int tc_chi2_zheng07_batch_async(tc_table* table, const double* theta_pinned, int n_theta,
                                int64_t n_draws, int n_gauss_prim, unsigned flags,
                                const double* data, const double* precision,
                                double* ngal_pinned, double* chi2_pinned, int64_t* ticket);
int tc_table_wait(tc_table* table, int64_t ticket);
int tc_table_query(tc_table* table, int64_t ticket, int* done);

/* TabCorr.predict(ndarray): the operator seam of tabcorr.py:616-621 for arbitrary
 * occupation models evaluated by the caller.  occupation: (n_draws, n_bins). */
int tc_predict_occupation_batch(tc_table* table, const double* occupation,
                                int64_t n_draws, unsigned flags, double* ngal,
                                double* xi);

/* Reverse-mode derivative at that seam (extension beyond the reference): the vector-Jacobian
 * product of (ngal, xi) = predict(occupation) with respect to the occupation array, for every
 * occupation model at once -- the caller contracts g_occupation with its own d<N>/dtheta.  With
 * w = occupation . n_h and the cotangents g_ngal (n_draws, or NULL = 0) and g_xi (n_draws, n_r):
 *   auto:  g_occ_i = n_h_i [g_ngal + (2 / ngal^2) sum_r g_r (S_r w)_i - (2 / ngal) sum_r g_r xi_r]
 *   cross: g_occ_i = n_h_i [g_ngal + (1 / ngal) sum_r g_r T_ri - (1 / ngal) sum_r g_r xi_r]
 * Outputs: ngal (n_draws), xi (n_draws, n_r), g_occupation (n_draws, n_bins) in the row order of
 * `occupation`.  One launch per batch (host arrays: per slab of draws); ngal and xi agree with
 * tc_predict_occupation_batch to parity (1e-10 relative), not necessarily to the bit.  A draw's
 * results depend on the draw alone.  Where ngal = 0 the results are what IEEE arithmetic gives
 * (NaN or inf).  flags must be 0.  TC_ERR_UNSUPPORTED with a message: TC_FLAG_SEPARATE_GAL_TYPE,
 * a float32 compute dtype, tables whose rows do not fit the kernel's LDS (mode auto: 2 n_bins +
 * 6 n_r + 3 <= 1280 rows of 128 bytes; mode cross: any number of bins, 3 n_r + 66 <= 1280). */
int tc_predict_occupation_vjp_batch(tc_table* table, const double* occupation, int64_t n_draws,
                                    unsigned flags, const double* g_ngal, const double* g_xi,
                                    double* ngal, double* xi, double* g_occupation);
/* The same on device pointers: enqueues on the next lane of the handle and returns. */
int tc_predict_occupation_vjp_batch_device(tc_table* table, const double* occupation_device,
                                           int64_t n_draws, unsigned flags,
                                           const double* g_ngal_device,
                                           const double* g_xi_device, double* ngal_device,
                                           double* xi_device, double* g_occupation_device);
/* The likelihood form: chi2 = (xi - data)^T precision (xi - data) and dchi2 / docc, i.e. the VJP
 * with g_xi = 2 P_sym (xi - data), P_sym = (precision + precision^T) / 2, and g_ngal = 0, formed
 * in the same launch from its own xi (mode auto runs the matrix product twice; nothing leaves
 * the device in between).  ngal, chi2 (n_draws), dchi2_docc (n_draws, n_bins); dngal / docc is
 * n_h.  data / precision are host arrays in both forms (uploaded when they change). */
int tc_chi2_occupation_grad_batch(tc_table* table, const double* occupation, int64_t n_draws,
                                  unsigned flags, const double* data, const double* precision,
                                  double* ngal, double* chi2, double* dchi2_docc);
int tc_chi2_occupation_grad_batch_device(tc_table* table, const double* occupation_device,
                                         int64_t n_draws, unsigned flags, const double* data,
                                         const double* precision, double* ngal_device,
                                         double* chi2_device, double* dchi2_docc_device);

/* ---- interpolation over a grid of tables (replaces `Interpolator`) -------------------
 *
 * tables: K handles in tabcorr_list order.  points: (K, n_dim) extra-parameter values
 * of each table (the rows of param_dict_table, interpolator.py:14-61).  The library
 * validates the grid (TC_ERR_INVALID if it is not one, interpolator.py:45-57), builds
 * the spline matrices (interpolator.py:219-272) and shares occupations between tables
 * whose gal_type tables are identical (interpolator.py:63-70).
 */
int tc_interp_create(tc_table* const* tables, int n_tables, int n_dim,
                     const double* points, tc_interp** interp);
int tc_interp_destroy(tc_interp* interp);
int tc_interp_synchronize(tc_interp* interp);
/* abscissae of dimension d (sorted unique values): returns n and copies min(n, size). */
int tc_interp_axis(const tc_interp* interp, int dim, int* n, double* xp, int size);

/* Interpolator.predict(model) for a batch (interpolator.py:124-216): theta as above,
 * x: (n_draws, n_dim) values of the extra parameters (model.param_dict[key]).
 * Out-of-range x is clamped to the outermost spline segment (extrapolate=True,
 * interpolator.py:327-328); the extrapolate=False ValueError is raised by the host
 * class before the call.  Outputs as tc_predict_zheng07_batch. */
int tc_interp_predict_zheng07_batch(tc_interp* interp, const double* theta, int n_theta,
                                    const double* x, int64_t n_draws, int n_gauss_prim,
                                    unsigned flags, double* ngal, double* xi);
int tc_interp_predict_zheng07_batch_device(tc_interp* interp, const double* theta_device,
                                           int n_theta, const double* x_device,
                                           int64_t n_draws, int n_gauss_prim,
                                           unsigned flags, double* ngal_device,
                                           double* xi_device);

/* The fused Gaussian likelihood (tc_chi2_zheng07_batch) behind Interpolator.predict: what an
 * MCMC over interpolated tables (cosmology / phase-space parameters next to the HOD) needs per
 * draw.  Host arrays in, ngal (n_draws) and chi2 (n_draws) out; the `_device` form keeps the
 * draws, x and the results on the device (data / precision are host arrays, uploaded when
 * they change), enqueues and returns. */
int tc_interp_chi2_zheng07_batch(tc_interp* interp, const double* theta, int n_theta,
                                 const double* x, int64_t n_draws, int n_gauss_prim,
                                 unsigned flags, const double* data, const double* precision,
                                 double* ngal, double* chi2);
int tc_interp_chi2_zheng07_batch_device(tc_interp* interp, const double* theta_device,
                                        int n_theta, const double* x_device, int64_t n_draws,
                                        int n_gauss_prim, unsigned flags, const double* data,
                                        const double* precision, double* ngal_device,
                                        double* chi2_device);

/* Analytic gradients behind Interpolator.predict (extension, as tc_predict_grad_zheng07_batch):
 * the interpolated prediction of a batch of draws (theta, x) with its exact derivatives with
 * respect to the five Zheng07 parameters and the D = n_dim extra parameters, in one launch per
 * batch.  Derivative columns: the five Zheng07 parameters, then the extra parameters in axis
 * order: ngal (n_draws), xi (n_draws, n_r), dngal (n_draws, 5 + D), dxi (n_draws, 5 + D, n_r).
 * The spline is C2, so the results have no kink in x; a clamped x (beyond the grid) gets the
 * derivative of the outermost polynomial.  n_theta must be 5; flags 0 or
 * TC_FLAG_MODULATE_WITH_CENOCC.  TC_ERR_UNSUPPORTED as for a table (float32 tables,
 * TC_FLAG_SEPARATE_GAL_TYPE, TC_FLAG_ASSEMBIAS, TC_FLAG_LEAUTHAUD11) and for a grid whose rows do
 * not fit the kernel's LDS: a table's rows plus 64 D rows of weights and (6 + D) n_r rows of
 * accumulators (twice those in mode cross) within 160 KiB.  Batch-invariant by construction.
 * Host arrays run on lane 0; the `_device` forms enqueue on the next lane and return. */
int tc_interp_predict_grad_zheng07_batch(tc_interp* interp, const double* theta, int n_theta,
                                         const double* x, int64_t n_draws, int n_gauss_prim,
                                         unsigned flags, double* ngal, double* xi, double* dngal,
                                         double* dxi);
int tc_interp_predict_grad_zheng07_batch_device(tc_interp* interp, const double* theta_device,
                                                int n_theta, const double* x_device,
                                                int64_t n_draws, int n_gauss_prim, unsigned flags,
                                                double* ngal_device, double* xi_device,
                                                double* dngal_device, double* dxi_device);
/* ... and of the likelihood (tc_chi2_grad_zheng07_batch): ngal, chi2 (n_draws), dngal, dchi2
 * (n_draws, 5 + D); data / precision are host arrays in both forms. */
int tc_interp_chi2_grad_zheng07_batch(tc_interp* interp, const double* theta, int n_theta,
                                      const double* x, int64_t n_draws, int n_gauss_prim,
                                      unsigned flags, const double* data, const double* precision,
                                      double* ngal, double* chi2, double* dngal, double* dchi2);
int tc_interp_chi2_grad_zheng07_batch_device(tc_interp* interp, const double* theta_device,
                                             int n_theta, const double* x_device, int64_t n_draws,
                                             int n_gauss_prim, unsigned flags, const double* data,
                                             const double* precision, double* ngal_device,
                                             double* chi2_device, double* dngal_device,
                                             double* dchi2_device);
/* ... with the Fisher matrix of the likelihood (tc_chi2_fisher_zheng07_batch: the same
 * definition, fisher[k][l] = dxi_k^T P_sym dxi_l) over the 5 + D differentiated quantities, the
 * five Zheng07 parameters first, then the extra parameters in axis order: fisher (n_draws, 5 + D,
 * 5 + D).  The other outputs are those of tc_interp_chi2_grad_zheng07_batch, bit for bit;
 * arguments are checked and calls refused exactly as there. */
int tc_interp_chi2_fisher_zheng07_batch(tc_interp* interp, const double* theta, int n_theta,
                                        const double* x, int64_t n_draws, int n_gauss_prim,
                                        unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dngal, double* dchi2, double* fisher);
int tc_interp_chi2_fisher_zheng07_batch_device(tc_interp* interp, const double* theta_device,
                                               int n_theta, const double* x_device,
                                               int64_t n_draws, int n_gauss_prim, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dngal_device, double* dchi2_device,
                                               double* fisher_device);
/* The interpolator's gradients for the model decorated with assembly bias (as
 * tc_predict_grad_assembias_batch: n_theta must be 7, flags 0 or TC_FLAG_MODULATE_WITH_CENOCC):
 * 7 + D columns, the seven model parameters first -- dngal (n_draws, 7 + D), dxi (n_draws, 7 + D,
 * n_r), dchi2 (n_draws, 7 + D), fisher (n_draws, 7 + D, 7 + D), which may be NULL. */
int tc_interp_predict_grad_assembias_batch(tc_interp* interp, const double* theta, int n_theta,
                                           const double* x, int64_t n_draws, int n_gauss_prim,
                                           unsigned flags, double* ngal, double* xi,
                                           double* dngal, double* dxi);
int tc_interp_predict_grad_assembias_batch_device(tc_interp* interp, const double* theta_device,
                                                  int n_theta, const double* x_device,
                                                  int64_t n_draws, int n_gauss_prim,
                                                  unsigned flags, double* ngal_device,
                                                  double* xi_device, double* dngal_device,
                                                  double* dxi_device);
int tc_interp_chi2_grad_assembias_batch(tc_interp* interp, const double* theta, int n_theta,
                                        const double* x, int64_t n_draws, int n_gauss_prim,
                                        unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dngal, double* dchi2, double* fisher);
int tc_interp_chi2_grad_assembias_batch_device(tc_interp* interp, const double* theta_device,
                                               int n_theta, const double* x_device,
                                               int64_t n_draws, int n_gauss_prim, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dngal_device, double* dchi2_device,
                                               double* fisher_device);

/* The interpolator's gradients for the Leauthaud et al. (2011) family (as
 * tc_predict_grad_leauthaud11_batch: theta (n_draws, 14), n_theta must be 14, flags 0 or
 * TC_FLAG_MODULATE_WITH_CENOCC -- the family is implied, every other flag is
 * TC_ERR_UNSUPPORTED): 11 + D columns, the eleven differentiated model parameters first -- dngal
 * (n_draws, 11 + D), dxi (n_draws, 11 + D, n_r), dchi2 (n_draws, 11 + D), fisher (n_draws, 11 + D,
 * 11 + D), which may be NULL.  The LDS budget: 12 for 6 quantities, 7 rows per central and 12 per
 * satellite bin in mode auto; in mode cross one slab of 32 bins (12 x 33 rows with the totals)
 * where the other families keep 64.  Grids of up to four dimensions (12 + D quantities per draw,
 * of 16): beyond them TC_ERR_UNSUPPORTED. */
int tc_interp_predict_grad_leauthaud11_batch(tc_interp* interp, const double* theta, int n_theta,
                                             const double* x, int64_t n_draws, int n_gauss_prim,
                                             unsigned flags, double* ngal, double* xi,
                                             double* dngal, double* dxi);
int tc_interp_predict_grad_leauthaud11_batch_device(tc_interp* interp, const double* theta_device,
                                                    int n_theta, const double* x_device,
                                                    int64_t n_draws, int n_gauss_prim,
                                                    unsigned flags, double* ngal_device,
                                                    double* xi_device, double* dngal_device,
                                                    double* dxi_device);
int tc_interp_chi2_grad_leauthaud11_batch(tc_interp* interp, const double* theta, int n_theta,
                                          const double* x, int64_t n_draws, int n_gauss_prim,
                                          unsigned flags, const double* data,
                                          const double* precision, double* ngal, double* chi2,
                                          double* dngal, double* dchi2, double* fisher);
int tc_interp_chi2_grad_leauthaud11_batch_device(tc_interp* interp, const double* theta_device,
                                                 int n_theta, const double* x_device,
                                                 int64_t n_draws, int n_gauss_prim, unsigned flags,
                                                 const double* data, const double* precision,
                                                 double* ngal_device, double* chi2_device,
                                                 double* dngal_device, double* dchi2_device,
                                                 double* fisher_device);

/* The occupation seam of an interpolator (extension): the interface for ANY occupation model.
 * The tables of an interpolator fall into n_classes classes of identical halo tables
 * (interpolator.py:63-70), numbered by first appearance in the list.  tc_interp_info: table_class
 * holds n_tables entries (the class of every table), class_table n_classes (the first table of
 * every class); any pointer may be NULL.
 * occupation: (n_draws, n_classes, n_bins) mean occupations, class v's row in the gal_type row
 * order of that class's tables; x: (n_draws, n_dim), out of range clamped to the outermost
 * polynomial as above.  With c_t(x) the spline weight of table t: ngal = sum_t c_t ngal_t and
 * xi_r = sum_t c_t xi_t,r (ngal (n_draws), xi (n_draws, n_r)).
 * tc_interp_predict_occupation_vjp_batch: with the cotangents g_ngal (n_draws; NULL = 0) and g_xi
 * (n_draws, n_r) also g_occupation (n_draws, n_classes, n_bins) = g_ngal dngal/dn + sum_r g_r
 * dxi_r/dn and g_x (n_draws, n_dim) likewise with respect to x.  g_xi, g_occupation and g_x all
 * NULL: the forward-only form -- (ngal, xi) alone, the same bits, no adjoint work; some but not
 * all of them NULL is TC_ERR_INVALID.
 * tc_interp_chi2_occupation_grad_batch: chi2 (n_draws) of the interpolated prediction against
 * data (n_r) and precision (n_r, n_r) -- host arrays in both forms, uploaded when they change --
 * with dchi2_docc (n_draws, n_classes, n_bins), dchi2_dx (n_draws, n_dim) and dngal_dx (n_draws,
 * n_dim); the three all NULL: the forward-only form, some but not all TC_ERR_INVALID.  The
 * cotangent 2 P_sym (xi - data) is formed in the launch, which walks the tables twice.
 * One launch per batch; a draw's results depend on the draw alone, not on the batch, its place in
 * it or the entry point.  TC_ERR_UNSUPPORTED with a message, the interpolator and its tables
 * staying usable: a float32 compute dtype, TC_FLAG_SEPARATE_GAL_TYPE, any other flag, and a
 * workgroup beyond 160 KiB of LDS ("LDS" in the message) -- rows of 128 bytes: 64 n_dim of
 * spline weights, (2 + n_dim) n_r + 4 of cotangents, results and per-draw sums, and in mode auto
 * 3 n_bins + 1 + 5 n_r (the class in flight: w, the table's and the class's sum_r g_r U_ri, the
 * per-wave partial q_r), in mode cross 64 + (1 + n_dim) n_r (one slab of w for any number of
 * bins, the class's weighted products).
 * Host arrays run slab-wise on lane 0 of the interpolator; the `_device` forms enqueue on its
 * next lane and return (tc_interp_synchronize waits). */
int tc_interp_info(const tc_interp* interp, int* n_tables, int* n_classes, int* table_class,
                   int* class_table);
int tc_interp_predict_occupation_vjp_batch(tc_interp* interp, const double* occupation,
                                           const double* x, int64_t n_draws, unsigned flags,
                                           const double* g_ngal, const double* g_xi, double* ngal,
                                           double* xi, double* g_occupation, double* g_x);
int tc_interp_predict_occupation_vjp_batch_device(tc_interp* interp,
                                                  const double* occupation_device,
                                                  const double* x_device, int64_t n_draws,
                                                  unsigned flags, const double* g_ngal_device,
                                                  const double* g_xi_device, double* ngal_device,
                                                  double* xi_device, double* g_occupation_device,
                                                  double* g_x_device);
int tc_interp_chi2_occupation_grad_batch(tc_interp* interp, const double* occupation,
                                         const double* x, int64_t n_draws, unsigned flags,
                                         const double* data, const double* precision, double* ngal,
                                         double* chi2, double* dchi2_docc, double* dchi2_dx,
                                         double* dngal_dx);
int tc_interp_chi2_occupation_grad_batch_device(tc_interp* interp,
                                                const double* occupation_device,
                                                const double* x_device, int64_t n_draws,
                                                unsigned flags, const double* data,
                                                const double* precision, double* ngal_device,
                                                double* chi2_device, double* dchi2_docc_device,
                                                double* dchi2_dx_device, double* dngal_dx_device);

/* Joint likelihood of several tables (extension): the data vector of the reference's documented
 * likelihood step is the concatenation of two tables' predictions, (w_p, DeltaSigma)
 * (docs/guides/overview.rst:86-92), and its covariance couples them.  A joint handle over 1 .. 16
 * tables that share one halo table evaluates a batch of draws against ALL of them in one launch:
 * the occupations and their derivatives once per draw, then every table's contraction (mode auto
 * and mode cross may be mixed) into its rows r_offset[t] .. r_offset[t] + n_r[t] of the N =
 * sum_t n_r[t] concatenated ones, in list order.
 *
 * tc_joint_create: every table on the same device, with a float64 compute dtype and the bins
 * (all gal_type columns) of the first one, no handle twice; anything else is TC_ERR_INVALID with
 * a message naming the table.  The joint owns no table: it works through them (Conventions);
 * tc_joint_destroy does not touch them.  tc_joint_info: r_offset holds n_tables entries; any pointer may be
 * NULL. */
int tc_joint_create(tc_table* const* tables, int n_tables, tc_joint** joint);
int tc_joint_destroy(tc_joint* joint);
int tc_joint_synchronize(tc_joint* joint);
int tc_joint_info(const tc_joint* joint, int* n_tables, int* n_r_total, int* r_offset);
/* The concatenated prediction with its exact derivatives (tc_predict_grad_zheng07_batch): ngal
 * (n_draws), xi (n_draws, N), dngal (n_draws, 5), dxi (n_draws, 5, N) -- the tables share their
 * bins, so there is one ngal per draw.  flags selects the family: 0 or
 * TC_FLAG_MODULATE_WITH_CENOCC plain Zheng07 (n_theta 5); with TC_FLAG_ASSEMBIAS the model
 * decorated with assembly bias (tc_predict_grad_assembias_batch: n_theta 7, and 7 wherever 5
 * stands).  TC_ERR_UNSUPPORTED with a message: TC_FLAG_LEAUTHAUD11, TC_FLAG_SEPARATE_GAL_TYPE,
 * any other flag, and a joint beyond the LDS of a workgroup: the rows of w and dw of every bin (3
 * per central and 6 per satellite bin; 4 and 7 decorated) plus 6 (8) rows of totals plus, for the
 * likelihood, 6 N (8 N) rows of 128 bytes within 160 KiB.  Every joint keeps the rows in LDS, so
 * a joint of mode-cross tables with more bins than that admits is refused although each table
 * alone is served.
 * One launch per batch; a draw's results depend on the draw alone (batch-invariant by
 * construction), and a row's arithmetic does not depend on the wave that runs it.  A joint of ONE
 * table returns the bits of that table's own tc_predict_grad_* / tc_chi2_grad_* /
 * tc_chi2_fisher_* call.  Where ngal = 0 the results are what IEEE arithmetic gives.
 * Host arrays run slab-wise on lane 0 of the first table; the `_device` forms enqueue on its next
 * lane and return (tc_joint_synchronize waits). */
int tc_joint_predict_grad_batch(tc_joint* joint, const double* theta, int n_theta,
                                int64_t n_draws, int n_gauss_prim, unsigned flags, double* ngal,
                                double* xi, double* dngal, double* dxi);
int tc_joint_predict_grad_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                       int64_t n_draws, int n_gauss_prim, unsigned flags,
                                       double* ngal_device, double* xi_device,
                                       double* dngal_device, double* dxi_device);
/* chi2, its gradient and the Fisher matrix of the joint data vector, finished in the same launch
 * against the full precision matrix: data (N) and precision (N, N) in the concatenated order,
 * host arrays in both forms (uploaded when they change).  chi2 (n_draws), dchi2 (n_draws, 5),
 * fisher (n_draws, 5, 5) -- which may be NULL: not asked for -- are defined as by
 * tc_chi2_fisher_zheng07_batch with N for n_r: P_sym = (precision + precision^T) / 2, the sums
 * over s ascending inside r ascending, every pair k <= l computed once (bit-symmetric); fisher
 * does not depend on `data`, and the other outputs do not depend on whether it is asked for. */
int tc_joint_chi2_grad_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                             int n_gauss_prim, unsigned flags, const double* data,
                             const double* precision, double* ngal, double* chi2, double* dngal,
                             double* dchi2, double* fisher);
int tc_joint_chi2_grad_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                    int64_t n_draws, int n_gauss_prim, unsigned flags,
                                    const double* data, const double* precision,
                                    double* ngal_device, double* chi2_device,
                                    double* dngal_device, double* dchi2_device,
                                    double* fisher_device);
/* The forward form, what an ensemble sampler asks per step: the concatenated prediction -- ngal
 * (n_draws), xi (n_draws, N) -- or chi2 (n_draws) of the joint data vector against the full
 * precision matrix, chi2 = (xi - data)^T precision (xi - data) with xi never stored, in ONE launch
 * per batch without any derivative: the occupations once per draw, every mode-auto table's packed
 * triangle (its own forward unit layout) on the matrix cores, every mode-cross table by one fma
 * chain per row over the bins in library order.  The arguments are those of
 * tc_joint_chi2_grad_batch without the derivative outputs; n_theta 5, or 7 with
 * TC_FLAG_ASSEMBIAS; flags may also hold TC_FLAG_MODULATE_WITH_CENOCC.  data and precision are
 * host arrays in both forms (uploaded when they change).
 * TC_ERR_UNSUPPORTED with a message, the joint and its tables staying usable:
 * TC_FLAG_SEPARATE_GAL_TYPE, TC_FLAG_LEAUTHAUD11, any other flag; a mode-auto table of more than
 * 20 correlation function bins (one r tile) or without the unit layout of the one-launch form
 * (more than 248 bins); a workgroup beyond 160 KiB of LDS: 8 x (max(64 x bins in whole fours,
 * 65 N) + max(2306, N (N + 1)) + 1024 + 256 N) bytes.
 * A draw's results depend on the draw alone: not on the batch, its place in it, or the entry
 * point; ngal does not depend on the tables.  Where ngal = 0 the results are what IEEE arithmetic
 * gives.  Host arrays take the forward path of the tables (page-locked staging for small calls,
 * overlapping chunks beyond) on the first table's staging areas and lanes; the `_device` forms
 * enqueue on its next lane and return (tc_joint_synchronize waits). */
int tc_joint_predict_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                           int n_gauss_prim, unsigned flags, double* ngal, double* xi);
int tc_joint_predict_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                                  int64_t n_draws, int n_gauss_prim, unsigned flags,
                                  double* ngal_device, double* xi_device);
int tc_joint_chi2_batch(tc_joint* joint, const double* theta, int n_theta, int64_t n_draws,
                        int n_gauss_prim, unsigned flags, const double* data,
                        const double* precision, double* ngal, double* chi2);
int tc_joint_chi2_batch_device(tc_joint* joint, const double* theta_device, int n_theta,
                               int64_t n_draws, int n_gauss_prim, unsigned flags,
                               const double* data, const double* precision, double* ngal_device,
                               double* chi2_device);
/* The occupation seam of a joint, for ANY occupation model (tc_predict_occupation_vjp_batch and
 * tc_chi2_occupation_grad_batch with N for n_r, in ONE launch per batch for all the tables):
 * occupation (n_draws, n_bins) in gal_type row order; the concatenated prediction ngal (n_draws),
 * xi (n_draws, N); and for cotangents g_ngal (n_draws; NULL = 0) and g_xi (n_draws, N) the
 * vector-Jacobian product g_occupation (n_draws, n_bins), gal_type row order:
 *   g_occ,i = n_h,i [ g_ngal + (2 / ngal^2) sum_auto g_r U_ri + (1 / ngal) sum_cross g_r T_ri
 *                     - (2 / ngal) sum_auto g_r xi_r - (1 / ngal) sum_cross g_r xi_r ]
 * with U_r = S_r w of a mode-auto table's row and T_r the matrix row of a mode-cross one.  g_xi and
 * g_occupation both NULL: the forward-only form, (ngal, xi) alone; exactly one of them NULL is
 * TC_ERR_INVALID.  flags must be 0 (TC_ERR_INVALID otherwise).
 * tc_joint_chi2_occupation_grad_batch: chi2 = (xi - data)^T precision (xi - data) of the joint
 * data vector and dchi2_docc = the product above with g = 2 P_sym (xi - data), g_ngal = 0, formed
 * in the launch from its own xi -- the off-diagonal blocks of `precision` couple the tables.
 * dchi2_docc may be NULL: not asked for, (ngal, chi2) alone with one product per mode-auto table;
 * the other outputs do not depend on whether it is asked for.  data (N) and precision (N, N) are
 * host arrays in both forms (uploaded when they change).
 * Contracted with the caller's own d<N>/dtheta the results are the gradient for every occupation
 * model, Leauthaud11 among them (examples/example_joint_custom_model_grad.py).
 * One launch per batch; a draw's results depend on the draw alone, not on the batch, its place in
 * it or the entry point, and a row's arithmetic does not depend on the wave that runs it.  A joint
 * of ONE table returns the bits of that table's own tc_predict_occupation_vjp_batch /
 * tc_chi2_occupation_grad_batch call.  Where ngal = 0 the results are what IEEE arithmetic gives.
 * TC_ERR_UNSUPPORTED with a message naming the bytes, the joint and its tables staying usable: a
 * workgroup beyond 160 KiB of LDS, 128 x (2 bins + 1 + max(4 N_auto, N) + 2 N + 3) bytes with
 * N_auto the rows of the mode-auto tables (every bin stays in LDS, also for mode-cross tables).
 * Host arrays run slab-wise on lane 0 of the first table; the `_device` forms enqueue on its next
 * lane and return (tc_joint_synchronize waits). */
int tc_joint_predict_occupation_vjp_batch(tc_joint* joint, const double* occupation,
                                          int64_t n_draws, unsigned flags, const double* g_ngal,
                                          const double* g_xi, double* ngal, double* xi,
                                          double* g_occupation);
int tc_joint_predict_occupation_vjp_batch_device(tc_joint* joint, const double* occupation_device,
                                                 int64_t n_draws, unsigned flags,
                                                 const double* g_ngal_device,
                                                 const double* g_xi_device, double* ngal_device,
                                                 double* xi_device, double* g_occupation_device);
int tc_joint_chi2_occupation_grad_batch(tc_joint* joint, const double* occupation,
                                        int64_t n_draws, unsigned flags, const double* data,
                                        const double* precision, double* ngal, double* chi2,
                                        double* dchi2_docc);
int tc_joint_chi2_occupation_grad_batch_device(tc_joint* joint, const double* occupation_device,
                                               int64_t n_draws, unsigned flags,
                                               const double* data, const double* precision,
                                               double* ngal_device, double* chi2_device,
                                               double* dchi2_docc_device);

/* Joint likelihood of several interpolators (extension): the reference's AbacusSummit database
 * and its own suite read TWO interpolators, `wp` and `ds`, built over the same grid of simulations,
 * for one model; the covariance of the data vector (w_p, DeltaSigma) couples them, and the fit's
 * parameters are the model's AND the grid's extra parameters x.  A joint handle over 1 .. 16
 * interpolators evaluates a batch of draws (theta, x) against ALL of them in one launch: the
 * occupations of every class of halo tables once, every member's contraction at every grid node
 * (a member is mode auto or mode cross throughout; members may differ) into its rows r_offset[m]
 * .. r_offset[m] + n_r[m] of the N = sum_m n_r[m] concatenated ones, in list order.
 *
 * tc_joint_interp_create: every member on the same device and of float64 tables, no handle twice,
 * the same axes (bit-identical abscissae) and grid nodes as member 0 -- the members' LIST orders
 * may differ: tables are matched by grid node --, and at every node the bins (all gal_type
 * columns) of member 0's table there; anything else is TC_ERR_INVALID with a message naming the
 * member.  The walk over the grid is member 0's.  The joint owns no member and no table: it
 * works through them (Conventions: a call excludes calls on any member and any of their tables);
 * tc_joint_interp_destroy does not touch them.  tc_joint_interp_info: r_offset holds n_members
 * entries; any pointer may be NULL. */
int tc_joint_interp_create(tc_interp* const* members, int n_members, tc_joint_interp** joint);
int tc_joint_interp_destroy(tc_joint_interp* joint);
int tc_joint_interp_synchronize(tc_joint_interp* joint);
int tc_joint_interp_info(const tc_joint_interp* joint, int* n_members, int* n_dim, int* n_r_total,
                         int* r_offset);
/* The concatenated prediction with its exact derivatives (tc_interp_predict_grad_zheng07_batch
 * with N for n_r): ngal (n_draws), xi (n_draws, N), dngal (n_draws, 5 + n_dim), dxi (n_draws,
 * 5 + n_dim, N), the model's columns first.  flags selects the family as for tc_joint_*: with
 * TC_FLAG_ASSEMBIAS n_theta is 7, and 7 stands wherever 5 does.
 * One of two forms, chosen from the members' modes alone: a member of mode auto -- every bin's
 * rows stay in LDS (the budget of the interpolator's mode-auto kernel with N rows, plus
 * (6 + n_dim) rows per result row of the mode-cross members); all members mode cross -- the bins
 * in slabs, any number of them (the budget of the interpolator's mode-cross kernel with N rows).
 * A joint beyond the 160 KiB of a workgroup is TC_ERR_UNSUPPORTED with a message; the members
 * stay usable.  A draw's results depend on the draw alone; the order of every sum is member 0's
 * walk.  The rows of a mode-auto member, and of every member of an all-cross joint, are the bits
 * of that member's own tc_interp_predict_grad_* call where its list agrees node for node with
 * member 0's; ngal and dngal are member 0's bits; a joint of ONE member returns that member's
 * bits in every form.
 * Host arrays run slab-wise on lane 0 of member 0; the `_device` forms enqueue on its next lane
 * and return (tc_joint_interp_synchronize waits). */
int tc_joint_interp_predict_grad_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                       const double* x, int64_t n_draws, int n_gauss_prim,
                                       unsigned flags, double* ngal, double* xi, double* dngal,
                                       double* dxi);
int tc_joint_interp_predict_grad_batch_device(tc_joint_interp* joint, const double* theta_device,
                                              int n_theta, const double* x_device,
                                              int64_t n_draws, int n_gauss_prim, unsigned flags,
                                              double* ngal_device, double* xi_device,
                                              double* dngal_device, double* dxi_device);
/* chi2, its gradient and the Fisher matrix over (theta, x) of the joint data vector against the
 * full (N, N) precision matrix, in the same launch (tc_joint_chi2_grad_batch with 5 + n_dim
 * columns): fisher (n_draws, 5 + n_dim, 5 + n_dim) may be NULL: not asked for. */
int tc_joint_interp_chi2_grad_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                    const double* x, int64_t n_draws, int n_gauss_prim,
                                    unsigned flags, const double* data, const double* precision,
                                    double* ngal, double* chi2, double* dngal, double* dchi2,
                                    double* fisher);
int tc_joint_interp_chi2_grad_batch_device(tc_joint_interp* joint, const double* theta_device,
                                           int n_theta, const double* x_device, int64_t n_draws,
                                           int n_gauss_prim, unsigned flags, const double* data,
                                           const double* precision, double* ngal_device,
                                           double* chi2_device, double* dngal_device,
                                           double* dchi2_device, double* fisher_device);
/* The forward form of a joint of interpolators, what an ensemble sampler over (theta, x) asks per
 * step (tc_joint_predict_batch / tc_joint_chi2_batch with the grid's x): ngal (n_draws) and the
 * concatenated prediction xi (n_draws, N), or chi2 (n_draws) = (xi - data)^T precision (xi - data)
 * of the joint data vector against the full (N, N) precision matrix with xi never stored, in ONE
 * launch per batch without any derivative, 64 draws per workgroup.  With c_k(x) the
 * tensor-product spline weight of grid node k (x clamped to the outermost segment) and v(k) the
 * class of halo tables at node k: ngal = sum_k c_k ngal_v(k), and per member m and row r
 * xi[r_offset[m] + r] = sum_k c_k xi_r^(m,k), xi_r^(m,k) = d^T S_r d / ngal_v^2 over the packed
 * triangle of the member's table at node k (mode auto) or T_r . d / ngal_v (mode cross) -- the
 * semantics of tc_interp_predict_zheng07_batch per member.  The occupations of a class are
 * evaluated once for all members; a mode-auto member's table runs in its own forward unit layout
 * on the matrix cores, a mode-cross member's by one fma chain per (node, row, draw) over the bins
 * in library order.  The arguments are those of tc_joint_interp_chi2_grad_batch without the
 * derivative outputs; n_theta 5, or 7 with TC_FLAG_ASSEMBIAS; flags may also hold
 * TC_FLAG_MODULATE_WITH_CENOCC.  data and precision are host arrays in both forms (uploaded when
 * they change).
 * One of two forms, chosen from the members' modes alone.  Rows form (a member is mode auto):
 * every bin's densities of the class in flight stay in LDS; a workgroup needs the bytes of
 * tc_joint_predict_batch for N rows plus 512 x (sum of the axes' nodes + 2).  Slab form (every
 * member mode cross): the bins in slabs of 64, any number of them; 8 x (max(4096, 65 N) +
 * max(2306, N (N + 1)) + 1024 + 128 N + 64 x (sum of the axes' nodes + 2)) bytes.
 * TC_ERR_UNSUPPORTED with a message naming the bytes or the limit, the joint and its members
 * staying usable: TC_FLAG_SEPARATE_GAL_TYPE, TC_FLAG_LEAUTHAUD11, any other flag; a mode-auto
 * member of more than 20 correlation function bins (one r tile) or more than 248 bins (no unit
 * layout of the one-launch form); a workgroup beyond 160 KiB of LDS.
 * Guarantees: ONE form per joint.  A draw's results depend on the draw alone: not on the batch
 * size, the draw's place in the batch, or the host or device entry.  The ngal of
 * tc_joint_interp_chi2_batch is bit for bit that of tc_joint_interp_predict_batch, and it does
 * not depend on which members are in the joint (only on member 0's walk over the grid).
 * Permuting the members returns the same bits block for block (the members' lists agreeing), and
 * so does permuting the LIST of a member other than member 0: tables are matched by grid node,
 * the walk is member 0's.  No bit claim is made against tc_interp_predict_zheng07_batch, whose
 * kernels cut a draw's sums where the batch size puts them.
 * Host arrays take the forward path of the tables (page-locked staging for small calls,
 * overlapping chunks beyond) on member 0's staging areas and lanes; the `_device` forms enqueue on
 * its next lane and return (tc_joint_interp_synchronize waits).  There are no asynchronous
 * entries. */
int tc_joint_interp_predict_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                                  const double* x, int64_t n_draws, int n_gauss_prim,
                                  unsigned flags, double* ngal, double* xi);
int tc_joint_interp_predict_batch_device(tc_joint_interp* joint, const double* theta_device,
                                         int n_theta, const double* x_device, int64_t n_draws,
                                         int n_gauss_prim, unsigned flags, double* ngal_device,
                                         double* xi_device);
int tc_joint_interp_chi2_batch(tc_joint_interp* joint, const double* theta, int n_theta,
                               const double* x, int64_t n_draws, int n_gauss_prim, unsigned flags,
                               const double* data, const double* precision, double* ngal,
                               double* chi2);
int tc_joint_interp_chi2_batch_device(tc_joint_interp* joint, const double* theta_device,
                                      int n_theta, const double* x_device, int64_t n_draws,
                                      int n_gauss_prim, unsigned flags, const double* data,
                                      const double* precision, double* ngal_device,
                                      double* chi2_device);

/* Asynchronous host-to-host forms (page-locked theta, x, outputs; see
 * tc_predict_zheng07_batch_async): upload, kernels and download of a call on one of the
 * interpolator's two lanes (stream + workspaces), consecutive calls alternating between them. */
int tc_interp_predict_zheng07_batch_async(tc_interp* interp, const double* theta_pinned,
                                          int n_theta, const double* x_pinned, int64_t n_draws,
                                          int n_gauss_prim, unsigned flags, double* ngal_pinned,
                                          double* xi_pinned, int64_t* ticket);
int tc_interp_chi2_zheng07_batch_async(tc_interp* interp, const double* theta_pinned,
                                       int n_theta, const double* x_pinned, int64_t n_draws,
                                       int n_gauss_prim, unsigned flags, const double* data,
                                       const double* precision, double* ngal_pinned,
                                       double* chi2_pinned, int64_t* ticket);
int tc_interp_wait(tc_interp* interp, int64_t ticket);
int tc_interp_query(tc_interp* interp, int64_t ticket, int* done);

/* Run-time options of a table handle (the library never reads the environment):
 *   "pipeline"    1 (default): consecutive device-pointer calls rotate over the handle's
 *                 lanes (stream + workspaces) so that kernels of neighbouring batches
 *                 overlap; 0: every call on lane 0, kernels strictly serialised.
 *   "lanes"       number of lanes, 1..8 (default 4; more lose 20 %: four hardware queues).
 *   "ordered"     0 (default): device-pointer calls complete in any order -- wait with
 *                 tc_table_synchronize (or gather with tc_comm_gather, which waits for every
 *                 lane); 1: their finalisations are chained so that results appear in call
 *                 order (0.3 - 3 us per 10^4-draw step).
 *   "fused"       1 (default): calls that qualify (mode auto, at most 20 r values; 104 bins,
 *                 or 212 for the Zheng07 family with n_gauss_prim = 10; total or separated by
 *                 galaxy type) run as ONE launch per batch, a workgroup carrying 64, 40 or 32
 *                 draws from the parameters to the results, where that form is estimated to be
 *                 the faster one.  Pipelined device-pointer and asynchronous calls: batches of
 *                 "fused_min_draws" .. "fused_max_draws" draws (default 0 = chosen per table:
 *                 512 for small tables, ~7000 for 100 bins x 19 r values; 30720; asynchronous
 *                 calls: no upper bound).  Calls that run alone on their lane (host arrays, one
 *                 lane, "pipeline" 0) take it by the same estimate from 2048 draws on, whatever
 *                 "fused_min_draws" says: that option applies to pipelined calls only.  The
 *                 last bits of a result depend on the form that produced it (see
 *                 "deterministic").  0: always occupation, contraction, finalisation kernels;
 *                 2: one launch for every call it can serve, and for tables of 105 .. 248 bins
 *                 (one 16-wave workgroup per CU: level with the three kernels).
 *   "fused_waves" 0 (default): 8 waves per workgroup where two workgroups fit a CU; 8 / 16:
 *                 that many where the table fits.
 *   "fused_draws" 0 (default): workgroups of 32 draws (one tile, eight waves, two per CU) for
 *                 batches below 8192 draws of the Zheng07 family with n_gauss_prim = 10 --
 *                 a third faster there, and the one-launch form then pays from 12 draws per
 *                 bin on -- and for tables of 105 .. 212 bins, of 64 draws otherwise; 32 / 64:
 *                 forced; 40: the latency form ("fused_spread") for every batch it serves.
 *   "fused_spread" 1 (default): calls that have the chip to themselves (host arrays, one lane,
 *                 "pipeline" 0) take the latency form of the one-launch kernel -- workgroups of
 *                 40 draws, one per CU; undecorated Zheng07, n_gauss_prim = 10, total
 *                 correlation function -- for batches of "fused_spread_min" draws (default
 *                 8192) up to "fused_spread_rounds" (default 1, at most 64) workgroups per CU;
 *                 0: never.
 *   "sync_chunks" synchronous host-array calls (tc_predict_zheng07_batch, tc_chi2_zheng07_batch
 *                 beyond the zero-copy size): 0 (default) batches of 2048 draws and more are cut
 *                 into 2 .. 8 chunks of draws (about a megabyte of results each) whose staging,
 *                 kernels, transfers and copies into the caller's arrays overlap; N >= 1: N
 *                 chunks for every batch; -1: the serial path (upload, the kernels alone on one
 *                 lane, download).  "sync_form" (default 32): draws per workgroup of the
 *                 one-launch form the chunks take where it serves the table -- a draw's result
 *                 then does not depend on the number of chunks; 0: whatever a pipelined call of
 *                 the chunk's size takes.  "sync_direct_out": as "async_direct_out" for the
 *                 chunks' staging area (2, default: arrays up to 1 MB are stored by the kernels
 *                 themselves, larger ones travel by copy command).
 *   "sync_stagger"  synchronous host calls on float32 tables with 16 MB of results and more at
 *                 2 KB per draw and more (a (19, 40) table's 10^4 draws are 61 MB): the chunks' kernels run one after the other -- each
 *                 with the chip to itself, the previous chunk's results travelling and being
 *                 copied meanwhile -- and the chunks shrink geometrically to this many per cent
 *                 of the first (default 10, six chunks), so that only a small chunk's transfer
 *                 is left behind the last kernel: 3.1e6 -> 3.6e6 calls/s into arrays the caller
 *                 keeps.  0: equal chunks on all lanes, as for small results.
 *   "autotune"    value = the predict flags to tune for (a combination of TC_FLAG_*; 0 = the
 *                 total prediction of plain Zheng07), n_gauss_prim = 10: MEASURES on this table,
 *                 for batch sizes 256 .. 65536 (x 2 steps), which form serves a batch fastest in
 *                 the pipelined regime -- three kernels, one launch with 64-draw or with 32-draw
 *                 workgroups -- and keeps the choice in the handle (~0.5 s; draws from a wide
 *                 prior box on scratch buffers).  Pipelined device-pointer and asynchronous
 *                 calls with these flags then take the measured form of the nearest batch size
 *                 instead of the built-in estimate (fitted on a handful of table shapes).  -1:
 *                 forget every measurement.  tc_table_autotune_result reads it back.
 *   "autotune_after"  default 0 = never (round 6; it was 256 in round 5).  N > 0: the N-th
 *                 pipelined device-pointer or asynchronous call with one combination of predict
 *                 flags (tables the one-launch forms can serve) runs "autotune" for that
 *                 combination by itself -- that call BLOCKS for about half a second, once, and
 *                 every lane is synchronised -- so that a loop of calls gets the measured form
 *                 without asking; the built-in estimate serves the calls before it.  The
 *                 measured choice depends on wall-clock timings: the last bits of a draw may
 *                 differ before and after that call and from run to run, which is why it is
 *                 opt-in (and refused while "deterministic" is set).
 *   "series"      bit mask; default -1 = by the table: bit 0 for tables whose widest central
 *                 bin is at most 0.1 dex (with wider bins nearly every wavefront of a wide prior
 *                 holds a draw whose sigma_logM is below a bin width and runs the expansion AND
 *                 the node loop), bit 1 off.  Bit 0: the Gauss-Legendre sum of an undecorated
 *                 central bin (tabcorr/tabcorr.py:556-578) by its moment expansion around the
 *                 bin centre -- the same sum re-ordered, one erf and 8 .. 24 short terms instead
 *                 of n_gauss_prim erf evaluations, tabcorr_amd/csrc/series.h -- for every draw
 *                 whose sigma_logM is above about a bin width (truncation below 1e-16;
 *                 otherwise, and for decorated centrals, the node loop); bit 1: the binomial
 *                 expansion of a satellite bin well above the draw's M0.  0: always the node
 *                 loops.  Each draw takes the terms IT needs: with any value of this option a
 *                 draw's result is bit for bit the same wherever it sits in whatever batch
 *                 (round 4 chose the term count per wavefront, which was faster on wide priors
 *                 and made the last bits depend on the neighbouring draws).  Ensembles of
 *                 similar draws (an MCMC's walkers) gain from 3; on a wide prior box a
 *                 wavefront runs the satellites' expansion AND their node loop for most bins.
 *   "grouped"     1 (default): bins with identical log_prim_haloprop_min / max and galaxy type
 *                 -- the secondary-percentile bins of one mass bin (tabcorr/tabcorr.py:186-205)
 *                 -- share their Gauss-Legendre nodes (:548-549); the occupation functions are
 *                 evaluated once per node of such a GROUP and every member bin accumulates
 *                 them with its own weights (Zheng07 family, n_gauss_prim = 10).  No effect on
 *                 tables without such bins.  0: every bin by itself (same occupations per bin
 *                 to the last bit; sums over bins may differ in the last bits).
 *   "fused_defer" 2 (default) / 1: pipelined / asynchronous batches of undecorated Zheng07
 *                 predictions with n_gauss_prim = 10 that take the one-launch form with 64-draw
 *                 workgroups evaluate a satellite bin by its binomial expansion for the draws
 *                 the bin's SHORTEST expansion serves (csrc/series.h; the same number of terms
 *                 for all of them) and every other (bin, draw) pair after the wave's bins, 64
 *                 pairs per pass of the node loop -- tables whose satellite bins all have an
 *                 expansion (bins up to ~0.2 dex wide), unless "series" is 0.  BASELINE
 *                 configs[1] 39.2 -> 37.5 us per 10^4 draws, the reference's example table 18.2 ->
 *                 17.5.  What a draw defers depends on the draw alone: same bits wherever it
 *                 sits in whatever batch.  2: where the centrals take their expansion
 *                 (option "series"), a central bin comes from one record as well and the draws
 *                 no expansion serves (sigma_logM below about a tenth of a bin width, parameters
 *                 to fix up) join the deferred pairs: the node loops of BOTH galaxy types leave
 *                 the loop of bins (configs[1] 37.8 -> 37.2 us).  0: the node loops in place.
 *   "fused_skip"  1 (default): the one-launch form with eight waves x 64 draws and "fused_defer" 2
 *                 places a workgroup's draws in its density array in the order of M0 and
 *                 issues no matrix instruction for a block of four bins whose densities are
 *                 exactly zero for all 16 draws of a group (a Zheng07 satellite bin is, for
 *                 every draw with M0 at or above it) -- only where that keeps the bits: every
 *                 matrix entry finite, every pair-weight sum of the workgroup below 1e280.
 *                 The parts (0, 1) and (2, 3) of the matrix units then share a SIMD, since the
 *                 zero blocks lie in the later parts.  BASELINE configs[1] 35.9 -> 34.4 us per
 *                 10^4 draws.  3: the parts paired as ever; 2: the draws where they are as
 *                 well; 0: every product.  Same bits all four (profiles/skip_notes.md).
 *   "fused_share" 1 (default): with "fused_skip" 1, tables of 9-12 or 17-20 correlation
 *                 function bins (a last r pass of one sub-tile): the waves of a workgroup walk
 *                 their own parts of the matrix units for all r passes but the last and take the
 *                 last passes of the workgroup's eight (tile, part) jobs from a counter in LDS,
 *                 whoever comes first -- the waves whose parts had many zero blocks take more.
 *                 configs[1] 34.2 -> 33.85 us per 10^4 draws.  2: sixteen items of one group of
 *                 16 draws each (2.1 us behind); 0: every wave its own part's.  Same bits all
 *                 three (profiles/share_notes.md).
 *   "cross_wide_min_draws"  default 4096.  Mode cross (tpcf_matrix with one column per halo
 *                 bin), tables or interpolators of up to 16 result rows whose node groups have
 *                 at most two members: undecorated batches of this many draws take the one-launch
 *                 form that multiplies on the matrix pipe and reads a group's expansion
 *                 constants from one record (csrc/series.h, namespace record) -- 49.1 against
 *                 59.1 us per 10^4 draws of the reference's AbacusSummit table --, smaller ones
 *                 the form that keeps the row sums in registers (faster below ~3500 draws);
 *                 the two differ in the last bits.  0: always the register form.
 *   "single_draw" 1 (default): an un-batched predict() goes through one launch.
 *   "resident"    1: un-batched calls (tc_predict_zheng07_batch with one draw; total
 *                 correlation function, Zheng07 family) are served by ONE resident launch:
 *                 the call writes its parameters into a mailbox in page-locked memory, the
 *                 workgroups answer through page-locked partial sums -- no launch per call.
 *                 The kernel leaves when no call has arrived for "resident_idle_us"
 *                 microseconds (default 2000, 10 .. 10^6; the next call launches it again),
 *                 after 10 s, and before any other kind of call on the handle and
 *                 tc_table_destroy.  Device-wide synchronisations by the caller
 *                 (hipDeviceSynchronize, hipFree) wait for it at most that idle time.
 *                 2 (default): the library moves a loop of un-batched calls to the resident
 *                 kernel by itself -- from the eighth call on that follows its predecessor
 *                 within 300 us, with the idle time "resident_auto_idle_us" (default 250: the
 *                 caller's device-wide synchronisations wait at most that long) -- and goes
 *                 back to one launch per call for 4096 calls when more than a quarter of 32
 *                 such calls found the kernel gone (a caller that pauses or synchronises the
 *                 device between its calls).  Single draws only; ensembles need 1.
 *                 Whichever of the two kernels serves a call, the bits are the same (round 6:
 *                 both are instances of one body compiled with -ffp-contract=on), and an error
 *                 of the resident kernel in this mode never reaches the caller: the kernel is
 *                 stopped, the call served by a launch, the mode suspended for 4096 calls
 *                 and switched off after three such failures.
 *                 0: one launch per call, always.
 *                 Calls with 24 .. 256 draws in host arrays (an ensemble sampler's step) are
 *                 served the same way by a second resident kernel of one workgroup per CU
 *                 (kernel_args.h: EnsembleArgs): no launch, no copy command, no stream
 *                 synchronisation per call; a draw's result does not depend on the number of
 *                 draws in the call or its place among them.  When its workgroups do not
 *                 all find a place on the chip (other work running) the launched path serves
 *                 the call -- after three such calls all of them, until the option is set
 *                 again.  The kernel holds every CU's
 *                 LDS while it waits: the ensemble kernel of another handle starts when this
 *                 one has left (its idle time), so alternate between handles with a short
 *                 "resident_idle_us" or keep the option to the one table of the sampler.
 *   "resident_min_walkers"  smallest number of draws per call the resident ensemble kernel
 *                 takes (default 24, 2 .. 256): for fewer, one launch of the un-batched kernel
 *                 is faster.
 *   "resident_wait_us"  how long a workgroup of the resident ensemble kernel waits for another
 *                 one inside a call before it gives up (default 20 000, 1 .. 10^6).
 *   "resident_aperture"  1 (default): on large-BAR systems the mailbox of the resident
 *                 ensemble kernel lies in device memory that the host stores into through
 *                 the PCIe aperture (no PCIe reads while the kernel polls); 0: in page-locked
 *                 host memory, as on systems without a large BAR.
 *   "deterministic"  which of a call's possible kernel forms runs, and hence the LAST BITS of its
 *                 results (the reference itself, tabcorr/tabcorr.py:580-683, is deterministic).
 *                 Every form's mean occupations agree PER BIN with the reference's formula in
 *                 extended precision to 1.2e-15 absolute (centrals) and 7.7e-15 relative
 *                 (satellites) -- largest over the strata of tests/test_gpu_occupation_forms.py on
 *                 an MI355X: occ_zheng07_kernel 1.2e-15 / 7.6e-15, the one-launch forms 8 x 64
 *                 8.9e-16 / 6.3e-15, 16 x 64 4.5e-16 / 5.4e-15, 8 x 32 4.1e-16 / 5.0e-15, 8 x 40
 *                 4.5e-16 / 5.9e-15, mode cross 8.3e-16 / 7.6e-15 (register form 4.7e-16 /
 *                 6.5e-15), un-batched 3.5e-16 / 3.3e-15 -- for |sigma_logM| >= 0.03 and
 *                 satellite bins whose condition number with respect to M0 is at most 24: the
 *                 rounding of 10^logM0 (6e-16) reaches a bin multiplied by that number.
 *                 0 (default): the fastest form for the call -- a function of the table, the
 *                 flags, the entry point (un-batched, host arrays, device pointers,
 *                 asynchronous) and the batch size.  Never of timing or of the number of calls
 *                 made so far (round 6: "autotune_after" is off by default and the two
 *                 un-batched kernels give the same bits), so the same sequence of calls
 *                 returns the same bits in every run; the same DRAW in batches of different
 *                 sizes, or through different entry points, may differ in the last bits.
 *                 The gradient entry points (tc_predict_grad_* / tc_chi2_grad_*) have ONE form
 *                 each and are batch-invariant by construction at every value of this option:
 *                 a draw's results depend on the draw alone, host arrays or device pointers.
 *                 1: the same, and "autotune" / "autotune_after" are refused (nothing
 *                 measured can enter the choice).
 *                 2: batch-invariant -- ONE form per (table, flags): the one-launch kernel
 *                 (predict_fused_kernel with 64-draw workgroups, or the mode-cross one-launch
 *                 kernel with one workgroup per 64 draws) for every entry point and every
 *                 batch size, one draw included, so that a draw's (ngal, xi) depends on the
 *                 draw alone: wherever it sits in whatever batch, synchronous or asynchronous,
 *                 first call or millionth.  Where no one-launch form serves the table and the
 *                 flags (tc_table_batch_invariant says: float32 tables, several r tiles, more
 *                 than 248 bins, interpolators in mode auto, fused likelihood of separated
 *                 components) the call runs as with 1.  What it costs: un-batched calls
 *                 ~70 us instead of ~10-18 (a whole workgroup's latency for one draw); batches
 *                 below ~8000 draws up to 2x (64-draw workgroups do not fill the chip);
 *                 batches of 10^4 draws and more nothing (it is the default form there).
 *                 Setting the option waits for the handle's work in flight.
 *   "trace"       developer timelines (developer builds only, tabcorr_amd_testing.h). */
int tc_table_set_option(tc_table* table, const char* name, int value);
/* The handle's resident kernels so far: launches (of either kernel), calls that found the
 * single-draw kernel gone and launched it again, calls the automatic mode handed back to a
 * launch after an error (it switches itself off at three), and whether one is running now
 * (0 no, 1 the single-draw kernel, 2 the ensemble kernel).  Any pointer may be NULL. */
int tc_table_resident_stats(const tc_table* table, int64_t* launches, int64_t* relaunches,
                            int64_t* failures, int* running);
/* *out = 1 when option "deterministic" = 2 is set AND a one-launch form serves this table with
 * these predict flags and n_gauss_prim: every batched, un-batched and asynchronous call with
 * them then runs that one form (a draw's bits depend on the draw alone); else 0. */
int tc_table_batch_invariant(tc_table* table, int n_gauss, unsigned flags, int* out);
/* What option "autotune" measured for `flags`: per batch size (`count` of them, at most
 * `capacity`: 9) the form chosen (0 three kernels, 64 / 32: draws per workgroup of the
 * one-launch form) and the microseconds per call of the three forms in that order, us
 * (count, 3) (0: form not available). */
int tc_table_autotune_result(const tc_table* table, unsigned flags, int capacity, int* count,
                             int64_t* sizes, int* forms, float* us);

/* ---- measurement -------------------------------------------------------------------
 * HIP events on the handle's own stream (torch.cuda.Event would only see torch's).
 * tc_table_timer_begin/end bracket a region; with profile = 1 every launch of the
 * contraction kernel -- of this table, or of an interpolator whose first table this is --
 * additionally carries its own start / stop events (hipExtLaunchKernelGGL: the dispatch's
 * own begin and end, the interval rocprofv3 --kernel-trace reports) and
 * tc_table_kernel_time reports the count and mean duration since timer_begin.  profile = n
 * > 1: every n-th launch only, from the first on (a pair of events costs a launch ~1.5 us on
 * its queue; with n = the number of lanes the sampled launches are those of one lane). */
int tc_table_timer_begin(tc_table* table, int profile_kernels);
int tc_table_timer_end(tc_table* table, float* elapsed_ms);
int tc_table_kernel_time(tc_table* table, int* n_launches, float* mean_ms);
/* Launch geometry of the last predict call (for DESIGN.md / bench.py reporting). */
int tc_table_last_launch(const tc_table* table, int* n_workgroups, int* waves_per_workgroup,
                         int* n_splits, int* lds_bytes);

/* ---- tabulation: pair counting ---------------------------------
 *
 * tc_pair_count_rppi replaces one Corrfunc.theory.DDrppi call of tabcorr/corrfunc.py:62-84
 * (the pair count behind `wp` for one pair of halo bins): ORDERED pair counts between the
 * points pos1 (n1, 3) and pos2 (n2, 3) -- pos2 = NULL: of pos1 with itself, every pair then
 * counted twice as Corrfunc's autocorr = 1 does -- in a periodic box `boxsize` (3), per
 * projected-separation bin (rp_bins: n_rp + 1 increasing edges) and line-of-sight bin
 * (n_pi equal bins on [0, pi_max)): npairs (n_rp, n_pi), row-major.  Separations are
 * minimum-image; r_p^2 = dx dx + dy dy is compared with rp_bins^2; a pair with i == j only
 * counts when rp_bins[0] == 0.  Integer counters: the result is exact and independent of
 * the execution order.
 *
 * tc_pair_count_rppi_labelled is the loop of tabcorr/tabcorr.py:846-922
 * (compute_tpcf_matrix: one pair count per pair of halo bins, from a process pool) in ONE
 * pass: label1 / label2 give the halo bin of every point (0 <= label < n_labels) and
 * counts (n_rp, n_labels, n_labels) receives, for every pair of bins (a, b), the ordered
 * pair counts between the points of bin a in set 1 and of bin b in set 2 (pos2 = NULL:
 * set 1 with itself), summed over |pi| < pi_max.  Positions must lie in [0, boxsize]. */
int tc_pair_count_rppi(const double* pos1, int64_t n1, const double* pos2, int64_t n2,
                       const double* boxsize, const double* rp_bins, int n_rp, double pi_max,
                       int n_pi, uint64_t* npairs);
/* tc_pair_count_smu replaces one Corrfunc.theory.DDsmu call of tabcorr/corrfunc.py:141-163
 * (the pair count behind `s_mu_tpcf`): ordered pair counts per bin of the three-dimensional
 * separation s (s_bins: n_s + 1 increasing edges, compared squared) and of mu = |dz| / s
 * (n_mu equal bins on [0, 1); a pair with mu == 1 is not counted): npairs (n_s, n_mu). */
int tc_pair_count_smu(const double* pos1, int64_t n1, const double* pos2, int64_t n2,
                      const double* boxsize, const double* s_bins, int n_s, int n_mu,
                      uint64_t* npairs);
int tc_pair_count_rppi_labelled(const double* pos1, const int32_t* label1, int64_t n1,
                                const double* pos2, const int32_t* label2, int64_t n2,
                                int n_labels, const double* boxsize, const double* rp_bins,
                                int n_rp, double pi_max, uint64_t* counts);
/* The same one-pass form for `s_mu_tpcf` tables (tabcorr/tabcorr.py:846-922 with
 * tpcf = tabcorr/corrfunc.py:98-175): counts (n_s, n_mu, n_labels, n_labels); n_s n_mu <=
 * 15360 (the counters of one pair of labels in a workgroup's LDS). */
int tc_pair_count_smu_labelled(const double* pos1, const int32_t* label1, int64_t n1,
                               const double* pos2, const int32_t* label2, int64_t n2,
                               int n_labels, const double* boxsize, const double* s_bins,
                               int n_s, int n_mu, uint64_t* counts);

/* tc_mass_in_cylinders is the pair count behind an excess-surface-density table: what
 * TabCorr.tabulate does per halo bin when it is handed halotools' mean_delta_sigma with
 * tpcf_args = (particle positions, particle masses, rp_bins) (tabcorr/tabcorr.py:846-922 in
 * mode 'cross'; scripts/tabulate_snapshot.py:228-237), for the objects of ALL bins in one
 * pass: mass (n_objects, n_edges) receives, per object and per radius rp_bins[k], the summed
 * mass of the particles whose projected separation r = sqrt(dx^2 + dy^2) (periodic in x and y,
 * the line of sight spanning the box) is <= rp_bins[k].  masses = NULL: unit masses (counts).
 * Sums run in a fixed order (reproducible; exact for equal masses). */
int tc_mass_in_cylinders(const double* objects, int64_t n_objects, const double* particles,
                         int64_t n_particles, const double* masses, const double* boxsize,
                         const double* rp_bins, int n_edges, double* mass);

/* ---- multi-GPU: one process per GPU, results collected with one RCCL gather ---------- */

#define TC_UNIQUE_ID_BYTES 128
int tc_comm_unique_id(void* id /* TC_UNIQUE_ID_BYTES */);
int tc_comm_create(const void* id, int n_ranks, int rank, tc_comm** comm);
int tc_comm_destroy(tc_comm* comm);
/* Gather `count` doubles from every rank's send_device into recv_device on `root`
 * (rank-major), on the communicator's own stream, after the work queued so far on
 * `table`'s stream (NULL: no dependency).  `slot` in [0, 4) names the send buffer:
 * tc_comm_release(comm, table, slot) later makes `table`'s stream wait on the device
 * for that gather, so that the buffer can be overwritten -- this is what lets the gather
 * of batch k overlap with the prediction of batch k + 1. */
int tc_comm_gather(tc_comm* comm, tc_table* table, const double* send_device,
                   double* recv_device, int64_t count, int root, int slot);
int tc_comm_release(tc_comm* comm, tc_table* table, int slot);
/* The same for results produced by an interpolator handle (Interpolator.predict sharded
 * over the GPUs: BASELINE configs[3], interpolator.py:124-216). */
int tc_comm_gather_interp(tc_comm* comm, tc_interp* interp, const double* send_device,
                          double* recv_device, int64_t count, int root, int slot);
int tc_comm_release_interp(tc_comm* comm, tc_interp* interp, int slot);
int tc_comm_barrier(tc_comm* comm);
int tc_comm_synchronize(tc_comm* comm);

#ifdef __cplusplus
}
#endif

#endif /* TABCORR_AMD_H */
