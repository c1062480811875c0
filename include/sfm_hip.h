/* sfm_hip.h — C ABI of libsfm_hip.so: MI355X (gfx950) kernels for the RANSAC essential-matrix,
 * cheirality and triangulation hot path of Bazs/structure_from_motion.
 *
 * The reference has no FFI for this path (it is pure Python); each entry point below replaces the
 * Python inner loop cited next to it (paths relative to the reference repo).  A maintainer binds them
 * with ctypes as shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer marked "dev" is device memory (hipMalloc / a torch ROCm tensor's data_ptr());
 *     "host" pointers are ordinary process memory.  All arrays are dense, row-major, float64 unless
 *     another element type is given.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls only enqueue work;
 *     nothing synchronises with the host.
 *   - a leading `batch` dimension runs independent image pairs (blockIdx.y); batch == 1 for one pair.
 *   - size limits of ONE call: a kernel that gives every work item a thread or wave of its own is launched
 *     with at most 2^31-1 blocks and 2^32-1 threads along x, and `batch` (grid y) at most 65535; a call
 *     beyond that returns SFM_EINVAL before anything is launched (never a silently partial result).  In
 *     hypothesis counts per call: sfm_sample_philox* 2^32-256, sfm_fit_eight_point* / sfm_sample_fit_philox
 *     2^32-64, sfm_score_sed 2^28 (16 hypotheses per 256-thread block), sfm_cheirality / sfm_triangulate
 *     2^32-64 points.  Element-wise kernels (normalise, mask, SED values, select) walk their items with
 *     grid-stride loops and have no such limit.
 *   - return value: 0 on success, a negative SFM_E* code otherwise; sfm_last_error() returns a
 *     thread-local message for the last failure.
 */
#ifndef SFM_HIP_H
#define SFM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_OK 0
#define SFM_EINVAL (-1) /* bad argument (null pointer, negative size, n < 8, ...) */
#define SFM_EHIP (-2)   /* a HIP runtime call failed (message has the hipError string) */

/* error aggregation of reference lib/ransac/ransac.py:12-16 */
#define SFM_AGG_SUM 0
#define SFM_AGG_SQUARE 1
#define SFM_AGG_MEAN 2
#define SFM_AGG_RMS 3

/* per-hypothesis fit flags written by sfm_fit_eight_point */
#define SFM_FIT_DEGENERATE 1 /* eight_point.py:415-421 predicate: second-smallest eigenvalue <= 1e-10 */

/* Result record of sfm_select_best (one per batch entry, device memory, 40 bytes). */
typedef struct sfm_select_result {
    uint64_t key;          /* IEEE bits of best_err (monotone for err >= 0); INT64_MAX (0x7FFF...F) if no model */
    int64_t best_h;        /* global hypothesis index (h_offset + local), -1 if no model */
    double best_err;       /* aggregated inlier error of the winner (ransac.py:80-82), +inf if none */
    int64_t first_flagged; /* lowest global index with a fit flag set, INT64_MAX if none */
    int32_t n_flagged;     /* number of flagged hypotheses */
    int32_t best_cnt;      /* extra-inlier count of the winner */
} sfm_select_result;

/* Version of this interface: libsfm_hip.so reports the one it was compiled from (sfm_abi_version), the Python binding
 * and the torch op library (sfm_torch_ops_abi_version) refuse a library of another version. */
#define SFM_ABI_VERSION 15

const char* sfm_last_error(void);
int sfm_abi_version(void);

/* K-normalise matched pixel coordinates (eight_point.py:127-133, hoisted out of the H x N loop):
 * corr[i] = [(xa-cx)/fx, (ya-cy)/fy, (xb-cx)/fx, (yb-cy)/fy].
 * pix_a, pix_b: dev [count,2]; corr: dev [count,4]. */
int sfm_normalize_correspondences(const double* pix_a, const double* pix_b, int64_t count, double fx,
                                  double fy, double cx, double cy, double* corr, void* stream);

/* Counter-based hypothesis sampler (replaces the sequential random.shuffle of ransac.py:62-63 for
 * large H): S[b,h,:] = 8 distinct indices in [0,n) from Philox(seed + b*seed_stride, h_begin + h).
 * S: dev int32 [batch,h_count,8]. */
int sfm_sample_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, int64_t h_count, int64_t n,
                      int64_t batch, int32_t* S, void* stream);

/* Same sampler with the 64-bit seed read from device memory (seed_dev[0]) at kernel run time: a captured
 * hipGraph of sample -> fit -> score -> select can be replayed with a new seed by rewriting that word. */
int sfm_sample_philox_dev(const uint64_t* seed_dev, uint64_t seed_stride, int64_t h_begin, int64_t h_count,
                          int64_t n, int64_t batch, int32_t* S, void* stream);

/* Same sampler for ONE hypothesis per batch entry whose index is read from device memory:
 * S[b,:] = sample of hypothesis h_index[b] (0..7 if h_index[b] < 0).  Lets the multi-GPU winner be
 * re-derived on every rank without a host round trip.  h_index: dev int64 [batch]; S: dev int32 [batch,8]. */
int sfm_sample_philox_at(uint64_t seed, uint64_t seed_stride, const int64_t* h_index, int64_t n,
                         int64_t batch, int32_t* S, void* stream);

/* Normalised eight-point fit of every hypothesis (epipolar_ransac.py:28-42 -> eight_point.py:136-170).
 * corr: dev [batch,n,4]; S: dev int32 [batch,h_count,8]; E: dev [batch,h_count,9] (row-major 3x3,
 * E[8] == 1); flags: dev int32 [batch,h_count]; lambda2: optional dev [batch,h_count] receiving the
 * second-smallest eigenvalue of Y^T Y (NULL to skip). */
int sfm_fit_eight_point(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch,
                        double* E, int32_t* flags, double* lambda2, void* stream);

/* sfm_sample_philox (or, with seed_dev != NULL, sfm_sample_philox_dev) and sfm_fit_eight_point in ONE launch: the fit
 * kernel draws each hypothesis' sample itself and also stores it in S.  Same S, E, flags as the two calls. */
int sfm_sample_fit_philox(uint64_t seed, const uint64_t* seed_dev, uint64_t seed_stride, int64_t h_begin,
                          const double* corr, int64_t n, int64_t h_count, int64_t batch, int32_t* S, double* E,
                          int32_t* flags, void* stream);

/* The same fit with its intermediates written out, for parity checks of the fused stages against the
 * reference's private helpers (_normalize_coords :308-338, _get_yT_y :363-375, _compute_f_est :396-427,
 * _enforce_fundamental_mat_constraints :430-446).  trace: dev [batch,h_count,sfm_fit_trace_doubles()] doubles:
 * normalised coords a [8][2] | b [8][2] | T1 {scale,cx,cy} | T2 {scale,cx,cy} | Y^T Y [9][9] |
 * eigenvalues [9] | f_est [9] | rank-2 F [9]. */
int sfm_fit_trace_doubles(void);
int sfm_fit_eight_point_traced(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch,
                               double* E, int32_t* flags, double* trace, void* stream);

/* Single-problem stages of the fit (device pointers):
 *   stage 0  Y^T Y of 8 coordinate pairs as given   in [8][4] {xa,ya,xb,yb}  out [81]
 *   stage 1  _compute_f_est                          in [81]                  out f_est[9] | eigenvalues[9] | flag
 *   stage 2  _enforce_fundamental_mat_constraints    in [9]                   out [9] */
int sfm_fit_stage(int stage, const double* in, double* out, void* stream);

/* _normalize_coords (eight_point.py:308-338) for n points.  coords: dev [n,2]; out: dev [2n+3] =
 * normalised coords [n][2] then {scale, centroid x, centroid y} of the forward transform. */
int sfm_hartley_normalize(const double* coords, int64_t n, double* out, void* stream);

/* Symmetric-epipolar-distance scoring of all n correspondences under all hypotheses
 * (ransac.py:66-82 with epipolar_ransac.py:18-25 / sed.py:7-30 as the scorer).
 * cnt[b,h] = #non-sample points with sed <= thr; s1 / s2 = sum of sed / sed^2 over the 8 sample points
 * plus those survivors.  cnt: dev int32 [batch,h_count]; s1, s2: dev [batch,h_count].
 * workspace: dev scratch of at least sfm_score_workspace_bytes(n, h_count, batch) bytes, 16-byte aligned; it
 * enables the two-tier kernels (a conservative reject filter + exact fp64 evaluation of the survivors, hypotheses
 * processed longest-first; identical counts and inlier decisions — the exact tier decides with sed.py's own operation sequence
 * wherever a cheaper form of the same fp64 value is not clear of the threshold by 1e-13 — sums in a fixed order, each summand
 * within 1.2e-15 of the all-fp64 kernel's): the fp32 VALU filter, and for a
 * single pair of at least 4000 points, 2048 hypotheses and 3.5e8 evaluations (at most 4 194 304 points) the kernel with the
 * filter on the fp16 / bf16 matrix pipe and a lane-per-hypothesis exact tier (sfm_score_options.kernel forces it on / off).
 * Large single-pair launches are cut into ranges of the points whose partial results are added in range order.  NULL selects
 * the all-fp64 kernel.
 * Footprint (ABI 11: sized by what the call will launch; until then every region was reserved whether or not a launch could
 * pick it): always 16 bytes per point (fp32 points of the VALU filter; the matrix-pipe kernel keeps its partial maxima there),
 * 16 KiB of counters per pair and 4 bytes per hypothesis (scoring order); for one pair 4 more per hypothesis (state of a fused
 * pass's selection); where the launch is cut into k ranges of the points 20 k bytes per hypothesis (their partials); where the
 * matrix-pipe kernel runs its tables — 96 bytes per point, 96 + 20 bytes per hypothesis — and, for a single pair whose cost
 * pre-pass hands its filter results to the scoring launch, 512 bytes per hypothesis.  50 000 x 100 000 (matrix-pipe kernel, 8
 * ranges): 86 MB; 256 pairs x 10 000 x 2 000: 444 MB with the matrix-pipe kernel (9 ranges), 47 MB with the VALU filter
 * (521 MB either way until ABI 10).
 * sfm_score_workspace_bytes_ex sizes for a call made with `options` (NULL = the process-wide defaults, what the plain form
 * uses): options that pick another kernel or more ranges than the workspace was sized for make the call return SFM_EINVAL —
 * never a silent overrun.  -1: negative size or bad options. */
int64_t sfm_score_workspace_bytes(int64_t n, int64_t h_count, int64_t batch);   /* (_ex: below, behind sfm_score_options) */
int sfm_score_sed(const double* corr, int64_t n, const double* E, const int32_t* S, int64_t h_count,
                  int64_t batch, double thr, int32_t* cnt, double* s1, double* s2, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* Launch options of the two-tier scoring kernels.  They change HOW a call is launched, never what it returns: counts and
 * decisions are identical under every setting, the sums differ in their last bits between kernels / numbers of ranges
 * (summation order; the two-tier kernels' summands within 1.2e-15 of the all-fp64 kernel's) and are bit-identical from run to
 * run under one setting.  The library does not read the process
 * environment: a call carries its options (sfm_score_sed_ex; NULL = the process-wide defaults) and the embedding application
 * sets the defaults once (sfm_score_set_default_options; the Python package translates SFM_SCORE_MATRIX / _HPW / _SPLIT /
 * _ORDER / _ONE_SIDED / _XCD / _SYNC / _PERSISTENT there when it is imported).  Safe to call from several threads: a default set is
 * replaced as a whole. */
#define SFM_SCORE_KERNEL_AUTO 0     /* the size rule described at sfm_score_sed */
#define SFM_SCORE_KERNEL_FILTERED 1 /* fp32 VALU filter */
#define SFM_SCORE_KERNEL_MATRIX 2   /* fp16 / bf16 matrix-pipe filter, where it applies (<= 4 194 304 points per pair), else FILTERED */
typedef struct sfm_score_options {
    int32_t kernel;        /* SFM_SCORE_KERNEL_AUTO / _FILTERED / _MATRIX */
    int32_t hyps_per_wave; /* VALU-filter kernel: 0 = by launch size, or 1 / 2 / 4 */
    int32_t split;         /* ranges of the points of a single pair: -1 = by launch size, 0 = none, k = k ranges (at most 16) */
    int32_t order;         /* heaviest-first processing order: -1 = by launch size, 0 = index order, 1 = on */
    int32_t one_sided;     /* VALU filter: -1 / 1 = one-sided test r^2 / dB (default), 0 = two-sided (ablation) */
    int32_t xcd_map;       /* batches: -1 / 1 = all blocks of a pair on one XCD (default), 0 = plain (block, pair) grid */
    int32_t block_sync;    /* sfm_ransac_pass_small: -1 = by size, k = block barrier every k loop iterations, 0 = never */
    int32_t persistent;    /* matrix-pipe kernel, single pair: 1 = persistent waves taking (hypothesis group, range) items from
                              per-XCD counters; -1 / 0 = one block per four items, placed by the hardware dispatcher (default:
                              measured equal at 5e9 evaluations and faster below — the 4096 first tickets cost ~45 us) */
    /* Measurement hook of THIS call (ABI 11; until then process-global state behind sfm_score_set_timing_events): hipEvent_t
     * handles (either may be NULL) recorded on the launch stream immediately before / after the scoring kernel itself — not the
     * workspace preparation or the ordering pre-pass — so that a benchmark times exactly the kernel a profiler reports.  Never
     * part of the process-wide defaults (sfm_score_set_default_options clears them). */
    void* timing_before;
    void* timing_after;
} sfm_score_options;
#define SFM_SCORE_OPTIONS_DEFAULT {SFM_SCORE_KERNEL_AUTO, 0, -1, -1, -1, -1, -1, -1, 0, 0}
int sfm_score_sed_ex(const double* corr, int64_t n, const double* E, const int32_t* S, int64_t h_count,
                     int64_t batch, double thr, int32_t* cnt, double* s1, double* s2, void* workspace,
                     int64_t workspace_bytes, void* stream, const sfm_score_options* options);
int64_t sfm_score_workspace_bytes_ex(int64_t n, int64_t h_count, int64_t batch, const sfm_score_options* options);
/* Process-wide defaults for calls without options (sfm_score_sed, sfm_ransac_pass_small / _large and sfm_score_sed_ex with
 * options == NULL); NULL restores SFM_SCORE_OPTIONS_DEFAULT.  _get copies the current set out. */
int sfm_score_set_default_options(const sfm_score_options* options);
int sfm_score_get_default_options(sfm_score_options* out);
/* Which kernel a call would launch for these sizes with a workspace: SFM_SCORE_KERNEL_FILTERED or SFM_SCORE_KERNEL_MATRIX;
 * negative sizes or bad options: -1.  (For reports and tests: the results do not depend on it.)  The plain form uses the
 * process-wide defaults. */
int sfm_score_kernel_choice(int64_t n, int64_t h_count, int64_t batch);
int sfm_score_kernel_choice_ex(int64_t n, int64_t h_count, int64_t batch, const sfm_score_options* options);

/* One whole RANSAC pass of a SMALL problem (one image pair, 8 <= n <= 8192, h_count <= 32768) in THREE lean launches
 * instead of the five of sfm_sample_fit_philox / sfm_fit_eight_point -> sfm_score_sed -> sfm_select_best -> sfm_inlier_mask, and the same
 * outputs (S, E, flags, cnt, s1, s2, result, mask) bit for bit:
 *   launch 1  the eight-point fits — use_philox != 0: samples drawn in the kernel from (seed or *seed_dev, h_begin + h)
 *             and stored in S; use_philox == 0: the caller's table in S — and, in spare blocks of the same launch, the
 *             preparation of the scoring workspace (no launch of its own);
 *   launch 2  SED scoring;
 *   launch 3  the selection of ransac.py:75-86 spread over up to 32 blocks, folded by the block that arrives last
 *             (a single block walking all hypotheses is latency-bound: 14 us at 10 000 hypotheses); when a mask is
 *             wanted the same launch carries ceil(n / 256) more blocks that wait for the published record and write
 *             the winner's inlier mask.
 * A small pass is a chain of dependent, latency-bound launches: what shortens it is fewer and leaner ones.
 * h_offset as in sfm_select_best (the record carries global indices = local + h_offset); the mask is always the
 * winner's, whatever h_offset: the kernels index E and S with the local winner.
 * workspace: sfm_score_workspace_bytes_ex(n, h_count, 1, options) bytes, 16-byte aligned.  options: launch options of the
 * scoring launch (NULL = the process-wide defaults). */
int sfm_ransac_pass_small(uint64_t seed, const uint64_t* seed_dev, int use_philox, int64_t h_begin, const double* corr,
                          int64_t n, int64_t h_count, double thr, double min_extra, int aggregation, int64_t h_offset,
                          int32_t* S, double* E, int32_t* flags, int32_t* cnt, double* s1, double* s2,
                          sfm_select_result* result, uint8_t* mask, void* workspace, int64_t workspace_bytes,
                          void* stream, const sfm_score_options* options);

/* Diagnostic of the matrix-pipe reject filter (tests measure the margin of its error bound with it; not on the product
 * path): prepares the operand tables of one pair exactly as sfm_score_sed does and evaluates tier 1 — the three 16-bit
 * matrix instructions — for EVERY (hypothesis, point), writing the raw fp32 accumulators instead of deciding on them.
 * n <= 4 194 304.  workspace: sfm_score_workspace_bytes_ex(n, h_count, 1, {kernel = SFM_SCORE_KERNEL_MATRIX, split = 0}) bytes.
 * With n_pad = 32 * ceil(n / 32):
 *   r_out  dev float [h_count, n_pad]   r'' = the scaled bilinear form c b^T E a s_p s_h as the matrix unit accumulated it
 *   d_out  dev float [h_count, n_pad]   the accumulated upper bound of (dA + dB) / 4 s_p^2 s_h^2 + slack (a point is rejected
 *                                       iff fma(-r'', r'', d) is negative); columns >= n are padding rows of zeros + slack
 *   bound_out dev float [h_count, 8]    {delta'' (bound on |r''_mfma - r''|), slack'' = delta''^2 (1 + k) / k, s_h, armed (1 / 0),
 *                                       s_p, the bf16-rounding term of the denominator chain in units of s_h^2, the constant
 *                                       slot as stored, 0} */
int sfm_debug_matrix_filter(const double* corr, int64_t n, const double* E, int64_t h_count, double thr, void* workspace,
                            int64_t workspace_bytes, float* r_out, float* d_out, float* bound_out, void* stream);

/* The same for a LARGE problem (one image pair, any n and h_count the separate calls take): sfm_sample_fit_philox /
 * sfm_fit_eight_point -> sfm_score_sed -> sfm_select_best -> sfm_inlier_mask in SEVEN launches instead of eighteen where the
 * matrix-pipe scoring kernel applies, with the same outputs (S, E, flags, cnt, result, mask bit for bit; s1 / s2 bit for
 * bit too: the ranges of the scoring launch are added in the same order):
 *   1  partial maxima of the points + every zeroing the pass needs;  2  the eight-point fits — every lane also writes its
 *   hypothesis' rows of the scoring kernel's operand table and its sample correction (E and the sample are in registers there),
 *   blocks behind the fit blocks write the point operand table;  3  cost pre-pass;  4  class histogram;  5  scan + scatter (the
 *   heaviest-first order);  6  the scoring kernel;  7  fold of the point ranges + selection (ransac.py:75-86) over up to 256
 *   blocks + the blocks that write the winner's inlier mask.
 * Sizes for which sfm_score_sed picks another kernel run the fit, that call's launches and launch 7.  Arguments as for
 * sfm_ransac_pass_small. */
int sfm_ransac_pass_large(uint64_t seed, const uint64_t* seed_dev, int use_philox, int64_t h_begin, const double* corr,
                          int64_t n, int64_t h_count, double thr, double min_extra, int aggregation, int64_t h_offset,
                          int32_t* S, double* E, int32_t* flags, int32_t* cnt, double* s1, double* s2,
                          sfm_select_result* result, uint8_t* mask, void* workspace, int64_t workspace_bytes,
                          void* stream, const sfm_score_options* options);

/* The same for a BATCH of independent image pairs (BASELINE configs[4]: 256 pairs x 10 000 x 2 000; every array with a leading
 * pair dimension as in the separate calls, pair b sampling from Philox(seed + b * seed_stride, h_begin + h)): where the batch takes
 * the matrix-pipe scoring kernel (sfm_score_kernel_choice(n, h_count, batch)) —
 *   1  partial maxima of every pair's points + every zeroing;  2  the pairs' point operand tables;  3  the eight-point fits,
 *   whose lanes also write their hypothesis' operand rows and sample correction;  4  cost pre-pass;  5  class histogram;
 *   6  scan + scatter;  7  the scoring kernel;  8  per pair one block: fold of the point ranges + selection + inlier mask
 * — instead of the fifteen launches of sfm_sample_fit_philox -> sfm_score_sed -> sfm_select_best -> sfm_inlier_mask, with the same
 * outputs bit for bit.  Other sizes: the fit, that scoring call's own launches, and launch 8.  result: dev [batch]; mask: dev
 * uint8 [batch, n] or NULL. */
int sfm_ransac_pass_batch(uint64_t seed, const uint64_t* seed_dev, uint64_t seed_stride, int use_philox, int64_t h_begin,
                          const double* corr, int64_t n, int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation,
                          int32_t* S, double* E, int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result,
                          uint8_t* mask, void* workspace, int64_t workspace_bytes, void* stream, const sfm_score_options* options);

/* Model selection (ransac.py:75-86): lowest aggregated error among hypotheses with
 * cnt >= min_extra, strict <, earliest index wins, NaN/inf never win.  sample_size: the items of a sample that enter
 * the mean and RMS aggregates (count + sample_size): 8 (eight-point), 6 (five-point, PnP DLT), 4 (P3P, homography) or 3
 * (similarity); SFM_EINVAL
 * otherwise.  result: dev [batch]. */
int sfm_select_best(const int32_t* cnt, const double* s1, const double* s2, const int32_t* flags, int64_t h_count, int64_t batch,
                    double min_extra, int aggregation, int64_t h_offset, int sample_size, sfm_select_result* result, void* stream);

/* Cross-shard selection for hypothesis-sharded RANSAC (one rank per GPU).  Each rank runs
 * sfm_select_best over its own block of hypotheses with h_offset = the block's first global index, the ranks
 * all-gather their [batch] records (40 bytes each) into gathered[world][batch], and this folds them: lowest error
 * key, then lowest global index (the sequential "strictly lower error replaces the incumbent" rule of
 * ransac.py:83-86 for any partition); first_flagged = minimum, n_flagged = sum (saturating), so every rank takes
 * the same decision about degenerate samples (eight_point.py:415-421 raised through ransac.py:65).
 * Outputs (each optional, dev): global [batch] = the folded records; best_h [batch] = the winners' global indices
 * (-1 if none; the form sfm_sample_philox_at reads); single [batch] = the folded records with best_h replaced by
 * 0 / -1, i.e. addressed at a one-hypothesis E / S array holding the locally re-derived winner (for sfm_inlier_mask).
 * The _host variant takes host pointers and runs on the calling thread (the fold is 40 bytes per rank: it exists so
 * that the N > 1 selection logic is testable over a CPU process group). */
int sfm_fold_select_records(const sfm_select_result* gathered, int64_t world, int64_t batch,
                            sfm_select_result* global, int64_t* best_h, sfm_select_result* single, void* stream);
int sfm_fold_select_records_host(const sfm_select_result* gathered, int64_t world, int64_t batch,
                                 sfm_select_result* global, int64_t* best_h, sfm_select_result* single);

/* Inlier mask of the selected model: mask[b,i] = 1 if point i is a non-sample survivor, 2 if it is one of
 * the sample_size sample points (the first sample_size entries of its row of S: 8 or 6; SFM_EINVAL otherwise), 0 otherwise.
 * `result` as written by sfm_select_best with h_offset 0 (or with best_h rewritten to a local index); entries with
 * best_h < 0 leave their mask zeroed.  mask: dev uint8 [batch,n]. */
int sfm_inlier_mask(const double* corr, int64_t n, const double* E, const int32_t* S, int64_t h_count, int64_t batch,
                    const sfm_select_result* result, double thr, int sample_size, uint8_t* mask, void* stream);

/* ---- RANSAC absolute pose (PnP) of a further view against triangulated points (csrc/sfm_pnp.hip) ----
 * The reference's fit_with_ransac (ransac.py:55-86) with a six-item sample, a six-point DLT fitter and the squared
 * reprojection error in pixels as the scorer.  pts: dev [batch,n,5] = {X, Y, Z, u, v}: a 3-D point in the frame of camera 1
 * and the pixel of its match in the new view.  K: host [9], the camera matrix row-major; row 2 must be (0, 0, 1)
 * and K00 K11 - K01 K10 neither zero nor NaN (SFM_EINVAL otherwise, here and in every entry point below that takes K); all
 * six entries of rows 0 and 1 count in every kernel, the DLT's normalisation included, so K may carry skew.  S: dev int32 [batch,h_count,8], the sample tables of sfm_sample_philox / sfm_pyshuffle_table:
 * the first 6 entries of each row are the sample (an entry outside [0, n) flags the hypothesis).  model: dev
 * [batch,h_count,12] = R row-major (9) | t (3), x_cam = R X + t.  flags: dev int32 [batch,h_count], SFM_FIT_DEGENERATE when
 * sigma_11 / sigma_1 of the conditioned 12 x 12 DLT matrix is below 1e-9 (coplanar or collinear points) or not a number.
 * n >= 6 in every call. */

/* Six-point DLT fit of every hypothesis: K-normalised 2-D side, 3-D side conditioned per sample (centroid, mean distance
 * sqrt(3)), null vector by a 12 x 12 one-sided Jacobi SVD, conditioning undone, R = U V^T of M = [P]_{3x3} (sign of P
 * flipped first if det M < 0), t = p4 / mean(singular values of M). */
int sfm_pnp_fit(const double* pts, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, const double* K, double* model,
                int32_t* flags, void* stream);

/* Philox sampling fused into the fit: hypothesis h of entry b uses the first 6 of philox_sample8(seed + b * seed_stride,
 * h_begin + h), the sampler of sfm_sample_philox; all 8 are stored in S (-1 at positions >= n). */
int sfm_pnp_sample_fit_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pts, int64_t n,
                              int64_t h_count, int64_t batch, const double* K, int32_t* S, double* model, int32_t* flags,
                              void* stream);

/* Scoring of all n items under all hypotheses: e = (p0/c2 - u)^2 + (p1/c2 - v)^2 with c = R X + t, p = K c (operation order
 * fixed in sfm_pnp.hip), +inf when c2 <= 0.  The first sample_size entries of a row of S are the sample (6 for the DLT, 4 for
 * P3P; SFM_EINVAL otherwise).  cnt[b,h] = non-sample items with e <= thr; s1 / s2 = sums of e / e^2 over the sample_size
 * sample items plus those survivors.  All fp64, exact divisions: the values are the host scorer's bit for bit.  Selection:
 * sfm_select_best with the same sample_size. */
int sfm_pnp_score(const double* pts, int64_t n, const double* model, const int32_t* S, int64_t h_count, int64_t batch,
                  const double* K, double thr, int sample_size, int32_t* cnt, double* s1, double* s2, void* stream);

/* Inlier mask of the selected model: 2 for the sample_size (6 or 4) sample items, 1 for other items with e <= thr, 0 otherwise
 * (all 0 when the record holds no model).  `result` as written by sfm_select_best with h_offset 0.  mask: dev uint8 [batch,n]. */
int sfm_pnp_inlier_mask(const double* pts, int64_t n, const double* model, const int32_t* S, int64_t h_count, int64_t batch,
                        const double* K, const sfm_select_result* result, double thr, int sample_size, uint8_t* mask, void* stream);

#define SFM_PNP_SOLVER_DLT 0 /* six-point DLT, six-item samples */
#define SFM_PNP_SOLVER_P3P 1 /* P3P, four-item samples; n >= 4 */

/* One whole PnP pass with the fit of `solver` (use_philox: sampled in the fit launch as sfm_pnp_sample_fit_philox /
 * sfm_p3p_sample_fit_philox, else from S), then the scoring, selection (sfm_select_best) and, when `mask` is not NULL, the
 * mask of its sample size — every argument checked before the first launch. */
int sfm_pnp_ransac_pass(int solver, uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* pts,
                        int64_t n, int64_t h_count, int64_t batch, const double* K, double thr, double min_extra, int aggregation,
                        int32_t* S, double* model, int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result,
                        uint8_t* mask, void* stream);

/* ---- P3P: the minimal solver of RANSAC PnP (csrc/sfm_p3p.h, csrc/sfm_pnp.hip; an extension, added under ABI 14) ----
 * Four-item samples: the first 4 entries of each row of S (the same [batch,h_count,8] tables).  Items 0-2 are solved for
 * (up to four poses with depths lambda_i > 0 along f_i = normalise(K^-1 (u_i, v_i, 1)) and |lambda_i f_i - lambda_j f_j| =
 * |X_i - X_j|), item 3 picks the pose with the strictly lowest sfm_pnp_score error, the earliest on ties.  A sample with no
 * such pose ("no solution") gets a model of 12 NaNs and flag 0: it never gates nor wins.  flags: SFM_FIT_DEGENERATE when
 * items 0-2 are collinear or coincide (|(X1-X0) x (X2-X0)|^2 <= 1e-18 |X1-X0|^2 |X2-X0|^2) or an index is out of range.
 * Coplanar samples are not degenerate.  n >= 4. */
int sfm_p3p_fit(const double* pts, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, const double* K, double* model,
                int32_t* flags, void* stream);

/* Philox sampling fused into the P3P fit (first 4 of philox_sample8, all 8 stored in S, -1 at positions >= n). */
int sfm_p3p_sample_fit_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pts, int64_t n,
                              int64_t h_count, int64_t batch, const double* K, int32_t* S, double* model, int32_t* flags,
                              void* stream);


/* ---- five-point essential matrix (csrc/sfm_five_point.hip; an extension, off unless asked for) ----
 * corr: dev [batch,n,4] K-normalised {xa, ya, xb, yb}; S: dev int32 [batch,h_count,8], the first 6 entries of a row are the
 * sample: items 0-4 are solved for, item 5 picks the candidate with the smallest SED (strict <, the earlier root on ties).
 * E: dev [batch,h_count,9], scaled to ||E||_F = sqrt(2) with its largest-magnitude entry positive (E[2,2] is not 1); 9 NaNs
 * with flag 0 when the sample has no real solution.  flags: SFM_FIT_DEGENERATE when the 5 x 9 system of items 0-4 has
 * numerical rank < 5 (collinear or repeated items), an input is not finite or an index is out of range.  n >= 6. */
int sfm_five_point_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* E, int32_t* flags,
                       void* stream);

/* Philox sampling fused into the five-point fit (first 6 of philox_sample8, all 8 stored in S, -1 at positions >= n). */
int sfm_five_point_sample_fit_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n,
                                     int64_t h_count, int64_t batch, int32_t* S, double* E, int32_t* flags, void* stream);

/* Every candidate of items 0-4 of each sample in ascending root order: out dev [batch,h_count,10,9] (NaN beyond the count),
 * count dev int32 [batch,h_count] (-1 for a sample sfm_five_point_fit flags). */
int sfm_five_point_candidates(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* out,
                              int32_t* count, void* stream);

/* sfm_score_sed (all-fp64 kernel) for samples of sample_size items (6 or 8; SFM_EINVAL otherwise): the first sample_size
 * entries of a row of S are the sample (select and mask with the same sample_size). */
int sfm_score_sed_sample_ex(const double* corr, int64_t n, const double* E, const int32_t* S, int64_t h_count, int64_t batch,
                            double thr, int sample_size, int32_t* cnt, double* s1, double* s2, void* stream);

/* One five-point pass: fit (from S, or Philox-sampled with use_philox), six-item scoring, selection and (mask != NULL) the
 * winner's mask, as the separate calls above.  Every size is checked before the first launch. */
int sfm_five_point_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S, double* E,
                               int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                               void* stream);

/* ---- RANSAC homography (csrc/sfm_homography.hip; an extension, added under ABI 15) ----
 * corr: dev [batch,n,4] = {xa, ya, xb, yb} in any one unit (the public route passes K-normalised coordinates); S: dev int32
 * [batch,h_count,8], the first 4 entries of a row are the sample.  H: dev [batch,h_count,9] row-major with x_b ~ H x_a,
 * ||H||_F = 1 and det H >= 0.  flags: SFM_FIT_DEGENERATE when sigma_8 / sigma_1 of the conditioned 8 x 9 DLT system is below
 * 1e-9 or not a number (a repeated item, three points collinear in both images, four coincident points) or an index is out
 * of range; det H is not tested (three points collinear in one image only give a singular H, which cannot win).  n >= 4. */

/* Four-point DLT fit of every hypothesis: each side conditioned per sample (centroid, mean distance sqrt(2)), null vector of
 * the 8 x 9 system by Householder QR, conditioning undone in closed form, scale and sign as above. */
int sfm_homography_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* H, int32_t* flags,
                       void* stream);

/* Scoring of all n items under all hypotheses with the symmetric transfer error e = |H xa - xb|^2 + |adj(H) xb - xa|^2 in
 * inhomogeneous coordinates (operation order fixed in sfm_homography.h), +inf when either third coordinate is <= 0.
 * cnt[b,h] = non-sample items with e <= thr; s1 / s2 = sums of e / e^2 over the 4 sample items plus those survivors.  All
 * fp64, exact divisions: the values are the host scorer's bit for bit.  Selection: sfm_select_best with sample_size 4. */
int sfm_homography_score(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch,
                         double thr, int32_t* cnt, double* s1, double* s2, void* stream);

/* Inlier mask of the selected model: 2 for its 4 sample items, 1 for other items with e <= thr, 0 otherwise (all 0 when the
 * record holds no model).  `result` as written by sfm_select_best with h_offset 0.  mask: dev uint8 [batch,n]. */
int sfm_homography_inlier_mask(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count,
                               int64_t batch, const sfm_select_result* result, double thr, uint8_t* mask, void* stream);

/* One homography pass: fit (from S, or with use_philox from the first 4 of philox_sample8(seed + b * seed_stride, h_begin + h),
 * all 8 stored in S, -1 at positions >= n), scoring, selection (sfm_select_best) and, when `mask` is not NULL, the winner's
 * mask — every argument checked before the first launch. */
int sfm_homography_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr,
                               int64_t n, int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation,
                               int32_t* S, double* H, int32_t* flags, int32_t* cnt, double* s1, double* s2,
                               sfm_select_result* result, uint8_t* mask, void* stream);

/* ---- two-view verification of every pair of a match graph in one call (csrc/sfm_view_graph.hip; an
 * extension, added under ABI 15) ----
 * corr: dev [n_total,4], the K-normalised correspondences of all pairs, concatenated; offset: dev int64 [pairs+1], pair q owns
 * items offset[q] .. offset[q+1]-1 (n_q of them, any count, 0 included); min_extra: dev double [pairs], the gate of pair q.
 * Pair q's outputs are those of sfm_homography_ransac_pass(seed + q * seed_stride, seed_stride, use_philox = 1, h_begin,
 * its items, n_q, h_count, 1, thr, min_extra[q], aggregation, ...) followed by sfm_five_point_ransac_pass(use_philox = 0) on
 * the rows of S the first one filled:
 *   S int32 [pairs,h_count,8]; H, E [pairs,h_count,9]; h_* / e_* flags, cnt int32 and s1, s2 double [pairs,h_count];
 *   h_result, e_result [pairs] (best_h local to the pair); h_mask, e_mask uint8 [n_total] (0 for an item no pair owns);
 *   verdict [pairs].
 * Every element of every output is written.  A pair with n_q below a model's sample size (4 for H, 6 for E) gets that model's
 * filler: 9 NaNs, flag SFM_FIT_DEGENERATE, cnt 0, s1 = s2 = NaN, hence a record without a winner (n_flagged = h_count); with
 * n_q < 4 the rows of S are -1 throughout.
 * The offset table is checked on the device by the first launch: unless 0 <= offset[0] <= ... <= offset[pairs] <= n_total,
 * every pair is treated as empty (filler throughout, masks 0) and every verdict is SFM_PAIR_BAD_OFFSETS; that is a status,
 * not an error return, and nothing is read through such a table.
 * Seven launches whatever `pairs` is, nothing read back; every size is checked before the first launch (pairs <= 65535,
 * n_total < 2^31); pairs == 0 is a no-op.  No atomics: a call is reproducible bit for bit. */
#define SFM_PAIR_NONE 0        /* neither model has a winner */
#define SFM_PAIR_ESSENTIAL 1   /* an essential matrix explains the pair */
#define SFM_PAIR_HOMOGRAPHY 2  /* E has no winner, or homography_count / essential_count > max_ratio */
#define SFM_PAIR_BAD_OFFSETS 3 /* the offset table of the call is not non-decreasing within [0, n_total]: every pair, no model */

typedef struct sfm_pair_verdict {
    int32_t kind;             /* SFM_PAIR_* */
    int32_t homography_count; /* the H winner's sample size (4) plus its extra inliers, 0 without a winner */
    int32_t essential_count;  /* the same for E (sample size 6) */
    int32_t reserved;         /* 0 */
    double ratio;             /* homography_count / essential_count, +inf when essential_count is 0 */
} sfm_pair_verdict;
#ifdef __cplusplus
static_assert(sizeof(sfm_pair_verdict) == 24, "sfm_pair_verdict is 24 bytes");
#endif

int sfm_verify_pairs(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n_total,
                     const int64_t* offset, int64_t pairs, const double* min_extra, int64_t h_count, double thr, int aggregation,
                     double max_ratio, int32_t* S, double* H, double* E, int32_t* h_flags, int32_t* h_cnt, double* h_s1,
                     double* h_s2, int32_t* e_flags, int32_t* e_cnt, double* e_s1, double* e_s2, sfm_select_result* h_result,
                     sfm_select_result* e_result, uint8_t* h_mask, uint8_t* e_mask, sfm_pair_verdict* verdict, void* stream);

/* ---- relative pose and triangulation angle of every pair, behind sfm_verify_pairs on that call's buffers
 * (csrc/sfm_view_graph_pose.hip; an extension, added under ABI 15) ----
 * corr, offset, E, e_result, e_mask, verdict: as sfm_verify_pairs took and left them.  Per pair q with an essential winner
 * (whatever its kind), E_q = E[q, e_result[q].best_h]:
 *   candidates  the four poses of sfm_decompose_essential(E_q), bit for bit, order (R1,t), (R1,-t), (R2,t), (R2,-t);
 *   items       those of pair q with e_mask != 0 (the sample and the survivors; none is skipped);
 *   cheirality  sfm_cheirality_batched's rule: DLT with P1 = [I|0], P2 = [R|t]; an item passes iff X[2] >= -1e-8 and
 *               z2 >= -1e-8 and |X| <= distance_threshold; NaN fails;
 *   votes[p]    the passing items of candidate p; best = the first maximum, -1 when all are zero;
 *   angle       of an item under the best R, each operation rounded on its own: a = (xa, ya, 1), c = R^T (xb, yb, 1) with
 *               c_j = (R[0][j] xb + R[1][j] yb) + R[2][j], w = a x c, atan2(sqrt((w0^2 + w1^2) + w2^2), (a0 c0 + a1 c1) + a2 c2);
 *   median      the lower median of the angles of the k = votes[best] items passing under the best pose: the element of
 *               rank (k - 1) / 2 in ascending order, selected exactly (a bit pattern of one of the angles).
 * Every byte of pose[q] is written for every q.  Unless status is SFM_POSE_OK, R, t and median_angle are NaN, best is -1 and
 * votes are 0.  workspace: dev, sfm_pair_poses_workspace_bytes(n_total, pairs) bytes (-1 for sizes the call refuses); after
 * the call its first n_total doubles hold each item's angle under its pair's best pose, NaN for an item that is not a passing
 * inlier of a pair with status SFM_POSE_OK.
 * Three launches whatever `pairs` is, nothing read back; every size and pointer is checked before the first launch
 * (pairs <= 65535, n_total < 2^31, h_count >= 1, the workspace size); pairs == 0 is a no-op that writes nothing, the angles
 * of the workspace included, whatever n_total is.  No global and no floating-point atomics: a call is reproducible bit for bit.
 * Nothing is indexed through an offset table marked SFM_PAIR_BAD_OFFSETS. */
#define SFM_POSE_OK 0
#define SFM_POSE_NO_MODEL 1      /* the pair has no essential winner (e_result[q].best_h < 0) */
#define SFM_POSE_NOT_ESSENTIAL 2 /* the decomposition's own status 1: sigma_3 not ~0 */
#define SFM_POSE_NO_VOTE 3       /* all four votes are zero */
#define SFM_POSE_BAD_OFFSETS 4   /* verdict[q].kind == SFM_PAIR_BAD_OFFSETS: every pair */

typedef struct sfm_pair_pose {
    double R[9];         /* row-major; x_b ~ R x_a + t */
    double t[3];         /* |t| = 1 */
    double median_angle; /* radians */
    int32_t votes[4];    /* passing inliers per candidate */
    int32_t best;        /* first maximum of votes, -1 if all are zero */
    int32_t status;      /* SFM_POSE_* */
} sfm_pair_pose;
#ifdef __cplusplus
static_assert(sizeof(sfm_pair_pose) == 128, "sfm_pair_pose is 128 bytes");
#endif

int64_t sfm_pair_poses_workspace_bytes(int64_t n_total, int64_t pairs);
int sfm_pair_poses(const double* corr, int64_t n_total, const int64_t* offset, int64_t pairs, const double* E, int64_t h_count,
                   const sfm_select_result* e_result, const uint8_t* e_mask, const sfm_pair_verdict* verdict,
                   double distance_threshold, sfm_pair_pose* pose, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- refinement of every pair's relative pose on its inliers, behind sfm_pair_poses on that call's buffers
 * (csrc/sfm_view_graph_refine.hip; an extension, off unless asked for, added under ABI 15) ----
 * corr, offset: as sfm_verify_pairs took them; pose_in: dev [pairs], as sfm_pair_poses left it.  Per pair q with
 * pose_in[q].status == SFM_POSE_OK, with E = [t]x R (each entry two products and one subtraction) and e the value of
 * sfm_sed_values under E:
 *   start set   the items of the pair with e <= thr under the start pose, scored here (e_mask is not read: a sample item
 *               that is an outlier stays out; a NaN item never enters);
 *   a round     Levenberg-Marquardt on the current set I (at most `max_steps` trial steps) minimising C = sum over I of e,
 *               written as the two residuals r / sqrt(da), r / sqrt(db) per item, over five unknowns: R <- exp([w]x) R and
 *               t <- (t + a b1 + b b2) / |t + a b1 + b b2| with b1 = (t x e_i) / |t x e_i|, b2 = t x b1, e_i the axis of the
 *               smallest |t_i| (the first on ties); damping lambda diag(H) from 1e-3 (/10 on an accepted step, *10
 *               otherwise).  Then every item of the pair is re-scored and the result kept iff it has more items within thr,
 *               or as many and a lower aggregated error (`aggregation` over those items, no sample term); a kept result's
 *               inliers are the next round's set, a result that is not kept ends the rounds.  A round stops at once when the
 *               Gauss-Newton matrix of its start point is rank-deficient (a Cholesky pivot <= 1e-10 of its diagonal entry);
 *               fewer than 6 items in the set end the rounds.
 * pose_out: dev [pairs], pose_in byte for byte with R and t replaced when at least one round was kept; votes, best,
 * median_angle and status are carried over, not recomputed under the refined pose.  pose_out must not alias pose_in.
 * mask_out: dev uint8 [n_total], 1 for an item within thr under its pair's kept pose, 0 elsewhere (pairs without a pose,
 * items no pair owns).  info: dev [pairs].  Every byte of every output is written.
 * Segment bounds are clamped to [0, n_total]; a pose table marked SFM_POSE_BAD_OFFSETS has no pair with a pose, so nothing
 * is read through its offset table.  Two launches whatever `pairs` is, nothing read back; every size and pointer is checked
 * before the first launch (pairs <= 65535, n_total < 2^31, rounds >= 0, max_steps >= 0, the aggregation); pairs == 0 is a
 * no-op that writes nothing.  No atomics: a call is reproducible bit for bit. */
#define SFM_PAIR_REFINE_OK 0      /* the pair had a pose and at least 6 items within thr under it */
#define SFM_PAIR_REFINE_NO_POSE 1 /* pose_in[q].status != SFM_POSE_OK: pose_out[q] = pose_in[q], errors NaN, counts 0 */
#define SFM_PAIR_REFINE_TOO_FEW 2 /* fewer than 6 items within thr under the start pose: the pose is unchanged */

typedef struct sfm_pair_refine_info {
    double start_error;  /* aggregated error of pose_in over its start set */
    double error;        /* aggregated error of the pose left in pose_out over its `count` inliers */
    int32_t start_count; /* items within thr under pose_in */
    int32_t count;       /* items within thr under pose_out: the ones of mask_out */
    int32_t accepted;    /* rounds whose result was kept (0 = pose_out is pose_in) */
    int32_t lm_steps;    /* Levenberg-Marquardt trial steps over all rounds */
    int32_t status;      /* SFM_PAIR_REFINE_* */
    int32_t reserved;    /* 0 */
} sfm_pair_refine_info;
#ifdef __cplusplus
static_assert(sizeof(sfm_pair_refine_info) == 40, "sfm_pair_refine_info is 40 bytes");
#endif

int sfm_refine_pair_poses(const double* corr, int64_t n_total, const int64_t* offset, int64_t pairs, const sfm_pair_pose* pose_in,
                          double thr, int aggregation, int rounds, int max_steps, sfm_pair_pose* pose_out, uint8_t* mask_out,
                          sfm_pair_refine_info* info, void* stream);

/* ---- refinement of a PnP winner on its inliers (csrc/sfm_pnp_refine.hip; an extension, off unless asked for) ---- */

typedef struct sfm_pnp_refine_info {
    double error;     /* aggregated error of the model left in model_out (over its `count` inliers) */
    int32_t count;    /* inliers of that model (for an unrefined model: non-zero entries of mask_in) */
    int32_t accepted; /* rounds whose result was kept (0 = model_out is model_in) */
    int32_t lm_steps; /* Levenberg-Marquardt trial steps over all rounds */
    int32_t reserved; /* 0 */
} sfm_pnp_refine_info;

/* Per view, up to `rounds` times: Levenberg-Marquardt on the current inliers I (at most `max_steps` trial steps) minimising
 * C = sum over I of the squared reprojection error e of sfm_pnp_score (+inf behind the camera), with R <- exp([w]x) R,
 * t <- t + dt, damping lambda diag(H) from 1e-3 (/10 on an accepted step, *10 otherwise); then every item re-scored
 * (e <= thr) and the result kept iff it has more inliers, or as many and a lower aggregated error.  A round stops early
 * when |I| < 6 or when the Gauss-Newton matrix of its start point is rank-deficient (a Cholesky pivot <= 1e-10 of its
 * diagonal entry).  pts: dev [batch,n,5] as sfm_pnp_score; K: host [9], row 2 (0, 0, 1); model_in: dev [batch,12], R | t
 * of each view (e.g. model[b, best_h] of a pass); mask_in: dev uint8 [batch,n], non-zero = inlier (as written by
 * sfm_pnp_inlier_mask); err_in: dev [batch], the aggregated error of model_in (sfm_select_result.best_err);
 * model_out: dev [batch,12] (may be model_in); mask_out: dev uint8 [batch,n], 1 = inlier, must not alias mask_in;
 * info: dev [batch].  A view whose mask is all zero keeps its model and reports count 0. */
int sfm_pnp_refine(const double* pts, int64_t n, int64_t batch, const double* K, const double* model_in, const uint8_t* mask_in,
                   const double* err_in, double thr, int aggregation, int rounds, int max_steps, double* model_out,
                   uint8_t* mask_out, sfm_pnp_refine_info* info, void* stream);

/* ---- absolute pose of every candidate view against the model in one call (csrc/sfm_register_views.hip; an
 * extension, added under ABI 15) ----
 * pts: dev [n_total,5] = {X, Y, Z, u, v} as sfm_pnp_score takes them, the 2D-3D items of all views, concatenated; offset: dev
 * int64 [views+1], view v owns items offset[v] .. offset[v+1]-1 (n_v of them, any count, 0 included); min_extra: dev double
 * [views], the gate of view v; K: host [9], row 2 (0, 0, 1).  View v's outputs are those of
 * sfm_pnp_ransac_pass(SFM_PNP_SOLVER_P3P, seed + v * seed_stride, seed_stride, use_philox = 1, h_begin, its items, n_v, h_count,
 * 1, K, thr, min_extra[v], aggregation, ...) with a mask, followed by sfm_pnp_refine(its items, n_v, 1, K, model[v, best_h],
 * that mask with the winner's sample item 3 cleared, the record's best_err, thr, aggregation, refine_rounds, refine_max_steps,
 * ...), bit for bit:
 *   S int32 [views,h_count,8]; model [views,h_count,12]; flags, cnt int32 and s1, s2 double [views,h_count]; result [views]
 *   (best_h local to the view); mask uint8 [n_total] (2 sample item of the winner, 1 other inlier, 0 otherwise);
 *   pose_out [views,12]; mask_out uint8 [n_total] (1 = inlier of pose_out), must not alias mask; info [views]; status int32
 *   [views].
 * refine_rounds = 0 means what it means for sfm_pnp_refine: pose_out is the winner, mask_out is mask != 0 with item 3 cleared,
 * accepted = lm_steps = 0.  Only the P3P solver is supported.  Every element of every output is written; a mask byte that no
 * view owns is 0.  A view without a winner has pose_out = 12 NaNs, its mask and mask_out bytes 0 and info {+inf, 0, 0, 0}; a
 * view with n_v < 4 also gets the pass's filler: rows of S all -1, models of 12 NaNs, flags SFM_FIT_DEGENERATE, cnt 0,
 * s1 = s2 = NaN, hence a record without a winner (n_flagged = h_count).
 * The offset table is checked on the device by the first launch: unless 0 <= offset[0] <= ... <= offset[views] <= n_total,
 * every view is treated as empty (filler throughout, masks 0) and every status is SFM_REGISTER_BAD_OFFSETS; that is a status,
 * not an error return, and nothing is read through such a table.
 * Six launches whatever `views` is, nothing read back; every size and pointer is checked before the first launch
 * (views <= 65535, n_total < 2^31, h_count >= 1, h_begin >= 0, refine_rounds >= 0, refine_max_steps >= 0, the aggregation,
 * K); views == 0 is a no-op that writes nothing.  No atomics: a call is reproducible bit for bit. */
#define SFM_REGISTER_OK 0          /* the view has a winner: pose_out is that winner, refined where a round was kept */
#define SFM_REGISTER_NO_MODEL 1    /* n_v >= 4, but no hypothesis passed the gate */
#define SFM_REGISTER_TOO_FEW 2     /* n_v < 4 */
#define SFM_REGISTER_BAD_OFFSETS 3 /* the offset table of the call is not non-decreasing within [0, n_total]: every view */

int sfm_register_views(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pts, int64_t n_total,
                       const int64_t* offset, int64_t views, const double* min_extra, const double* K, int64_t h_count,
                       double thr, int aggregation, int refine_rounds, int refine_max_steps, int32_t* S, double* model,
                       int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                       double* pose_out, uint8_t* mask_out, sfm_pnp_refine_info* info, int32_t* status, void* stream);

/* ---- RANSAC similarity alignment of two reconstructions (csrc/sfm_similarity.hip; an extension, added under
 * ABI 15) ----
 * pairs: dev [batch,n,6] = {ax, ay, az, bx, by, bz}, 16-byte aligned; a model is 13 doubles R (row-major) | t | s with
 * b ~ s R a + t.  The error of a pair is e = |s R a + t - b|^2, squared and in the units of side B (operation order fixed in
 * csrc/sfm_similarity.h).  The least-squares model of an index set I (Umeyama 1991; Horn 1987): mu_a, mu_b the means over I,
 * a' = a - mu_a, b' = b - mu_b, M = sum b' a'^T, sa2 = sum |a'|^2, sb2 = sum |b'|^2; R = argmax over SO(3) of tr(R^T M), always
 * a proper rotation; s = tr(R^T M) / sa2; t = mu_b - s R mu_a.  With sigma_1 >= sigma_2 >= sigma_3 the singular values of M and
 * d = sigma_2 + sign(det M) sigma_3 (d = sigma_2 when det M = 0), the flag is SFM_FIT_DEGENERATE when d <= 1e-9 sqrt(sa2 sb2),
 * sa2 = 0, s is not finite or <= 0, anything is not a number or, for a minimal fit, a sample index lies outside [0, n).
 * n >= 3. */

/* One similarity pass: three-item fit (from S, or with use_philox from the first 3 of philox_sample8(seed + b * seed_stride,
 * h_begin + h), all 8 stored in S, -1 at positions >= n), scoring (cnt[b,h] = non-sample items with e <= thr; s1 / s2 = sums of
 * e / e^2 over the 3 sample items plus those survivors), selection (sfm_select_best with sample_size 3) and, when `mask` is not
 * NULL, the winner's mask (2 sample item, 1 other inlier, 0 otherwise; all 0 without a winner) — every argument checked before
 * the first launch.  S: dev int32 [batch,h_count,8]; model: dev [batch,h_count,13]; flags, cnt: dev int32 and s1, s2: dev double
 * [batch,h_count]; result: dev [batch]; mask: dev uint8 [batch,n] or NULL. */
int sfm_similarity_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* pairs, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S,
                               double* model, int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result,
                               uint8_t* mask, void* stream);

/* Bytes of workspace sfm_similarity_fit_masked needs; -1 for sizes it refuses (n < 3, n >= 2^31, batch < 0 or > 65535). */
int64_t sfm_similarity_fit_workspace_bytes(int64_t n, int64_t batch);

/* The least-squares model of the set {i : mask[b,i] != 0} of every entry, or of all n items when mask is NULL: one model and
 * one flag per entry.  Two reduction passes (centroid, then centred moments) over up to 128 blocks per entry whose partial sums
 * are added in block order, then the solve: three launches, no atomics, bit-reproducible.  mask: dev uint8 [batch,n] or NULL;
 * model_out: dev [batch,13]; flags_out: dev int32 [batch]; workspace: dev, 16-byte aligned, at least
 * sfm_similarity_fit_workspace_bytes(n, batch).  SFM_EINVAL before the first launch for a refused size, a null or misaligned
 * pointer or a workspace too small; batch == 0 is a no-op. */
int sfm_similarity_fit_masked(const double* pairs, int64_t n, int64_t batch, const uint8_t* mask, double* model_out, int32_t* flags_out,
                              void* workspace, int64_t workspace_bytes, void* stream);

typedef struct sfm_similarity_refine_info {
    double error;       /* aggregated error of the model left in model_out (over its `count` inliers) */
    int32_t count;      /* inliers of that model (for an unrefined model: non-zero entries of mask_in) */
    int32_t accepted;   /* rounds whose result was kept (0 = model_out is model_in) */
    int32_t rounds_run; /* rounds that fitted a model: entered with at least 3 inliers (a degenerate or rejected one included) */
    int32_t reserved;   /* 0 */
} sfm_similarity_refine_info;

/* Bytes of workspace sfm_similarity_refine needs; -1 for sizes it refuses (as sfm_similarity_fit_workspace_bytes). */
int64_t sfm_similarity_refine_workspace_bytes(int64_t n, int64_t batch);

/* Per entry, up to `rounds` times: the least-squares model of the current inliers (the reductions and the solve of
 * sfm_similarity_fit_masked), every item re-scored (e <= thr), and the result kept iff it has more inliers, or as many and a
 * lower aggregated error (the rule of sfm_pnp_refine).  A round stops early with fewer than 3 inliers or a degenerate set, and
 * nothing follows a rejected round.  model_in: dev [batch,13] (e.g. model[b, best_h] of a pass); mask_in: dev uint8 [batch,n],
 * non-zero = inlier; err_in: dev [batch], the aggregated error of model_in (sfm_select_result.best_err); model_out: dev
 * [batch,13]; mask_out: dev uint8 [batch,n], 1 = inlier, must not alias mask_in; info: dev [batch]; workspace: dev, 16-byte
 * aligned, at least sfm_similarity_refine_workspace_bytes(n, batch).  An entry whose mask is all zero keeps its model and reports
 * count 0; rounds = 0 copies.  2 + 4 rounds launches, nothing read back; SFM_EINVAL before the first launch for a refused size,
 * rounds < 0, an unknown aggregation, a null or misaligned pointer or a workspace too small. */
int sfm_similarity_refine(const double* pairs, int64_t n, int64_t batch, const double* model_in, const uint8_t* mask_in,
                          const double* err_in, double thr, int aggregation, int rounds, double* model_out, uint8_t* mask_out,
                          sfm_similarity_refine_info* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- similarity alignment of every overlapping pair of sub-models in one call (csrc/sfm_align_models.hip; an
 * extension, added under ABI 15) ----
 * pairs: dev [n_total,6] = {ax, ay, az, bx, by, bz} as sfm_similarity_ransac_pass takes them, the items of all sub-model pairs,
 * concatenated, 16-byte aligned; offset: dev int64 [pair_count+1], pair q owns items offset[q] .. offset[q+1]-1 (n_q of them, any
 * count, 0 included); max_items: host, an upper bound on every n_q (it sizes the grid of the reduction passes: the host never
 * reads the table); thr: dev double [pair_count], squared distance in the units of side B of pair q; min_extra: dev double
 * [pair_count], the gate of pair q.  Pair q's outputs are those of sfm_similarity_ransac_pass(seed + q * seed_stride, seed_stride,
 * use_philox = 1, h_begin, its items, n_q, h_count, 1, thr[q], min_extra[q], aggregation, ...) with a mask, followed by
 * sfm_similarity_refine(its items, n_q, 1, model[q, best_h], that mask, the record's best_err, thr[q], aggregation, refine_rounds,
 * ...), bit for bit:
 *   S int32 [pair_count,h_count,8]; model [pair_count,h_count,13]; flags, cnt int32 and s1, s2 double [pair_count,h_count]; result
 *   [pair_count] (best_h local to the pair); mask uint8 [n_total] (2 sample item of the winner, 1 other inlier, 0 otherwise);
 *   model_out [pair_count,13]; mask_out uint8 [n_total] (1 = inlier of model_out), must not alias mask; info [pair_count]; status
 *   int32 [pair_count].
 * refine_rounds = 0 means what it means for sfm_similarity_refine: model_out is the winner, mask_out is mask != 0.  Every element
 * of every output is written; a mask byte that no pair owns is 0.  A pair without a winner has model_out = 13 NaNs, its mask and
 * mask_out bytes 0 and info {+inf, 0, 0, 0, 0} (not the single call's "row 0 with an empty mask"); a pair with n_q < 3 also gets
 * the pass's filler: rows of S all -1, models of 13 NaNs, flags SFM_FIT_DEGENERATE, cnt 0, s1 = s2 = NaN, hence a record without a
 * winner (n_flagged = h_count).
 * The offset table is checked on the device by the first launch: unless 0 <= offset[0] <= ... <= offset[pair_count] <= n_total
 * and every n_q <= max_items, every pair is treated as empty (filler throughout, masks 0) and every status is
 * SFM_ALIGN_BAD_OFFSETS; that is a status, not an error return, and nothing is read through such a table.
 * workspace: dev, 16-byte aligned, at least sfm_align_models_workspace_bytes(n_total, pair_count, max_items).
 * 7 + 4 refine_rounds launches whatever pair_count is, nothing read back; every size and pointer is checked before the first
 * launch (pair_count <= 65535, n_total < 2^31, 0 <= max_items <= n_total, h_count >= 1, h_begin >= 0, refine_rounds >= 0, the
 * aggregation, alignment, the workspace); pair_count == 0 is a no-op that writes nothing.  No atomics: a call is reproducible bit
 * for bit. */
#define SFM_ALIGN_OK 0          /* the pair has a winner: model_out is that winner, refitted where a round was kept */
#define SFM_ALIGN_NO_MODEL 1    /* n_q >= 3, but no hypothesis passed the gate */
#define SFM_ALIGN_TOO_FEW 2     /* n_q < 3 */
#define SFM_ALIGN_BAD_OFFSETS 3 /* the offset table of the call was refused: every pair */

/* Bytes of workspace sfm_align_models needs; -1 for sizes it refuses (n_total < 0 or >= 2^31, pair_count < 0 or > 65535,
 * max_items < 0 or > n_total). */
int64_t sfm_align_models_workspace_bytes(int64_t n_total, int64_t pair_count, int64_t max_items);

int sfm_align_models(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pairs, int64_t n_total,
                     const int64_t* offset, int64_t pair_count, int64_t max_items, const double* thr, const double* min_extra,
                     int64_t h_count, int aggregation, int refine_rounds, int32_t* S, double* model, int32_t* flags, int32_t* cnt,
                     double* s1, double* s2, sfm_select_result* result, uint8_t* mask, double* model_out, uint8_t* mask_out,
                     sfm_similarity_refine_info* info, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- plane-sweep depth maps and their consistency filter (csrc/sfm_plane_sweep.hip; an extension, added under
 * ABI 15) ----
 * Both calls are defined as a fixed sequence of fp64 + - * / sqrt (DESIGN.md §6ai states it; tests/plane_sweep_oracle.py is the
 * same sequence in NumPy), so their outputs are reproducible bit for bit. */
#define SFM_SWEEP_OK 0            /* the reference index is a view: its maps are computed */
#define SFM_SWEEP_BAD_REFERENCE 1 /* refs[r] is outside [0, views): the maps of r hold the filler */

/* Bytes of workspace sfm_plane_sweep needs (the homographies, [refs, sources, depths, 9] doubles); -1 for sizes it refuses
 * whatever the radius: views < 1, height or width < 4, height * width >= 2^31, refs < 0 or > 65535, sources outside [1, 8],
 * depths outside [1, 4096]. */
int64_t sfm_plane_sweep_workspace_bytes(int64_t views, int64_t height, int64_t width, int64_t refs, int64_t sources, int64_t depths);

/* One depth map per reference view by plane-sweep stereo.
 * images: dev uint8 [views,height,width], grey, all of one size; K: dev [9], upper triangular (the entries 0, 1, 2, 4, 5 are read);
 * poses: dev [views,12], world to camera, R row-major (9) then t (3); refs: dev int32 [ref_count]; sources: dev int32 [ref_count,source_count],
 * a slot that is -1, outside [0, views) or the reference itself is absent; depths: dev [ref_count,depth_count], the hypotheses of
 * each reference, a non-finite or non-positive one is invalid.  Host scalars: the window is (2 radius + 1)^2 pixels, 1 <= radius
 * <= 5; the cost of a hypothesis is the mean of its top_k lowest source scores (0: all); it is valid with at least min_sources >= 1
 * valid scores; a score is valid with both window variances (times n^2) at least min_variance n^2, min_variance >= 0.
 * Outputs, every element written: depth [ref_count,height,width] (the winner's depth after a parabola step in inverse depth, NaN
 * without a winner), index int32 (the winner, -1 without), cost (the winner's, NaN without), status int32 [ref_count] (SFM_SWEEP_*),
 * and, unless NULL, volume [ref_count,depth_count,height,width] (the cost of each hypothesis, NaN where invalid).  A reference with
 * status SFM_SWEEP_BAD_REFERENCE has depth = cost = NaN, index = -1 and a volume of NaNs; that is a status, never an error return,
 * and no table is read by the host.
 * workspace: dev, 16-byte aligned, at least sfm_plane_sweep_workspace_bytes(...).  Two launches, no atomics, no memset, the same
 * bits on every call.  SFM_EINVAL before the first launch for a refused size (as above; height and width at least 2 radius + 2), a
 * scalar out of range, a null or misaligned pointer or a workspace too small; ref_count == 0 is a no-op. */
int sfm_plane_sweep(const uint8_t* images, int64_t views, int64_t height, int64_t width, const double* K, const double* poses,
                    const int32_t* refs, int64_t ref_count, const int32_t* sources, int64_t source_count, const double* depths,
                    int64_t depth_count, int radius, int top_k, int min_sources, double min_variance, double* depth, int32_t* index,
                    double* cost, int32_t* status, double* volume, void* workspace, int64_t workspace_bytes, void* stream);

/* Forward-backward consistency of depth maps across views.
 * depth: dev [views,height,width], NaN = none; K, poses, refs, sources as for sfm_plane_sweep.  A pixel of view refs[r] with a finite
 * depth d is taken to the world, into each source, to the nearest pixel there (which must lie in the image and hold a finite depth),
 * back to the world with that depth and into the reference again as (x', y', z'); the source agrees iff
 * (x' - x)^2 + (y' - y)^2 <= max_pixel_error^2 and |z' - d| <= max_relative_depth_error d.
 * Outputs, every element written: count int32 [ref_count,height,width], the agreeing sources; filtered [ref_count,height,width], d
 * iff count >= min_consistent, else NaN; points [ref_count,height,width,3], the world point of a kept pixel, else NaN; status int32
 * [ref_count] (SFM_SWEEP_*; a bad reference has count 0 and NaNs).
 * One launch, no workspace, no atomics.  SFM_EINVAL before the launch for views < 1, height * width outside [1, 2^31), ref_count
 * outside [0, 65535], source_count outside [1, 8], a bound that is negative or not finite, min_consistent < 0 or a null or
 * misaligned pointer; ref_count == 0 is a no-op. */
int sfm_filter_depth_maps(const double* depth, int64_t views, int64_t height, int64_t width, const double* K, const double* poses,
                          const int32_t* refs, int64_t ref_count, const int32_t* sources, int64_t source_count, double max_pixel_error,
                          double max_relative_depth_error, int min_consistent, int32_t* count, double* filtered, double* points,
                          int32_t* status, void* stream);

/* ---- semi-global smoothing of the plane-sweep cost volume (csrc/sfm_sgm.hip; an extension, added under ABI 15) ----
 * The call is defined as a fixed sequence of fp64 + - * / min (DESIGN.md §6ak states it; tests/sgm_oracle.py is the same sequence in
 * NumPy), so its outputs are reproducible bit for bit. */

/* Bytes of workspace sfm_sgm_aggregate needs: the running sum, [refs, depths, height, width] doubles, when the call is not given an
 * `aggregated` to keep it in (keep_aggregated == 0), else 0; -1 for sizes it refuses: refs < 0 or > 65535, depths outside [1, 256],
 * height or width < 1, height * width >= 2^31. */
int64_t sfm_sgm_workspace_bytes(int64_t refs, int64_t depths, int64_t height, int64_t width, int keep_aggregated);

/* Semi-global aggregation of a cost volume along 4 or 8 scanline directions, and the winner of every pixel.
 * volume: dev [ref_count,depth_count,height,width] and depths: dev [ref_count,depth_count], what sfm_plane_sweep writes and reads.
 * C'(p, d) is volume[r,d,y,x] if finite, else invalid_cost; d is eligible at p iff volume[r,d,y,x] is finite and depths[r,d] is
 * finite and > 0.  Directions (dx, dy), in this order: (0,1) (1,1) (-1,1) (0,-1) (-1,-1) (1,-1) (1,0) (-1,0) for paths == 8,
 * (0,1) (0,-1) (1,0) (-1,0) for paths == 4.  Along direction k, with q = (x - dx, y - dy): L_k(p, d) = C'(p, d) if q is outside the
 * image, else (C'(p, d) + min(L_k(q, d), L_k(q, d-1) + p1 [d > 0], L_k(q, d+1) + p1 [d < depth_count-1], m + p2)) - m with
 * m = min_j L_k(q, j).  S = ((L_0 + L_1) + L_2) + ..., in the order of the list.
 * Outputs, every element written: aggregated [ref_count,depth_count,height,width], S at every hypothesis, eligible or not, or NULL
 * (the workspace then holds it); index int32 [ref_count,height,width], the eligible d of lowest S, ties to the lower index, -1
 * without one; cost, S at the winner, NaN without; depth, the winner's depth after the parabola step of sfm_plane_sweep on S in
 * inverse depth (both neighbours eligible), NaN without.  A volume of NaNs gives maps of NaN and -1.
 * workspace: dev, 16-byte aligned, at least sfm_sgm_workspace_bytes(..., aggregated != NULL).  paths + 1 launches whatever the
 * sizes, no atomics, no memset, nothing read by the host, the same bits on every call.  SFM_EINVAL before the first launch for a
 * refused size (as above), paths other than 4 or 8, p1, p2 or invalid_cost not finite or not 0 <= p1 <= p2, a null or misaligned
 * pointer, aggregated == volume or a workspace too small; ref_count == 0 is a no-op. */
int sfm_sgm_aggregate(const double* volume, int64_t ref_count, int64_t depth_count, int64_t height, int64_t width, const double* depths,
                      double p1, double p2, double invalid_cost, int paths, double* depth, int32_t* index, double* cost,
                      double* aggregated, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fusion of depth maps into a TSDF volume and the triangles of its zero level set (csrc/sfm_tsdf.hip; an
 * extension, added under ABI 15) ----
 * Both calls are defined as a fixed sequence of fp64 + - * / (DESIGN.md §6aj states it; tests/tsdf_oracle.py is the same sequence
 * in NumPy), so their outputs are reproducible bit for bit.  A volume has nx x ny x nz voxels, voxel (i, j, k) at the linear index
 * (k ny + j) nx + i with its centre at (ox + (i + 0.5) s, oy + (j + 0.5) s, oz + (k + 0.5) s), s = voxel_size. */
#define SFM_TSDF_OK 0       /* the view index is a view: its depth map was added */
#define SFM_TSDF_BAD_VIEW 1 /* view_list[n] is outside [0, views): the entry was skipped */

/* Average depth maps into a volume.
 * State, in-out, dev, so that views can be added in several calls (the caller zeroes a fresh volume): sum [nz,ny,nx] doubles, count
 * int32 [nz,ny,nx], grey_sum int32 [nz,ny,nx] or NULL.  Inputs, dev: depth [views,height,width], z-depths, a non-finite or
 * non-positive one is no depth; images uint8 [views,height,width] or NULL, NULL exactly when grey_sum is; K [9] and poses [views,12]
 * as for sfm_plane_sweep; view_list int32 [view_count], the views to add, in this order.  Host scalars: the origin, finite;
 * voxel_size and truncation, finite and > 0.
 * Per voxel and listed view: the centre is projected as sfm_filter_depth_maps projects a point; with a camera depth z > 0 and
 * the nearest pixel (floor(u + 0.5), floor(v + 0.5)) in the image holding a depth d, sdf = d - z; the view is skipped for
 * sdf < -truncation, else sum += sdf < truncation ? sdf / truncation : 1, count += 1 and grey_sum += the pixel's grey value.
 * A voxel depends on no other and adds its views in the order of the list: splitting the list over calls gives the same bytes.
 * Output: status int32 [view_count] (SFM_TSDF_*); a bad view index is a status, never an error return, and no table is read by
 * the host.  One launch, no workspace, no atomics, no memset.  SFM_EINVAL before the launch for nx, ny or nz < 1,
 * nx ny nz >= 2^31, views < 1, height * width outside [1, 2^31), view_count < 0, a scalar out of range, images and grey_sum not
 * both or neither NULL, or a null or misaligned pointer; view_count == 0 is a no-op. */
int sfm_tsdf_integrate(double* sum, int32_t* count, int32_t* grey_sum, int64_t nx, int64_t ny, int64_t nz, double ox, double oy, double oz,
                       double voxel_size, double truncation, const double* depth, const uint8_t* images, int64_t views, int64_t height,
                       int64_t width, const double* K, const double* poses, const int32_t* view_list, int64_t view_count, int32_t* status,
                       void* stream);

/* Bytes of workspace sfm_tsdf_extract_mesh needs (an int32 per cell and the tiles of the scan); -1 for sizes it refuses: nx, ny or
 * nz < 2, nx ny nz >= 2^31, or 12 (nx-1)(ny-1)(nz-1) >= 2^31 (twelve triangles a cell at most, counted in int32). */
int64_t sfm_tsdf_mesh_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);

/* The zero level set of a volume as triangles, by marching tetrahedra.
 * sum, count, grey_sum (or NULL): the state of sfm_tsdf_integrate, read only.  Cell (i, j, k), i < nx-1, j < ny-1, k < nz-1, has the
 * voxels (i + (q&1), j + ((q>>1)&1), k + ((q>>2)&1)) as corners q = 0..7; it is valid iff every corner has count >= min_count
 * (>= 1); a corner's value is sum / count, its grey grey_sum / count, and it is negative iff the value is < 0.  A valid cell is
 * split into the six tetrahedra (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7); each gives no, one or two triangles
 * with their vertices where the value interpolated along an edge is zero, oriented so that the normal (B - A) x (C - A) points to
 * the non-negative side (DESIGN.md §6aj has the table).
 * Outputs, dev, every element written: vertices [max_triangles,3,3]; grey [max_triangles,3], or NULL when grey_sum is NULL; total
 * int64 [1], the true number of triangles, also when it exceeds max_triangles.  The rows below min(total, max_triangles) hold
 * the first triangles in the order cells (x fastest), tetrahedra, triangles; every later row is NaN.  max_triangles == 0 asks
 * for the total alone (vertices and grey may then be NULL).
 * workspace: dev, 16-byte aligned, at least sfm_tsdf_mesh_workspace_bytes(...), taken as it comes.  Six launches, no atomics,
 * no memset, nothing read by the host, the same bits on every call.  SFM_EINVAL before the first launch for a refused size, a
 * scalar out of range, min_count < 1, max_triangles < 0, grey and grey_sum not both or neither NULL, a null or misaligned pointer
 * or a workspace too small. */
int sfm_tsdf_extract_mesh(const double* sum, const int32_t* count, const int32_t* grey_sum, int64_t nx, int64_t ny, int64_t nz, double ox,
                          double oy, double oz, double voxel_size, int min_count, int64_t max_triangles, double* vertices, double* grey,
                          int64_t* total, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- bundle adjustment of cameras and points (csrc/sfm_bundle.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 14 without a version change: they are new, and nothing an ABI-14 caller uses changed. */

#define SFM_BUNDLE_OK 0
#define SFM_BUNDLE_BAD_START 1 /* the starting cost is not finite (a point behind a camera, a NaN): output = input */
#define SFM_BUNDLE_BAD_INDEX 2 /* a camera or point index is out of range: output = input */

typedef struct sfm_bundle_info {
    double initial_cost; /* cost of the input (NaN for SFM_BUNDLE_BAD_INDEX) */
    double final_cost;   /* cost of the last accepted trial (= initial_cost when none was accepted) */
    int32_t steps;       /* Levenberg-Marquardt trial steps */
    int32_t accepted;    /* accepted steps */
    int32_t status;      /* SFM_BUNDLE_* */
    int32_t reserved;    /* 0 */
} sfm_bundle_info;

/* Bytes of workspace sfm_bundle_adjust needs; -1 for sizes it refuses. */
int64_t sfm_bundle_workspace_bytes(int64_t cameras, int64_t points, int64_t observations);

/* Levenberg-Marquardt on F = sum over the observations m of e_m, e the squared reprojection error of sfm_pnp_score (+inf
 * behind the camera), over every camera c with fixed[c] == 0 (R <- exp([w]x) R, t <- t + dt) and every point with at least
 * two observations (X <- X + dX); the other points and the fixed cameras are held.  Damping lambda diag(H) from 1e-3 (/10 on
 * an accepted step, *10 otherwise; a damped system that does not factor is a rejected step); at most max_steps trial steps,
 * stop at lambda > 1e16, on an accepted step that lowers F by less than 1e-12 of F, or on a step |delta| <= 1e-12 (1 + |x|).
 * With exactly one fixed camera, every accepted step is followed by a similarity about that camera's centre that restores the
 * input distance from it to the lowest-index free camera's centre: every point and every free camera's centre scale by the
 * same factor (F does not change).  The whole call is enqueued at once; the LM state stays on the device.
 * K: host [9], row 2 (0, 0, 1); fixed: host uint8 [cameras], at least one non-zero; poses_in / poses_out: dev [cameras,12]
 * (R | t, world -> camera); points_in / points_out: dev [points,3] (either may alias its input); camera_index, point_index:
 * dev int32 [observations]; pixels: dev [observations,2]; info: dev, one record; workspace: dev, 16-byte aligned, at least
 * sfm_bundle_workspace_bytes.  cameras <= 64; points, observations < 2^31. */
int sfm_bundle_adjust(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                      const double* poses_in, const double* points_in, const int32_t* camera_index,
                      const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                      double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- bundle adjustment with an iterative Schur solver (csrc/sfm_bundle_pcg.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 14 without a version change: they are new, and nothing an ABI-14 caller uses changed. */

typedef struct sfm_bundle_pcg_info {
    double initial_cost;   /* cost of the input (NaN for SFM_BUNDLE_BAD_INDEX) */
    double final_cost;     /* cost of the last accepted trial (= initial_cost when none was accepted) */
    int32_t steps;         /* Levenberg-Marquardt trial steps */
    int32_t accepted;      /* accepted steps */
    int32_t status;        /* SFM_BUNDLE_* */
    int32_t cg_iterations; /* conjugate-gradient iterations over all trial steps */
    int32_t cg_max;        /* the most conjugate-gradient iterations of one trial step */
    int32_t reserved;      /* 0 */
} sfm_bundle_pcg_info;

/* Bytes of workspace sfm_bundle_adjust_pcg needs; -1 for sizes it refuses (cameras < 1; points or observations < 0;
 * any of them >= 2^31).  There is no limit on the camera count below that. */
int64_t sfm_bundle_pcg_workspace_bytes(int64_t cameras, int64_t points, int64_t observations);

/* sfm_bundle_adjust's Levenberg-Marquardt loop (its cost, updates, damping, stops, held points and cameras, gauge rule and
 * statuses) over any number of cameras, with the damped reduced camera system S* dc = b (S* = U* - W V*^-1 W^T,
 * b = -g_c + W V*^-1 g_p) solved by conjugate gradients instead of a dense Cholesky factorisation.  S* is applied
 * matrix-free and never formed; the preconditioner is block Jacobi on S*'s 6 x 6 diagonal blocks, each factored by
 * Cholesky (a block or a V_p* that does not factor is a rejected step).  CG starts from dc = 0 and stops at the first of
 * |r_k| <= cg_tolerance |b|, k = max_cg_iterations, or a breakdown (p^T S* p <= 0 or a non-finite scalar: the iterate
 * reached so far is the step; at k = 0 the step is rejected).  The host reads two flags from the device once per LM step
 * and once per 10 CG iterations to stop enqueuing work, so the call synchronises `stream`; the result does not depend on
 * those reads, and a call is bit-reproducible.  Arguments as sfm_bundle_adjust, with no camera limit, plus
 * max_cg_iterations >= 1 and cg_tolerance finite in (0, 1); the workspace is at least sfm_bundle_pcg_workspace_bytes. */
int sfm_bundle_adjust_pcg(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                          const double* poses_in, const double* points_in, const int32_t* camera_index,
                          const int32_t* point_index, const double* pixels, int max_steps, int max_cg_iterations,
                          double cg_tolerance, double* poses_out, double* points_out, sfm_bundle_pcg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ---- robust losses of both bundle adjusters (csrc/sfm_loss.h; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_BUNDLE_LOSS_SQUARED 0 /* rho(e) = e */
#define SFM_BUNDLE_LOSS_HUBER 1   /* rho(e) = e for e <= a^2, else 2 a sqrt(e) - a^2 */
#define SFM_BUNDLE_LOSS_CAUCHY 2  /* rho(e) = a^2 log1p(e / a^2) */

typedef struct sfm_bundle_options {
    int32_t loss;      /* SFM_BUNDLE_LOSS_* */
    int32_t reserved;  /* 0 */
    double loss_scale; /* a, in pixels: positive, a * a a normal finite double, about 1.5e-154 .. 1.3e154 (read and checked
                          for the squared loss too, where it has no effect) */
} sfm_bundle_options;

/* sfm_bundle_adjust and sfm_bundle_adjust_pcg on F = sum over the observations of rho(e), e the squared reprojection error
 * in px^2: initial_cost, final_cost, the accept test, the relative-decrease stop and SFM_BUNDLE_BAD_START all use this F
 * (rho(+inf) = +inf).  The linearisation is iteratively reweighted least squares in its first-order form: the residual and
 * both Jacobians of an observation are multiplied by sqrt(w), w = rho'(e) at the linearisation point (1 | a / sqrt(e) above
 * a^2 | 1 / (1 + e / a^2)); everything else is the squared adjuster's.  options == NULL is the squared loss, and a squared
 * call computes the bits of the entry point without options.  SFM_EINVAL before the first launch for a loss outside 0..2,
 * reserved != 0 or a loss_scale that is not positive with a normal finite square (a^2 is computed in double: at 0 or inf
 * Cauchy's rho would be NaN for every e).  Within that range rho is +inf where e / a^2 overflows, and the start is then
 * SFM_BUNDLE_BAD_START, as for a point behind a camera.  The dense adjuster's workspace is
 * sfm_bundle_workspace_bytes for every loss; the iterative one keeps sqrt(w) per observation for a non-squared loss and
 * needs sfm_bundle_pcg_workspace_bytes_ex (-1 also for options it refuses; the plain size for NULL or squared). */
int sfm_bundle_adjust_ex(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                         const double* poses_in, const double* points_in, const int32_t* camera_index,
                         const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                         double* points_out, sfm_bundle_info* info, void* workspace, int64_t workspace_bytes, void* stream,
                         const sfm_bundle_options* options);
int64_t sfm_bundle_pcg_workspace_bytes_ex(int64_t cameras, int64_t points, int64_t observations,
                                          const sfm_bundle_options* options);
/* As sfm_bundle_adjust_pcg, the host reads the two stop flags between LM steps and CG chunks: the call synchronises `stream`. */
int sfm_bundle_adjust_pcg_ex(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                             const double* poses_in, const double* points_in, const int32_t* camera_index,
                             const int32_t* point_index, const double* pixels, int max_steps, int max_cg_iterations,
                             double cg_tolerance, double* poses_out, double* points_out, sfm_bundle_pcg_info* info,
                             void* workspace, int64_t workspace_bytes, void* stream, const sfm_bundle_options* options);

/* ---- shared intrinsics refined by the dense bundle adjuster (csrc/sfm_bundle.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_BUNDLE_REFINE_FOCAL 1           /* f = K[0,0] */
#define SFM_BUNDLE_REFINE_PRINCIPAL_POINT 2 /* cx = K[0,2] and cy = K[1,2], free or held together */

typedef struct sfm_bundle_calibration_options {
    sfm_bundle_options loss; /* as for sfm_bundle_adjust_ex */
    int32_t refine;          /* SFM_BUNDLE_REFINE_* bits, at least one */
    int32_t reserved;        /* 0 */
} sfm_bundle_calibration_options;

/* Bytes of workspace sfm_bundle_adjust_calibrated needs (at least sfm_bundle_workspace_bytes); -1 for sizes it refuses. */
int64_t sfm_bundle_calibrated_workspace_bytes(int64_t cameras, int64_t points, int64_t observations);

/* sfm_bundle_adjust_ex with up to three more unknowns theta = (f, cx, cy), shared by all cameras.  A step (df, dcx, dcy)
 * gives K[0,0] <- f + df, multiplies K[0,1], K[1,0] and K[1,1] by (f + df) / f (the 2 x 2 block keeps its shape and a zero
 * entry stays exactly zero) and adds (dcx, dcy) to (K[0,2], K[1,2]); an intrinsic whose bit is not set in options->refine is
 * held.  F is the cost of sfm_bundle_adjust_ex under the current K.  With w the projection, the rows of the new Jacobian
 * block are dw/df = ((w_0 - K[0,2]) / K[0,0], (w_1 - K[1,2]) / K[0,0]), dw/dcx = (1, 0), dw/dcy = (0, 1), multiplied by
 * sqrt(w) under a robust loss as the others are.  Its normal-equation blocks are summed over every observation in front of
 * its camera, those of fixed cameras and of held points included, and after the Schur complement on the points they border
 * the reduced camera system with 1 to 3 rows, damped by lambda diag as every other block.  A trial K[0,0] that is not finite,
 * is zero or differs in sign from the input's is a rejected step.  The intrinsics' step counts into |delta| and the free
 * intrinsics into |x| of the small-step stop; the gauge similarity does not touch them.  The whole call is enqueued at once,
 * the refined camera matrix is written by its last launch, and a call is bit-reproducible.
 * K_out: dev [9], row 2 (0, 0, 1); for SFM_BUNDLE_BAD_START and SFM_BUNDLE_BAD_INDEX the input K.  options: not NULL.
 * SFM_EINVAL before the first launch for a refine outside 1..3, reserved != 0, loss options sfm_bundle_adjust_ex refuses,
 * K[0,0] == 0 with SFM_BUNDLE_REFINE_FOCAL, and everything else sfm_bundle_adjust_ex refuses.  The workspace is at least
 * sfm_bundle_calibrated_workspace_bytes.  The other arguments as sfm_bundle_adjust_ex. */
int sfm_bundle_adjust_calibrated(const double* K, int64_t cameras, int64_t points, int64_t observations, const uint8_t* fixed,
                                 const double* poses_in, const double* points_in, const int32_t* camera_index,
                                 const int32_t* point_index, const double* pixels, int max_steps, double* poses_out,
                                 double* points_out, sfm_bundle_info* info, double* K_out, void* workspace,
                                 int64_t workspace_bytes, void* stream, const sfm_bundle_calibration_options* options);

/* ---- triangulation of multi-view tracks (csrc/sfm_tracks.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 14 without a version change: they are new, and nothing an ABI-14 caller uses changed. */

#define SFM_TRACKS_OK 0
#define SFM_TRACKS_FEW_VIEWS 1   /* fewer than min_views observations: point, angle and errors NaN */
#define SFM_TRACKS_DEGENERATE 2  /* every observation names one camera, or the unit null vector is not finite or |v3| <= 1e-12:
                                  * point, angle and errors NaN */
#define SFM_TRACKS_BEHIND 3      /* behind a camera of one of its observations (the estimate is written) */
#define SFM_TRACKS_SMALL_ANGLE 4 /* triangulation angle below min_angle (the estimate is written) */
#define SFM_TRACKS_LARGE_ERROR 5 /* an observation's squared reprojection error above max_error (the estimate is written) */
#define SFM_TRACKS_BAD_INDEX 6   /* some camera or point index of the call is out of range: every output NaN */

typedef struct sfm_tracks_info {
    int64_t status;                 /* 0, or 1 when an index is out of range (every point SFM_TRACKS_BAD_INDEX) */
    int64_t points_ok;              /* points with SFM_TRACKS_OK */
    int64_t max_refine_steps_taken; /* the most Levenberg-Marquardt trial steps of any point */
    int64_t reserved;               /* 0 */
} sfm_tracks_info;

/* Bytes of workspace sfm_triangulate_tracks needs; -1 for sizes it refuses. */
int64_t sfm_tracks_workspace_bytes(int64_t points, int64_t observations);

/* Every point p from its observations m (point_index[m] == p, in increasing m; any order of the observations): the N-view
 * DLT of the reference's two-view rows (y P3 - P2, P1 - x P3 with P = K [R | t] of camera camera_index[m], pixels[m] = (x, y)),
 * X = v[0:3] / v[3] for v the right singular vector of the smallest singular value.  refine_steps > 0: then Levenberg-Marquardt
 * on the point alone on F = sum of sfm_pnp_score's e over its observations, with the rules of sfm_pnp_refine (a rank-deficient
 * start or a non-finite F skips it).  At the final X: obs_error[m] = e_m, the cheirality, and the angle
 * acos(min over pairs i < j of d_i . d_j) of the unit rays d from the camera centres -R^T t; the status is the first failing
 * rule of SFM_TRACKS_*.  Deterministic, bit for bit, from run to run.
 * K: host [9], row 2 (0, 0, 1); poses: dev [cameras,12] (R | t, world -> camera); camera_index, point_index: dev int32
 * [observations]; pixels: dev [observations,2]; min_views >= 2; min_angle (radians) finite and >= 0; max_error (px^2) >= 0,
 * may be +inf; refine_steps >= 0; points_out: dev [points,3]; status: dev uint8 [points]; obs_error: dev [observations] or
 * NULL; angle: dev [points] (radians) or NULL; info: dev, one record; workspace: dev, 16-byte aligned, at least
 * sfm_tracks_workspace_bytes.  cameras, observations < 2^31, points < 2^31 - 1. */
int sfm_triangulate_tracks(const double* K, int64_t cameras, int64_t points, int64_t observations, const double* poses,
                           const int32_t* camera_index, const int32_t* point_index, const double* pixels, int min_views,
                           double min_angle, double max_error, int refine_steps, double* points_out, uint8_t* status,
                           double* obs_error, double* angle, sfm_tracks_info* info, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ---- outlier-robust triangulation of multi-view tracks (csrc/sfm_tracks_robust.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_TRACKS_NO_CONSENSUS 7 /* sfm_triangulate_tracks_robust only: no valid hypothesis, or fewer than min_views inliers,
                                   * or inliers of one camera only: point, angle and errors NaN, no flags */

typedef struct sfm_tracks_robust_info {
    int64_t status;                 /* 0, or 1 when an index is out of range (every point SFM_TRACKS_BAD_INDEX) */
    int64_t points_ok;              /* points with SFM_TRACKS_OK */
    int64_t max_refine_steps_taken; /* the most Levenberg-Marquardt trial steps of any point */
    int64_t inlier_observations;    /* the inlier flags set on points with SFM_TRACKS_OK */
    int64_t hypotheses;             /* valid hypotheses scored, summed over the points */
    int64_t reserved;               /* 0 */
} sfm_tracks_robust_info;

/* Bytes of workspace sfm_triangulate_tracks_robust needs; -1 for sizes it refuses. */
int64_t sfm_tracks_robust_workspace_bytes(int64_t points, int64_t observations);

/* sfm_triangulate_tracks for tracks that hold wrong observations: per-track RANSAC (the definition is
 * tests/robust_tracks_oracle.py).  Point p has the observations o_0 .. o_{k-1} in increasing observation index.  An index out of
 * range, fewer than min_views observations and a track of one camera give SFM_TRACKS_BAD_INDEX, _FEW_VIEWS and _DEGENERATE as
 * there.  Otherwise, with T = k (k - 1) / 2 and H = min(T, max_hypotheses), hypothesis h is the pair i < j of rank r_h in
 * lexicographic order, r_h = h when T <= max_hypotheses and h (T div max_hypotheses) + min(h, T mod max_hypotheses) otherwise
 * (no random numbers).  It is valid when its two cameras differ, its two-view DLT (the four rows above, i then j) gives a
 * finite unit null vector with |v3| > 1e-12, the point lies in front of both cameras and their two rays open at least
 * min_angle.  A valid hypothesis scores n = the observations of the track with e <= max_error (sfm_pnp_score's e) and c = the
 * sum of min(e, max_error) in run order; the winner has the largest n, then the smallest c, then the smallest h.  No valid
 * hypothesis, or n < min_views, gives SFM_TRACKS_NO_CONSENSUS, and so does a winner whose inliers name one camera.  The point
 * is then sfm_triangulate_tracks's N-view DLT and optional Levenberg-Marquardt over the winner's inliers only (a bad null
 * vector: SFM_TRACKS_DEGENERATE).  At the final X: obs_error[m] = e_m for every observation of the track, inlier[m] =
 * e_m <= max_error; fewer than min_views inliers, or inliers of one camera, give SFM_TRACKS_NO_CONSENSUS; the angle is taken
 * over the pairs of final inliers, below min_angle gives SFM_TRACKS_SMALL_ANGLE, else SFM_TRACKS_OK.  SFM_TRACKS_BEHIND and
 * _LARGE_ERROR do not occur.  OK and SMALL_ANGLE write the estimate, the angle, the errors and the flags; every other status
 * writes NaN and no flags.  Deterministic, bit for bit, from run to run and under any permutation of the observations that
 * keeps each point's own order.
 * Arguments as sfm_triangulate_tracks, except: max_error (px^2) finite and >= 0; max_hypotheses in 1 .. 1024; inlier: dev
 * uint8 [observations]; workspace at least sfm_tracks_robust_workspace_bytes. */
int sfm_triangulate_tracks_robust(const double* K, int64_t cameras, int64_t points, int64_t observations, const double* poses,
                                  const int32_t* camera_index, const int32_t* point_index, const double* pixels,
                                  int min_views, double min_angle, double max_error, int refine_steps, int max_hypotheses,
                                  double* points_out, uint8_t* status, double* obs_error, uint8_t* inlier, double* angle,
                                  sfm_tracks_robust_info* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- multi-view tracks from pairwise matches (csrc/sfm_track_build.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_BUILD_OK 0        /* the feature belongs to a track */
#define SFM_BUILD_UNMATCHED 1 /* no match touches the feature */
#define SFM_BUILD_CONFLICT 2  /* its component holds two features of one image: the whole component is dropped */
#define SFM_BUILD_BAD_INDEX 3 /* some input of the call is out of range: every feature, no observations */

typedef struct sfm_build_tracks_info {
    int64_t status;       /* 0; 1 an input out of range (every feature SFM_BUILD_BAD_INDEX); 2 a bounded device loop gave up
                             (every other output undefined) */
    int64_t components;   /* components of two or more features */
    int64_t tracks;       /* OK components */
    int64_t observations; /* M: features of OK components */
    int64_t conflicts;    /* conflict components */
    int64_t unmatched;    /* features no match touches */
} sfm_build_tracks_info;

/* Bytes of workspace sfm_build_tracks needs; -1 for sizes it refuses. */
int64_t sfm_build_tracks_workspace_bytes(int64_t images, int64_t features, int64_t matches);

/* Tracks from the matches of image pairs.  Image i has features image_offset[i] .. image_offset[i + 1] (global ids,
 * image-major; image_offset[0] = 0, image_offset[images] = features, non-decreasing).  Pair q joins images
 * pair_images[2q] != pair_images[2q + 1]; its matches are match_offset[q] .. match_offset[q + 1] (match_offset[0] = 0,
 * match_offset[pairs] = matches, non-decreasing), each the local indices (a, b) = match_index[2m], match_index[2m + 1] in the
 * pair's two images.  Duplicate matches and duplicate or reversed pairs are allowed.  Outputs, every one a function of the
 * multiset of matches alone: component[g] the smallest global id of g's connected component (may be NULL); status[g]
 * (SFM_BUILD_*); the OK components are the tracks, numbered in increasing component id, track[g] = g's track or -1; the M
 * observations of the tracks by track and, inside a track, by global id: camera_index (the image), point_index (the track),
 * feature_index (the global id), each of capacity `features`, entries M .. features - 1 set to -1.  An input out of range
 * gives info.status 1.  No host synchronisation; deterministic, bit for bit.
 * image_offset: dev int32 [images + 1]; pair_images: dev int32 [pairs, 2]; match_offset: dev int32 [pairs + 1]; match_index:
 * dev int32 [matches, 2]; component, track, camera_index, point_index, feature_index: dev int32 [features]; status: dev
 * uint8 [features]; info: dev, one record; workspace: dev, 16-byte aligned, at least sfm_build_tracks_workspace_bytes.
 * images, features, pairs < 2^31 - 1, matches < 2^31. */
int sfm_build_tracks(int64_t images, int64_t features, int64_t pairs, int64_t matches, const int32_t* image_offset,
                     const int32_t* pair_images, const int32_t* match_offset, const int32_t* match_index, int32_t* component,
                     int32_t* track, uint8_t* status, int32_t* camera_index, int32_t* point_index, int32_t* feature_index,
                     sfm_build_tracks_info* info, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- rotation averaging over a view graph (csrc/sfm_rotation_averaging.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_ROTAVG_CONVERGED 0 /* the largest |x_c|_inf of a step was <= step_tolerance, or there is no free camera */
#define SFM_ROTAVG_MAX_STEPS 1 /* max_steps steps were taken (max_steps = 0: the initialisation is the result) */
#define SFM_ROTAVG_CG_FAILED 2 /* a step's CG broke down at k = 0 or met a non-finite scalar: the rotations of the last
                                * completed step are the result */
#define SFM_ROTAVG_BAD_INDEX 3 /* a camera index out of range or a self-pair: every rotation and residual NaN */

#define SFM_ROTAVG_INIT_TREE 0  /* start from the maximum-weight breadth-first spanning tree of the root */
#define SFM_ROTAVG_INIT_GIVEN 1 /* start from `initial` (the root keeps its given rotation and is held) */

typedef struct sfm_rotavg_options {
    int32_t loss;              /* SFM_BUNDLE_LOSS_*: rho of e = |log(R_j^T R_q R_i)|^2 in rad^2 */
    int32_t init;              /* SFM_ROTAVG_INIT_* */
    int32_t max_steps;         /* >= 0 */
    int32_t max_cg_iterations; /* >= 1 */
    double loss_scale;         /* a, in radians: positive with a normal finite square, as sfm_bundle_options.loss_scale */
    double cg_tolerance;       /* finite, in (0, 1) */
    double step_tolerance;     /* finite and positive, radians */
} sfm_rotavg_options;

typedef struct sfm_rotavg_info {
    double initial_cost;   /* sum over the used edges of w rho(e) at the initialisation (NaN for SFM_ROTAVG_BAD_INDEX) */
    double final_cost;     /* ... at the result */
    int32_t steps;         /* completed steps */
    int32_t status;        /* SFM_ROTAVG_* */
    int32_t cg_iterations; /* conjugate-gradient iterations over all steps */
    int32_t cg_max;        /* the most conjugate-gradient iterations of one step */
    int32_t registered;    /* cameras with a level, the root included */
    int32_t rounds;        /* the largest level */
} sfm_rotavg_info;

/* Bytes of workspace sfm_average_rotations needs; -1 for sizes it refuses (cameras < 1, cameras >= 2^31, edges < 0 or
 * edges >= 2^30). */
int64_t sfm_average_rotations_workspace_bytes(int64_t cameras, int64_t edges);

/* One absolute rotation per camera (world -> camera) that agrees with the relative rotations of all edges at once:
 * edge q joins cameras i = pairs[2q] != j = pairs[2q + 1] with R_q ~ R_j R_i^T (x_j ~ R_q x_i, the convention of
 * sfm_pair_pose.R) and weight w_q.  An edge is active iff w_q is finite and > 0 and the nine entries of R_q are finite; an
 * inactive edge is ignored and its residual is NaN.  Parallel edges and either orientation are allowed.
 * Levels: level[root] = 0; in round k a camera without a level that has an active edge to a camera of level < k takes level
 * k (with SFM_ROTAVG_INIT_TREE: and its rotation through the heaviest such edge, ties to the earliest half-edge 2q / 2q + 1 of
 * the camera in increasing index, R_root = I).  A camera that never gets a level is unregistered: rotation NaN, registered 0.
 * Then at most max_steps steps of iteratively reweighted Gauss-Newton: per used edge (active, both ends registered)
 * D = R_j^T (R_q R_i), r = log D, e = |r|^2, omega = w rho'(e); the weighted graph Laplacian system
 * sum_{q at c} omega (x_c - x_other) = sum_{q at c} s omega r (s = +1 at the j end, -1 at the i end; x_root = 0) is solved by
 * conjugate gradients with the Jacobi preconditioner from x = 0, stopping as sfm_bundle_adjust_pcg's CG does, and
 * R_c <- R_c exp([x_c]x).  The stop rules are the SFM_ROTAVG_* statuses.  residual[q] = |log D| in radians for a used edge.
 * Every sum runs in an order fixed by the edge list alone and there are no floating-point atomics: a call is reproducible
 * bit for bit.  The host reads three flags between batches of level rounds, steps and chunks of 10 CG iterations, so the
 * call synchronises `stream`; the result does not depend on those reads.  Every byte of every output is written whatever
 * the status.  The definition, operation by operation, is tests/rotation_averaging_oracle.py.
 * pairs: dev int32 [edges,2]; relative: dev [edges,9]; weights: dev [edges]; 0 <= root < cameras; initial: dev [cameras,9],
 * read with SFM_ROTAVG_INIT_GIVEN only (else may be NULL); rotations: dev [cameras,9]; registered: dev uint8 [cameras];
 * level: dev int32 [cameras] or NULL, -1 for an unregistered camera (and for every camera after SFM_ROTAVG_BAD_INDEX);
 * residual: dev [edges]; info: dev, one record; workspace: dev, 16-byte aligned, at least
 * sfm_average_rotations_workspace_bytes.  SFM_EINVAL before the first launch for a refused size, pointer or option. */
int sfm_average_rotations(int64_t cameras, int64_t edges, const int32_t* pairs, const double* relative,
                          const double* weights, int64_t root, const double* initial, const sfm_rotavg_options* options,
                          double* rotations, uint8_t* registered, int32_t* level, double* residual, sfm_rotavg_info* info,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ---- translation averaging over a view graph (csrc/sfm_translation_averaging.hip; an extension, off unless asked for) ----
 * These symbols were added under ABI 15 without a version change: they are new, and nothing an ABI-15 caller uses changed. */

#define SFM_TRANSAVG_CONVERGED 0 /* the largest |x_c|_inf of a step after the warm-up was <= step_tolerance, or no free camera */
#define SFM_TRANSAVG_MAX_STEPS 1 /* max_steps steps were taken (max_steps = 0: the initialisation is the result) */
#define SFM_TRANSAVG_CG_FAILED 2 /* a step's CG broke down at k = 0 or met a non-finite scalar: the positions of the last
                                  * completed step are the result */
#define SFM_TRANSAVG_BAD_INDEX 3 /* a camera index out of range or a self-pair: every position, residual and scale NaN */

#define SFM_TRANSAVG_INIT_TREE 0  /* start from the maximum-weight breadth-first spanning tree of the root, c_root = 0 */
#define SFM_TRANSAVG_INIT_GIVEN 1 /* start from `initial` (the root keeps its given position and is held) */

typedef struct sfm_transavg_options {
    int32_t loss;              /* SFM_BUNDLE_LOSS_*: rho of e = |d (c_j - c_i) - v|^2, at the best d the squared sine of the angle */
    int32_t init;              /* SFM_TRANSAVG_INIT_* */
    int32_t max_steps;         /* >= 0 */
    int32_t max_cg_iterations; /* >= 1 */
    int32_t warmup_steps;      /* >= 0: the first steps take every scale d = 1 and do not end the call as converged */
    int32_t reserved;          /* 0 */
    double loss_scale;         /* a, a sine: positive with a normal finite square, as sfm_bundle_options.loss_scale */
    double cg_tolerance;       /* finite, in (0, 1) */
    double step_tolerance;     /* finite and positive, in the unit of the positions */
} sfm_transavg_options;

typedef struct sfm_transavg_info {
    double initial_cost;   /* sum over the used edges of w rho(e) at the first linearisation (NaN for SFM_TRANSAVG_BAD_INDEX) */
    double final_cost;     /* ... at the result, with the best scales */
    int32_t steps;         /* completed steps */
    int32_t status;        /* SFM_TRANSAVG_* */
    int32_t cg_iterations; /* conjugate-gradient iterations over all steps */
    int32_t cg_max;        /* the most conjugate-gradient iterations of one step */
    int32_t registered;    /* cameras with a level, the root included */
    int32_t rounds;        /* the largest level */
} sfm_transavg_info;

/* Bytes of workspace sfm_average_translations needs; -1 for sizes it refuses (cameras < 1, cameras >= 2^31, edges < 0 or
 * edges >= 2^30). */
int64_t sfm_average_translations_workspace_bytes(int64_t cameras, int64_t edges);

/* One position (camera centre) per camera from one world direction per edge: edge q joins cameras i = pairs[2q] !=
 * j = pairs[2q + 1] with the unit vector v_q ~ c_j - c_i and the weight w_q.  rotations == NULL: directions holds v_q.
 * Otherwise directions holds t_q of x_j ~ R_q x_i + t_q (sfm_pair_pose.t) and rotations the global world -> camera rotations
 * (the result of sfm_average_rotations), and v_q = -(R_j^T t_q) / |t_q| is computed on the device.  An edge is active iff w_q
 * is finite and > 0, v_q (or t_q and the nine entries of R_j) is finite and |t_q| > 0; an inactive edge is ignored, its
 * residual and scale are NaN.  Parallel edges and either orientation are allowed.  Levels and registration as
 * sfm_average_rotations; with SFM_TRANSAVG_INIT_TREE c_root = 0 and a camera's start is its tree parent's position + v_q at
 * the j end, - v_q at the i end, so the unit of the result is one tree baseline.
 * Then at most max_steps steps on sum w rho(|d_q Delta_q - v_q|^2), Delta_q = c_j - c_i, d_q >= 0 (Zhuang, Cheong and Lee,
 * CVPR 2018): d_q = max(<Delta_q, v_q>, 0) / |Delta_q|^2 (0 for Delta_q = 0; 1 in the first warmup_steps steps),
 * r_q = v_q - d_q Delta_q, omega_q = w_q rho'(|r_q|^2), and the weighted graph Laplacian system
 * sum_{q at c} omega d^2 (x_c - x_other) = sum_{q at c} s omega d^2 (r / d) (s = +1 at the j end, -1 at the i end; x_root = 0; an
 * edge with d = 0 adds nothing, a camera whose row is zero takes a zero step) is solved by conjugate gradients as in
 * sfm_average_rotations; c <- c + x.  The stop rules are the SFM_TRANSAVG_* statuses.  residual[q] is the angle between
 * Delta_q and v_q in radians (0..pi) and scale[q] = d_q for a used edge.  Reproducible bit for bit; the call synchronises
 * `stream`; every byte of every output is written whatever the status.  The definition, operation by operation, is
 * tests/translation_averaging_oracle.py.
 * pairs: dev int32 [edges,2]; directions: dev [edges,3]; rotations: dev [cameras,9] or NULL; weights: dev [edges];
 * 0 <= root < cameras; initial: dev [cameras,3], read with SFM_TRANSAVG_INIT_GIVEN only (else may be NULL); positions: dev
 * [cameras,3]; registered: dev uint8 [cameras]; level: dev int32 [cameras] or NULL; residual, scale: dev [edges]; info: dev,
 * one record; workspace: dev, 16-byte aligned, at least sfm_average_translations_workspace_bytes.  SFM_EINVAL before the
 * first launch for a refused size, pointer or option. */
int sfm_average_translations(int64_t cameras, int64_t edges, const int32_t* pairs, const double* directions,
                             const double* rotations, const double* weights, int64_t root, const double* initial,
                             const sfm_transavg_options* options, double* positions, uint8_t* registered, int32_t* level,
                             double* residual, double* scale, sfm_transavg_info* info, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* SED of n correspondences under one E (sed.py:7-30).  E: dev [9]; out: dev [n]. */
int sfm_sed_values(const double* corr, int64_t n, const double* E, double* out, void* stream);

/* Cheirality test of m normalised correspondences under `poses` candidate poses
 * (eight_point.py:449-488).  pose_rt: dev [poses,12] rows [R(9) | t(3)]; pass: dev uint8 [poses,m]. */
int sfm_cheirality(const double* corr, int64_t m, const double* pose_rt, int64_t poses,
                   double distance_threshold, uint8_t* pass, void* stream);

/* Linear (DLT) triangulation of m correspondences (triangulation.py:9-39).  P1, P2: dev [12] each
 * (rows 0..2 of the camera matrices, 4 columns); X: dev [m,3]. */
int sfm_triangulate(const double* corr, int64_t m, const double* P1, const double* P2, double* X,
                    void* stream);

/* Decompose an essential matrix into the four candidate poses in the order (R1,t),(R1,-t),(R2,t),(R2,-t)
 * (eight_point.py:245-280, 210-212).  E: dev [batch,9]; pose_rt: dev [batch,4,12];
 * status: dev int32 [batch], 0 ok, 1 = smallest singular value not ~0 (eight_point.py:268-271). */
int sfm_decompose_essential(const double* E, int64_t batch, double* pose_rt, int32_t* status,
                            void* stream);

/* ---- local optimisation of the winner (an extension, the reference has no such step) ---- */

typedef struct sfm_refine_info {
    double error;     /* aggregated error of the model left in E_out (over its `count` inliers) */
    int32_t count;    /* inliers of that model (for an unrefined model: non-zero entries of mask_in) */
    int32_t accepted; /* refits that were accepted (0 = E_out is E_in) */
} sfm_refine_info;

/* Per image pair, up to `iterations` times: refit E on all current inliers with the N-point form of the reference's
 * normalised eight-point pipeline (eight_point.py:308-446 and :163-166 applied to M >= 8 pairs), re-score all n
 * correspondences (sed.py:7-30, sed <= thr), and keep the refit iff it has more inliers, or as many and a lower
 * aggregated error (ransac.py:96-108 over the inliers); stop at the first refit that is not kept, is degenerate
 * (eight_point.py:415-421) or has fewer than 8 inliers to work from.
 * corr: dev [batch,n,4]; E_in: dev [batch,9]; mask_in: dev uint8 [batch,n] (non-zero = inlier, as written by
 * sfm_inlier_mask); err_in: dev [batch] aggregated error of E_in (sfm_select_result.best_err);
 * E_out: dev [batch,9]; mask_out: dev uint8 [batch,n] (1 = inlier; must not alias mask_in); info: dev [batch]. */
int sfm_refine_inliers(const double* corr, int64_t n, int64_t batch, const double* E_in, const uint8_t* mask_in,
                       const double* err_in, double thr, int aggregation, int iterations, double* E_out,
                       uint8_t* mask_out, sfm_refine_info* info, void* stream);

/* ---- batched, device-resident pose selection + triangulation (chains after sfm_inlier_mask) ---- */

/* Cheirality of every correspondence of every pair under its 4 candidate poses.  corr: dev [batch,n,4]
 * (K-normalised); pose_rt: dev [batch,4,12] as written by sfm_decompose_essential; mask: dev uint8
 * [batch,n] inlier mask (points with 0 are reported as failing) or NULL; pass: dev uint8 [batch,4,n]. */
int sfm_cheirality_batched(const double* corr, int64_t n, int64_t batch, const double* pose_rt,
                           const uint8_t* mask, double distance_threshold, uint8_t* pass, void* stream);

/* Pose vote of eight_point.py:213-237 per pair: votes[b,p] = #passing correspondences except the one
 * with index skip_index[b] (the reference does not count position 0 of its list: np.count_nonzero of the
 * index array); best[b] = first maximum, -1 if all votes are 0.  skip_index: dev int32 [batch] or NULL;
 * votes: dev int32 [batch,4]; best: dev int32 [batch]. */
int sfm_pose_vote(const uint8_t* pass, int64_t n, int64_t batch, const int32_t* skip_index, int32_t* votes,
                  int32_t* best, void* stream);

/* Triangulate (triangulation.py:42-62) the correspondences that pass under the chosen pose:
 * P1 = [K|0], P2 = [K|0][R t; 0 1], pixel coordinates.  pix_a, pix_b: dev [batch,n,2]; K: HOST [9]
 * row-major intrinsics; X: dev [batch,n,3] (zeros where valid == 0); valid: dev uint8 [batch,n]. */
int sfm_triangulate_selected(const double* pix_a, const double* pix_b, int64_t n, int64_t batch,
                             const double* K, const double* pose_rt, const int32_t* best,
                             const uint8_t* pass, double* X, uint8_t* valid, void* stream);

/* ---- brute-force window matching (reference lib/feature_matching: matching.py, ncc.py, ssd.py, util.py) ---- */
#define SFM_MATCH_NCC 0 /* ncc.py:7-54: 1 - normalised cross-correlation, in [0,2]; 2.0 if a window leaves the image */
#define SFM_MATCH_SSD 1 /* ssd.py:7-36: mean squared difference; +inf if a window leaves the image */
/* ssd.py:31-36 on INTEGER images: the reference subtracts and squares in the image dtype — both wrap modulo 2^bits, into the
 * signed range for signed types (uint8 images, what apps/sfm.py:222-224 produces: modulo 256) —, np.sum accumulates in
 * int64 / uint64 and the division by the window size is float64.  bits: 8, 16, 32 or 64 (the NumPy result type of
 * image_a - image_b).  The patches then hold the pixels as int64 bit patterns (SFM_PATCH_RAW64).  Bit-exact. */
#define SFM_MATCH_SSD_INT(bits, is_signed) (0x100 | ((is_signed) ? 0x80 : 0) | (bits))

/* patch modes of sfm_patch_extract (its `subtract_mean` argument) */
#define SFM_PATCH_PLAIN 0        /* float64 pixels as they are (SSD on float images) */
#define SFM_PATCH_MEAN_REMOVED 1 /* float64 pixels minus the window mean (ncc.py:33-37) */
#define SFM_PATCH_RAW64 2        /* image holds int64 pixels: 8-byte copies, no arithmetic (SFM_MATCH_SSD_INT) */

/* Windows of n features of one image (util.py:8-27).  image: dev f64 [height,width] (int64 with SFM_PATCH_RAW64);
 * feats: dev f64 [n,2] (x, y); patches: dev f64 [window_size^2][stride] k-major (stride >= n), by `subtract_mean` =
 * SFM_PATCH_PLAIN / SFM_PATCH_MEAN_REMOVED (ncc.py:33-37) / SFM_PATCH_RAW64 (int64 bit patterns in the 8-byte slots);
 * ssq: dev [n] sum of squares of the stored patch (0 with SFM_PATCH_RAW64); ok: dev uint8 [n] window inside the image. */
int sfm_patch_extract(const double* image, int64_t height, int64_t width, const double* feats, int64_t n,
                      int window_size, int subtract_mean, int64_t stride, double* patches, double* ssq,
                      uint8_t* ok, void* stream);

/* scores[a,b] for every pair of features (the score_function calls of matching.py:57-65).
 * metric SFM_MATCH_NCC needs mean-removed patches, SFM_MATCH_SSD_INT(bits, signed) raw int64 ones.  scores: dev f64 [n_a,n_b].
 * Fast path (LDS-DMA staging) when both patch arrays are 16-byte aligned with an even `stride` >= n rounded up to a
 * multiple of 128 (the padding may hold anything); any other layout works through a slower staging loop. */
int sfm_pair_scores(int metric, const double* patches_a, int64_t stride_a, const double* patches_b,
                    int64_t stride_b, const double* ssq_a, const double* ssq_b, const uint8_t* ok_a,
                    const uint8_t* ok_b, int64_t n_a, int64_t n_b, int window_elements, double* scores,
                    void* stream);

/* Per A-feature, what the reference's heapq holds after pushing its row of scores in order
 * (matching.py:60-65): best[a] / arg[a] = heap[0] score and b index (first minimum), second[a] = heap[1]
 * score (the value the ratio test of matching.py:84-97 divides by; NaN if n_b == 1).
 * best, second: dev f64 [n_a]; arg: dev int32 [n_a]. */
int sfm_match_row_summary(const double* scores, int64_t n_a, int64_t n_b, double* best, int32_t* arg,
                          double* second, void* stream);

/* sfm_pair_scores + sfm_match_row_summary in one pass that never materialises the |A| x |B| matrix: each tile of
 * scores is reduced on chip to four numbers per row, a second small kernel walks them in b order.  Same outputs,
 * bit for bit.  workspace: dev, 16-byte aligned, >= sfm_match_summary_workspace_bytes(n_a, n_b) bytes. */
int64_t sfm_match_summary_workspace_bytes(int64_t n_a, int64_t n_b);
int sfm_match_summary(int metric, const double* patches_a, int64_t stride_a, const double* patches_b,
                      int64_t stride_b, const double* ssq_a, const double* ssq_b, const uint8_t* ok_a,
                      const uint8_t* ok_b, int64_t n_a, int64_t n_b, int window_elements, void* workspace,
                      int64_t workspace_bytes, double* best, int32_t* arg, double* second, void* stream);

/* ---- oriented integer BRIEF descriptors and their Hamming matcher (definition: tests/brief_oracle.py) ---- */

/* 256-bit descriptors of n features of a uint8 image, all in integer arithmetic (bit-exact against the NumPy definition).
 * Centre pixel xi = floor(x + 0.5), yi = floor(y + 0.5); a feature is valid iff x, y are finite, 15 <= xi <= width - 16 and
 * 15 <= yi <= height - 16.  Orientation: the intensity moments m10 = sum dx I, m01 = sum dy I over the disc
 * dx^2 + dy^2 <= 225 fall into the angle bin b with cross(B[b-1], m) >= 0 and cross(B[b], m) < 0 (indices mod bins,
 * cross(p, m) = p.x m01 - p.y m10 in int64; m = 0: bin 0).  Bit t = 1 iff the 5 x 5 box sum at centre + (ax, ay) is smaller
 * than the one at centre + (bx, by) for test t of that bin; byte t / 8, bit t % 8.
 * image: dev u8 [height,width]; feats: dev f64 [n,2] (x, y); offsets: dev int8 [bins,256,4] = (ax, ay, bx, by), every
 * coordinate within +-13 (clamped); boundaries: dev int64 [bins,2] = B; 1 <= bins <= 64; desc: dev u8 [n,32], 8-byte aligned;
 * ok, angle_bin: dev u8 [n].  An invalid feature gets an all-zero descriptor, ok = 0, angle_bin = 0. */
int sfm_brief_describe(const uint8_t* image, int64_t height, int64_t width, const double* feats, int64_t n,
                       const int8_t* offsets, const int64_t* boundaries, int bins, uint8_t* desc, uint8_t* ok,
                       uint8_t* angle_bin, void* stream);

/* sfm_match_summary for those descriptors: the score of (a, b) is the Hamming distance of the two 32-byte descriptors as a
 * double, +inf if either is invalid (ok = 0); best / arg / second have exactly the meaning they have there (heap[0] = first
 * minimum in b order, heap[1] of the reference's heapq, NaN if n_b == 1), and the |A| x |B| matrix is never written.
 * desc_a, desc_b: dev u8 [n,32], 16-byte aligned; workspace: dev, 16-byte aligned,
 * >= sfm_hamming_summary_workspace_bytes(n_a, n_b) bytes. */
int64_t sfm_hamming_summary_workspace_bytes(int64_t n_a, int64_t n_b);
int sfm_hamming_summary(const uint8_t* desc_a, const uint8_t* ok_a, int64_t n_a, const uint8_t* desc_b, const uint8_t* ok_b,
                        int64_t n_b, void* workspace, int64_t workspace_bytes, double* best, int32_t* arg, double* second,
                        void* stream);

/* ---- descriptor matching of every image pair of a collection (definition: tests/graph_matching_oracle.py) ---- */

/* (added within ABI 15) How sfm_match_pairs validates a row's nearest column. */
typedef struct sfm_match_pairs_options {
    int32_t max_distance; /* 0..256: a kept match has a Hamming distance of at most this */
    int32_t cross_check;  /* 0 or 1: the row must also be its column's nearest row, and distinctive on that side too */
    int32_t use_ratio;    /* 0 or 1: 0 skips the ratio test */
    int32_t reserved;     /* must be 0 */
    double ratio;         /* finite, > 0 (read only with use_ratio): distance d is distinctive against the runner-up s iff
                             (double)d <= ratio * (double)s */
} sfm_match_pairs_options;

/* Bytes of workspace sfm_match_pairs needs; -1 for sizes it refuses (negative, pairs > 65535, rows or max_image_features
 * >= 2^31). */
int64_t sfm_match_pairs_workspace_bytes(int64_t pairs, int64_t rows, int64_t max_image_features);

/* Matches the 32-byte binary descriptors (sfm_brief_describe's) of every image pair of a collection in one call.  The
 * descriptors of all images lie image-major in desc / ok: image i owns entries image_offset[i] .. image_offset[i + 1] - 1
 * (sfm_build_tracks's image_offset and pair_images).  Pair q = (i, j) has one output row per feature of image i, rows
 * row_offset[q] .. row_offset[q + 1] - 1; its columns are the features of image j.  d(a, b), the Hamming distance, is defined
 * when both descriptors are valid (ok != 0).  For a valid row a: best = the smallest d(a, .), arg = the smallest column that
 * attains it, second = the smallest d(a, b) over valid b != arg (none when there is no such b; a tie for the best gives
 * second == best); the same per column with the roles swapped.  Row a keeps partner[r] = arg, distance[r] = best iff best <=
 * max_distance, best is distinctive against the row's second (always, when there is none or use_ratio is 0) and, with
 * cross_check, a is the arg of column arg and best is distinctive against that column's second.  Every other row gets -1 in
 * both; an invalid descriptor never matches and is nobody's best or second.  All integer but the ratio test: bit-identical
 * to the NumPy definition.
 * pair_status[q] is 1, every row of the pair's span that lies inside [0, rows) is -1 and nothing is read through the pair's
 * indices, when the pair names an image outside [0, images) or twice the same image, an image's offsets leave
 * [0, features] or its size exceeds max_image_features, or the pair's row_offset span is not its first image's size or leaves
 * [0, rows]; otherwise 0.  A row no pair's span holds gets -1.  Every entry of partner, distance and pair_status is written.
 * image_offset: dev int32 [images + 1]; desc: dev u8 [features,32], 16-byte aligned; ok: dev u8 [features]; pair_images: dev
 * int32 [pairs,2]; row_offset: dev int64 [pairs + 1], non-decreasing; partner, distance: dev int32 [rows]; pair_status: dev
 * int32 [pairs]; workspace: dev, 16-byte aligned, at least sfm_match_pairs_workspace_bytes(pairs, rows, max_image_features).
 * SFM_EINVAL before the first launch for a negative size, pairs > 65535, a size >= 2^31, rows without pairs, a null or
 * misaligned pointer, an option out of range, reserved != 0 or a workspace too small. */
int sfm_match_pairs(int64_t images, int64_t features, int64_t pairs, int64_t rows, int64_t max_image_features,
                    const int32_t* image_offset, const uint8_t* desc, const uint8_t* ok, const int32_t* pair_images,
                    const int64_t* row_offset, const sfm_match_pairs_options* options, int32_t* partner, int32_t* distance,
                    int32_t* pair_status, void* workspace, int64_t workspace_bytes, void* stream);

/* (added within ABI 15) Guided matching: sfm_match_pairs restricted to the partners that each pair's verified two-view model
 * admits (definition: tests/guided_matching_oracle.py).  Every argument of sfm_match_pairs keeps its meaning; in addition
 * xy: dev f64 [features,2], the K-normalised coordinates of every feature, image-major like desc; model: dev f64 [pairs,9],
 * row-major; model_kind: dev int32 [pairs], sfm_pair_verdict's codes 0 none, 1 essential, 2 homography; threshold: dev f64
 * [pairs].  For pair q = (i, j), feature a of image i and feature b of image j are admissible iff both are valid and
 * err(a, b) <= threshold[q] (one IEEE compare: false for a NaN error, so a NaN model, coordinate or threshold admits
 * nothing), where err is the symmetric epipolar distance of sfm_sed_values under model q for kind 1 and the symmetric
 * transfer error of sfm_homography_score under model q and its adjugate for kind 2, always with image i's feature first.
 * Kind 0 admits nothing: the pair's rows are -1 and its status 0.  The row summary (best, arg, second) is taken over the
 * admissible columns only and the column summary over the admissible rows only; the keep rule and the outputs are
 * sfm_match_pairs's on those summaries.  With kind 2, the identity matrix, finite coordinates and threshold +inf everything
 * valid is admissible and the outputs are sfm_match_pairs's byte for byte.  Bit-identical to the NumPy definition.
 * pair_status[q] is 1 and the pair's rows are -1, as for a pair sfm_match_pairs refuses, also when model_kind[q] is not 0, 1
 * or 2.  Every entry of partner, distance and pair_status is written.  The workspace is sfm_match_pairs's:
 * sfm_match_pairs_workspace_bytes(pairs, rows, max_image_features).
 * SFM_EINVAL before the first launch for everything sfm_match_pairs refuses, a null xy (with features > 0), model, model_kind
 * or threshold, an xy, model or threshold that is not 8-byte aligned or a model_kind that is not 4-byte aligned. */
int sfm_match_pairs_guided(int64_t images, int64_t features, int64_t pairs, int64_t rows, int64_t max_image_features,
                           const int32_t* image_offset, const uint8_t* desc, const uint8_t* ok, const double* xy,
                           const int32_t* pair_images, const int64_t* row_offset, const double* model, const int32_t* model_kind,
                           const double* threshold, const sfm_match_pairs_options* options, int32_t* partner, int32_t* distance,
                           int32_t* pair_status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- multi-scale FAST keypoints with BRIEF per pyramid level (definition: tests/keypoint_oracle.py) ---- */

/* (added within ABI 15) One plane of the pixel pool of sfm_detect_keypoints: level `level` of image `image`. */
typedef struct sfm_keypoint_plane {
    int32_t image;    /* 0 .. images - 1 */
    int32_t level;    /* 0 .. 11 */
    int32_t height;   /* level 0: the image's; level l + 1: 4 * height_l / 5, at least 48 */
    int32_t width;    /* likewise */
    int64_t offset;   /* of the plane's first pixel in the pool, and of its first entry in both score maps */
    int32_t quota;    /* >= 0: how many of its strongest keypoints the plane is to keep */
    int32_t reserved; /* must be 0 */
} sfm_keypoint_plane;

/* (added within ABI 15) One keypoint candidate: plane = index into the plane table, (x, y) in that plane's pixels. */
typedef struct sfm_keypoint_candidate {
    int32_t plane, x, y, score;
} sfm_keypoint_candidate;

/* Bytes of workspace sfm_detect_keypoints needs for a table of `planes` planes; -1 for a negative count or more than 65535. */
int64_t sfm_detect_keypoints_workspace_bytes(int64_t planes);

/* Pyramid, FAST-9 score, non-maximum suppression, per-plane cutoff, candidate list and BRIEF descriptors of a whole image
 * collection in one submission; all integer, byte-identical to the NumPy definition.
 * The caller has put every image into its level-0 plane of `pool`; the call fills the planes of the levels above: pixel
 * (x, y) of level l + 1 is ((8-fy)((8-fx) I[y0,x0] + fx I[y0,x0+1]) + fy((8-fx) I[y0+1,x0] + fx I[y0+1,x0+1]) + 32) >> 6 of level
 * l with ux = 10 x + 1, x0 = ux >> 3, fx = ux & 7 and the same in y.  score[offset + y * width + x] is the FAST-9 score of the
 * pixel: with centre value p, circle pixel k (radius 3, 16 pixels from (0,-3) clockwise) is brighter iff I_k > p + threshold,
 * darker iff I_k < p - threshold; 9 cyclically contiguous brighter or darker pixels make a corner of score
 * max(sum over the brighter of I_k - p - threshold, sum over the darker of p - I_k - threshold), every other pixel, and every
 * pixel outside 15 <= x <= width - 16, 15 <= y <= height - 16, scores 0.  kept holds the score of every pixel that is positive,
 * larger than its 3 x 3 neighbours before it in raster order and at least as large as those after it (outside the plane: 0), 0
 * elsewhere.  A plane's cutoff is the largest T >= 1 with at least `quota` kept scores >= T, 1 if there are fewer, nothing
 * for quota 0; every kept pixel at or above it becomes a candidate, in no particular slot order.  *counter receives their
 * number; only the first `capacity` slots of candidates, desc, ok and angle_bin are written, and a caller that finds
 * *counter > capacity calls again with that capacity.  Slot i < min(*counter, capacity) holds sfm_brief_describe's descriptor
 * of candidate i on its plane.  The caller sorts by (score descending, y, x) and trims each plane to its quota: ties at the
 * cutoff are the only surplus.
 * plane_table: HOST [planes], in ascending levels, a plane above level 0 after the plane of its image one level down, planes
 * apart in the pool in table order; pool: dev u8 [pool_bytes], pool_bytes < 2^31; offsets, boundaries, bins: as
 * sfm_brief_describe; score, kept: dev u16 [pool_bytes]; counter: dev int32; candidates: dev [capacity], 16-byte aligned;
 * desc: dev u8 [capacity,32], 8-byte aligned; ok, angle_bin: dev u8 [capacity]; workspace: dev, 16-byte aligned, at least
 * sfm_detect_keypoints_workspace_bytes(planes).  planes == 0 only zeroes *counter.
 * SFM_EINVAL before the first launch for a negative or too large size, a threshold outside 1..254, bins outside 1..64,
 * capacity < 1, a null or misaligned pointer, a workspace too small or a table that breaks one of the rules above. */
int sfm_detect_keypoints(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, uint8_t* pool, int64_t pool_bytes,
                         int threshold, const int8_t* offsets, const int64_t* boundaries, int bins, uint16_t* score,
                         uint16_t* kept, int64_t capacity, int32_t* counter, sfm_keypoint_candidate* candidates, uint8_t* desc,
                         uint8_t* ok, uint8_t* angle_bin, void* workspace, int64_t workspace_bytes, void* stream);

/* Bytes of workspace sfm_build_pyramid needs for a table of `planes` planes; -1 for a negative count or more than 65535. */
int64_t sfm_build_pyramid_workspace_bytes(int64_t planes);

/* (added within ABI 15) The pyramid of sfm_detect_keypoints alone: the same table checks, the table's upload and the same
 * launches, so the pool holds the bytes sfm_detect_keypoints leaves there.  The caller has put every image into its level-0
 * plane; the call fills the planes above.  plane_table, planes, images, pool, pool_bytes: as sfm_detect_keypoints (the quotas
 * are checked and not used); workspace: dev, 16-byte aligned, at least sfm_build_pyramid_workspace_bytes(planes).
 * planes == 0 is a no-op.  SFM_EINVAL before the first launch for a negative or too large size, a null or misaligned pointer,
 * a workspace too small or a table that breaks one of the rules of sfm_detect_keypoints. */
int sfm_build_pyramid(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, uint8_t* pool, int64_t pool_bytes,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- sub-pixel refinement of track observations (definition: tests/track_refine_oracle.py) ---- */

/* (added within ABI 15) The statuses of sfm_refine_observations.  Every status but OK returns the integer input position and warp0. */
#define SFM_REFINE_OK 0              /* refined: xy and warp are the final state */
#define SFM_REFINE_REFERENCE 1       /* reference == own index or -1: nothing to align with */
#define SFM_REFINE_BAD_INDEX 2       /* a reference outside [0, M), a plane outside the table or a pixel outside its plane */
#define SFM_REFINE_OUTSIDE 3         /* the template window or a warped sample leaves its plane */
#define SFM_REFINE_FLAT 4            /* a window of constant grey value */
#define SFM_REFINE_SINGULAR 5        /* a pivot of the 6 x 6 system is not positive, or its solution is not finite */
#define SFM_REFINE_DIVERGED 6        /* the position moved further than max_shift from the input */
#define SFM_REFINE_LOW_CORRELATION 7 /* the final correlation is below min_correlation */

/* Bytes of workspace sfm_refine_observations needs for a table of `planes` planes; -1 for a negative count or more than 65535. */
int64_t sfm_refine_observations_workspace_bytes(int64_t planes);

/* (added within ABI 15) Aligns every observation o < observations with its reference observation q = reference[o] by
 * Gauss-Newton on six affine parameters, maximising the normalised correlation between the (2 radius + 1)^2 window around the
 * integer pixel (x[q], y[q]) on plane[q] and the window warped to plane[o]: sample (dx, dy) lies at u = t0 + (A00 dx + A01 dy),
 * v = t1 + (A10 dx + A11 dy), starting from t = (x[o], y[o]), A = warp0[o] = (A00, A01, A10, A11).  Every sample of every
 * iteration needs 1 <= u < W - 2 and 1 <= v < H - 2.  With I the bilinear samples, gx = 0.5 (I(u+1, v) - I(u-1, v)), gy likewise,
 * I0 = I - mean(I), s = sqrt(sum I0^2) and T the template normalised the same way: res = T - I0 / s, the Jacobian rows
 * (gx, gy, gx dx, gx dy, gy dx, gy dy) / s less their column means, H = sum J J^T + 1e-9 trace(H) on the diagonal, H delta =
 * sum J res by Cholesky, t += delta[0..1], A += delta[2..5]; the loop ends after max_iterations solves or when
 * delta0^2 + delta1^2 < min_step^2.  correlation = sum T (I0 / s) at the final state; at or above min_correlation the status is
 * SFM_REFINE_OK and xy, warp are the final t, A.  All arithmetic is fp64 in the order of the definition, which the device
 * equals byte for byte; the order of every window sum is stated there.  Every element of the five outputs is written;
 * correlation is NaN unless the final state was sampled; iterations counts the solves done.
 * plane_table, planes, images, pool, pool_bytes: as sfm_detect_keypoints after it (or sfm_build_pyramid) filled the pool;
 * plane, x, y, reference: dev int32 [observations]; warp0: dev f64 [observations,4]; radius 2..7; max_iterations 1..50;
 * min_step, max_shift > 0 and finite; xy: dev f64 [observations,2], level pixels; warp: dev f64 [observations,4]; correlation:
 * dev f64 [observations]; iterations, status: dev int32 [observations]; workspace: dev, 16-byte aligned, at least
 * sfm_refine_observations_workspace_bytes(planes).  observations == 0 is a no-op.  A wrong index is a status, never a fault.
 * SFM_EINVAL before the first launch for a negative or too large size, a scalar out of range, a null or misaligned pointer, a
 * workspace too small or a table that breaks one of the rules of sfm_detect_keypoints. */
int sfm_refine_observations(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, const uint8_t* pool,
                            int64_t pool_bytes, int64_t observations, const int32_t* plane, const int32_t* x, const int32_t* y,
                            const int32_t* reference, const double* warp0, int radius, int max_iterations, double min_step,
                            double max_shift, double min_correlation, double* xy, double* warp, double* correlation,
                            int32_t* iterations, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Harris corner detector stencils (reference lib/harris/harris_detector.py, lib/common/correlate.py) ---- */

/* Zero-'same' cross-correlation with an odd square kernel (correlate.py:4-39).  image, out: dev f64
 * [height,width]; kernel: dev f64 [kernel_size,kernel_size]. */
int sfm_cross_correlate(const double* image, int64_t height, int64_t width, const double* kernel,
                        int kernel_size, double* out, void* stream);

/* Harris cornerness det(M) - k trace(M)^2 from block sums of the Sobel products (harris_detector.py:57-86).
 * out: dev f64 [out_height,out_width] (the reference uses height/width - round(block_size/2)); entries outside
 * range(height-block_size) x range(width-block_size) are 0; clamp_negative applies harris_detector.py:29. */
int sfm_harris_cornerness(const double* sobel_x, const double* sobel_y, int64_t height, int64_t width,
                          int block_size, double k, int clamp_negative, int64_t out_height, int64_t out_width,
                          double* out, void* stream);

/* 3x3 non-maximum suppression IN PLACE in raster order, with the reference's sequential semantics
 * (harris_detector.py:95-105): a neighbour visited earlier may already be zero.  image: dev f64 [height,width]. */
int sfm_nms_inplace(double* image, int64_t height, int64_t width, void* stream);

/* The same suppression as a parallel fixpoint (fast path): call sfm_nms_round repeatedly on a zero-initialised
 * state array (dev uint8 [height,width]; bits 0-1: 0 unknown, 1 survives, 2 suppressed; bits 4-7 of an unknown pixel:
 * which raster-earlier neighbours are larger; a zero byte: not looked at yet — the first round classifies every pixel
 * from the image, the following ones read state bytes only) until *unresolved (dev int32, zeroed by the caller
 * before each round) stays 0, then sfm_nms_finalize zeroes the suppressed pixels of `image` in place.
 * The number of rounds is the longest chain of strictly increasing raster-earlier neighbours (a handful on natural
 * images); the result is identical to sfm_nms_inplace. */
int sfm_nms_round(const double* image, uint8_t* state, int64_t height, int64_t width, int32_t* unresolved,
                  void* stream);
int sfm_nms_finalize(double* image, const uint8_t* state, int64_t height, int64_t width, void* stream);

/* (flat index, value) of every non-zero (or NaN) element of `image` [count], in no particular order: what the top-k
 * selection of harris_detector.py:32-42 needs from the suppressed cornerness image.  counter: dev int32 [1], receives
 * the number found (may exceed `capacity`; only the first `capacity` slots are written); index: dev int32 [capacity];
 * value: dev f64 [capacity]. */
int sfm_compact_nonzero(const double* image, int64_t count, int32_t capacity, int32_t* counter, int32_t* index,
                        double* value, void* stream);

/* (new, ABI 12) Of the candidates sfm_compact_nonzero left — value / index: dev [capacity], *found: dev int32, the counter it
 * wrote (read on the device: no host round trip in between; min(*found, capacity) candidates are looked at) — those that can be
 * among the m largest values: every candidate at or above the m-th largest (ties included; a NaN of either sign counts as the
 * largest value there is), plus at most the ones that share the m-th's sign, exponent and top twelve mantissa bits.  What
 * np.argsort of harris_detector.py:32-42 needs of a 1080p image is then num_corners + a few pairs instead of 220 000.
 * workspace: dev, 8192 int32 (zeroed by the call).  *counter_out receives the number kept (may exceed capacity_out; only that many slots are written);
 * fewer than m candidates: all are kept. */
int sfm_prune_top(const double* value, const int32_t* index, const int32_t* found, int32_t capacity, int32_t m, void* workspace,
                  int32_t capacity_out, int32_t* counter_out, int32_t* index_out, double* value_out, void* stream);

/* HOST: exact replay of CPython's random.shuffle as used by ransac.py:59-64.  `mt_state` is the 624-word
 * MT19937 state and `*mt_index` its position (random.getstate()[1]); both are advanced.  The cumulative
 * permutation of range(n) is shuffled `iterations` times; S_out[it,:] receives its first 8 entries.  If
 * perm_io != NULL it supplies the starting permutation (n entries) and receives the final one; if
 * snapshot_iteration >= 0 and snapshot != NULL, the permutation after that iteration is stored there. */
int sfm_pyshuffle_table(uint32_t* mt_state, int32_t* mt_index, int64_t n, int64_t iterations,
                        int32_t* S_out, int32_t* perm_io, int64_t snapshot_iteration, int32_t* snapshot);

#ifdef __cplusplus
}
#endif
#endif /* SFM_HIP_H */
