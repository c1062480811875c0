// Refinement of every pair's relative pose on its inliers, chained behind sfm_pair_poses
// (sfm_view_graph_pose.hip) on the buffers that call took and left; off unless asked for.  Per pair with a pose:
// Levenberg-Marquardt on C = sum of the scorer's symmetric epipolar distance (sfm::sed_value under E = [t]x R) over the
// current inlier set, five unknowns (a rotation vector and two tangent directions of the unit translation), then a
// re-score of every item of the pair and the accept rule of the other winner refinements (sfmfit::refit_wins).  The
// first set is re-scored here under the start pose: e_mask is not read, so a sample item that is an outlier stays out.
// The LM constants, the step rules and the 5 x 5 Cholesky solve are those of sfm_lm.h; the rotation update is the
// Rodrigues form of sfmpnp::apply_step.
//
// Two launches whatever the number of pairs, nothing read back:
//   1. pair_refine_fill_kernel  grid-stride: the zeros of the mask, pose_out = pose_in, the info of a pair without a pose
//   2. pair_refine_kernel       one block per pair with a pose, walking its segment with a block stride as
//                               pose_vote_median_kernel and pnp_refine_kernel do.  Each LM step is one fused pass at the
//                               trial pose: C and, in the same pass, H = sum J^T J (15) and g = sum J^T r (5), so an accepted
//                               step already has its next system.  The LM state lives in LDS and only thread 0 changes it;
//                               every branch that contains a barrier depends only on LDS values published behind a
//                               barrier, or on values every thread computes alike, so it is block-uniform.
// No atomics, every sum sfm::block_sum in a fixed order: a call is reproducible bit for bit.  Nothing is indexed through
// an offset table that was refused (every pose then carries SFM_POSE_BAD_OFFSETS and no block reads its segment).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_lm.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

static_assert(sizeof(sfm_pair_refine_info) == 40, "sfm_pair_refine_info layout is part of the ABI");

namespace {

using sfm::block_sum;
using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_stride;

// 255 VGPRs, no scratch (the compiler keeps E and its five derivatives, 108 VGPRs, in registers over the item loop).  A
// 512-thread block would have to fit two waves per SIMD into 256 registers each and spills 12 bytes per lane: 256 it is.
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kUnknowns = 5;
constexpr int kSums = 21;       // H upper triangle (15, row-major) | g (5) | C
constexpr int kMinItems = 6;
constexpr int kModel = 54;      // E (9) | dE/d omega_0..2, dE/d a, dE/d b (5 x 9)
constexpr int kStop = 0, kEvaluate = 1;
constexpr int kFillBlock = 256;

// E = [t]x R, row-major, each entry two products and one subtraction.
SFM_DEVICE void essential_of(const double* R, const double* t, double* E) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[0 + j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[0 + j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[0 + j];
    }
}

// The tangent basis of the unit t, fixed by rule: e the axis of the smallest |t_i| (the first on ties),
// b1 = (t x e) / |t x e|, b2 = t x b1.
SFM_DEVICE void tangent_basis(const double* t, double (&b1)[3], double (&b2)[3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int axis = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double e[3] = {axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0};
    const double c0 = t[1] * e[2] - t[2] * e[1];
    const double c1 = t[2] * e[0] - t[0] * e[2];
    const double c2 = t[0] * e[1] - t[1] * e[0];
    const double n = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    b1[0] = c0 / n;
    b1[1] = c1 / n;
    b1[2] = c2 / n;
    b2[0] = t[1] * b1[2] - t[2] * b1[1];
    b2[1] = t[2] * b1[0] - t[0] * b1[2];
    b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// model = E | the five derivatives of E at pose (R | t): [t]x [e_k]x R for omega_k, [b_k]x R for the tangent directions
// ([e_k]x R is R with its rows recombined, so each is an essential_of of a 3 x 3 or a 3-vector that is already there).
SFM_DEVICE void build_model(const double* pose, double* model) {
    const double* R = pose;
    const double* t = pose + 9;
    essential_of(R, t, model);
    // [e_0]x R = (0; -R2; R1), [e_1]x R = (R2; 0; -R0), [e_2]x R = (-R1; R0; 0), rows R0, R1, R2 of R
    double G[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        G[j] = 0.0;
        G[3 + j] = -R[6 + j];
        G[6 + j] = R[3 + j];
    }
    essential_of(G, t, model + 9);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        G[j] = R[6 + j];
        G[3 + j] = 0.0;
        G[6 + j] = -R[j];
    }
    essential_of(G, t, model + 18);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        G[j] = -R[3 + j];
        G[3 + j] = R[j];
        G[6 + j] = 0.0;
    }
    essential_of(G, t, model + 27);
    double b1[3], b2[3];
    tangent_basis(t, b1, b2);
    essential_of(R, b1, model + 36);
    essential_of(R, b2, model + 45);
}

// trial = the pose `pose` moved by delta = (omega, a, b): R <- exp([omega]x) R (sfmpnp::apply_step's Rodrigues form),
// t <- (t + a b1 + b b2) / |t + a b1 + b b2|.
SFM_DEVICE void apply_delta(const double* pose, const double (&delta)[kUnknowns], double* trial) {
    const double step[6] = {delta[0], delta[1], delta[2], 0.0, 0.0, 0.0};
    double out[12];
    sfmpnp::apply_step(pose, step, out);
    double b1[3], b2[3];
    tangent_basis(pose + 9, b1, b2);
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (pose[9 + k] + delta[3] * b1[k]) + delta[4] * b2[k];
    const double n = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
#pragma unroll
    for (int k = 0; k < 9; ++k) trial[k] = out[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) trial[9 + k] = x[k] / n;
}

// This thread's share of C, H and g over the items of [first, last) with a non-zero mask, at `model` (LDS).  The
// residuals of an item are r / sqrt(da) and r / sqrt(db) with r, da, db as in sfm::sed_value; C sums sed_value itself.
// With D a derivative of E: dr = xb^T D xa, d la = D xa, d lb = D^T xb, and
// d (r / sqrt(d)) = dr / sqrt(d) - r (l . dl) / (d sqrt(d)).
SFM_DEVICE void accumulate(const Corr* __restrict__ corr, int64_t first, int64_t last, const uint8_t* __restrict__ mask,
                           const double* model, double (&a)[kSums]) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) a[j] = 0.0;
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = model[k];
    for (int64_t i = first + threadIdx.x; i < last; i += kThreads) {
        if (!mask[i]) continue;
        const Corr p = corr[i];
        a[kSums - 1] += sfm::sed_value(e, p.xa, p.ya, p.xb, p.yb);
        const double lb0 = (p.xb * e[0] + p.yb * e[3]) + e[6];
        const double lb1 = (p.xb * e[1] + p.yb * e[4]) + e[7];
        const double lb2 = (p.xb * e[2] + p.yb * e[5]) + e[8];
        const double r = (lb0 * p.xa + lb1 * p.ya) + lb2;
        const double la0 = (e[0] * p.xa + e[1] * p.ya) + e[2];
        const double la1 = (e[3] * p.xa + e[4] * p.ya) + e[5];
        const double da = la0 * la0 + la1 * la1;
        const double db = lb0 * lb0 + lb1 * lb1;
        const double ia = 1.0 / sqrt(da), ib = 1.0 / sqrt(db);
        const double ra = r * ia, rb = r * ib;   // the two residuals
        const double ca = ra / da, cb = rb / db; // r / (d sqrt(d))
        double Ja[kUnknowns], Jb[kUnknowns];
#pragma unroll
        for (int k = 0; k < kUnknowns; ++k) {
            const double* D = model + 9 + 9 * k;
            const double v0 = (D[0] * p.xa + D[1] * p.ya) + D[2];
            const double v1 = (D[3] * p.xa + D[4] * p.ya) + D[5];
            const double v2 = (D[6] * p.xa + D[7] * p.ya) + D[8];
            const double dr = (p.xb * v0 + p.yb * v1) + v2;
            const double w0 = (p.xb * D[0] + p.yb * D[3]) + D[6];
            const double w1 = (p.xb * D[1] + p.yb * D[4]) + D[7];
            Ja[k] = dr * ia - ca * (la0 * v0 + la1 * v1);
            Jb[k] = dr * ib - cb * (lb0 * w0 + lb1 * w1);
        }
        int idx = 0;
#pragma unroll
        for (int u = 0; u < kUnknowns; ++u)
#pragma unroll
            for (int c = u; c < kUnknowns; ++c) a[idx++] += Ja[u] * Ja[c] + Jb[u] * Jb[c];
#pragma unroll
        for (int u = 0; u < kUnknowns; ++u) a[15 + u] += Ja[u] * ra + Jb[u] * rb;
    }
}

// Cholesky factor L of H + lambda diag(H), H the upper triangle sys[0..15) in row-major order.  False when a pivot is
// not above rel times its diagonal entry (rel = 0: not positive), or not a number.
SFM_DEVICE bool damped_factor(const double* sys, double lambda, double rel, double (&L)[kUnknowns][kUnknowns]) {
    double A[kUnknowns][kUnknowns];
    int idx = 0;
#pragma unroll
    for (int r = 0; r < kUnknowns; ++r)
#pragma unroll
        for (int c = r; c < kUnknowns; ++c) A[r][c] = A[c][r] = sys[idx++];
#pragma unroll
    for (int i = 0; i < kUnknowns; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    return sfmlm::factor<kUnknowns>(A, rel, L);
}

// Solves (H + lambda diag H) delta = -g.  False when the factorisation fails or delta is not finite.
SFM_DEVICE bool damped_solve(const double* sys, double lambda, double (&delta)[kUnknowns]) {
    double L[kUnknowns][kUnknowns];
    if (!damped_factor(sys, lambda, 0.0, L)) return false;
    const double b[kUnknowns] = {-sys[15], -sys[16], -sys[17], -sys[18], -sys[19]};
    return sfmlm::solve<kUnknowns>(L, b, delta);
}

SFM_DEVICE void write_info(sfm_pair_refine_info* __restrict__ out, double start_error, double error, int start_count, int count,
                           int accepted, int steps, int status) {
    sfm_pair_refine_info r;
    r.start_error = start_error;
    r.error = error;
    r.start_count = start_count;
    r.count = count;
    r.accepted = accepted;
    r.lm_steps = steps;
    r.status = status;
    r.reserved = 0;
    *out = r;
}

// The zeros of the mask, the copy of the pose table and the info of the pairs pair_refine_kernel leaves alone.
__global__ __launch_bounds__(kFillBlock) void pair_refine_fill_kernel(int64_t n_total, int64_t pairs,
                                                                      const sfm_pair_pose* __restrict__ pose_in,
                                                                      sfm_pair_pose* __restrict__ pose_out,
                                                                      uint8_t* __restrict__ mask_out,
                                                                      sfm_pair_refine_info* __restrict__ info) {
    const int64_t stride = (int64_t)gridDim.x * kFillBlock;
    const int64_t start = (int64_t)blockIdx.x * kFillBlock + threadIdx.x;
    for (int64_t i = start; i < n_total; i += stride) mask_out[i] = 0;
    for (int64_t q = start; q < pairs; q += stride) {
        const sfm_pair_pose p = pose_in[q];
        pose_out[q] = p;
        write_info(info + q, NAN, NAN, 0, 0, 0, 0, p.status == SFM_POSE_OK ? SFM_PAIR_REFINE_OK : SFM_PAIR_REFINE_NO_POSE);
    }
}

__global__ __launch_bounds__(kThreads) void pair_refine_kernel(const Corr* __restrict__ corr, int64_t n_total,
                                                               const int64_t* __restrict__ offset,
                                                               const sfm_pair_pose* __restrict__ pose_in, double thr,
                                                               int aggregation, int rounds, int max_steps,
                                                               sfm_pair_pose* __restrict__ pose_out, uint8_t* __restrict__ mask,
                                                               sfm_pair_refine_info* __restrict__ info) {
    __shared__ double part[kWaves * kSums];
    __shared__ double total[kSums];
    __shared__ double sys[kSums];     // H | g | C at the LM point (thread 0)
    __shared__ double best[12];       // the pose kept so far
    __shared__ double pose[12];       // the LM point
    __shared__ double trial[12];      // the pose the next pass evaluates
    __shared__ double model[kModel];  // E and its derivatives at `trial`
    __shared__ int ctl;

    const int64_t q = blockIdx.x;
    if (pose_in[q].status != SFM_POSE_OK) return;   // block-uniform: the fill kernel wrote its record
    // within [0, n_total] whatever the table holds (a table sfm_verify_pairs accepted is)
    int64_t first = offset[q], last = offset[q + 1];
    first = first < 0 ? 0 : (first > n_total ? n_total : first);
    last = last < first ? first : (last > n_total ? n_total : last);
    const int tid = threadIdx.x;

    if (tid < 9) best[tid] = pose_in[q].R[tid];
    else if (tid < 12) best[tid] = pose_in[q].t[tid - 9];
    __syncthreads();
    // the start set: every item of the pair within thr under the start pose.  Every pass maps item first + k to thread
    // k % kThreads, so a thread only ever reads the mask entries it wrote itself.
    double E[9];
    essential_of(best, best + 9, E);
    double c[3] = {0.0, 0.0, 0.0};
    for (int64_t i = first + tid; i < last; i += kThreads) {
        const Corr p = corr[i];
        const double e = sfm::sed_value(E, p.xa, p.ya, p.xb, p.yb);
        const bool in = e <= thr;
        mask[i] = in ? 1 : 0;
        if (in) {
            c[0] += 1.0;
            c[1] += e;
            c[2] += e * e;
        }
    }
    block_sum<3, kThreads>(c, part, total);
    const double start_cnt = total[0];
    const double start_err = sfmfit::aggregate_error(aggregation, (int)start_cnt, total[1], total[2], 0);
    double best_cnt = start_cnt, best_err = start_err;
    int accepted = 0;
    int steps = 0;   // trial steps of every round (thread 0)

    for (int round = 0; round < rounds; ++round) {
        if (!(best_cnt >= (double)kMinItems)) break;   // block-uniform
        __syncthreads();   // total and best were read above
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) trial[k] = pose[k] = best[k];
            build_model(trial, model);
        }
        __syncthreads();
        double a[kSums];
        accumulate(corr, first, last, mask, model, a);
        block_sum<kSums, kThreads>(a, part, total);
        double lambda = sfmlm::kLambda0;
        bool stop = false;
        int round_steps = 0;
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) sys[k] = total[k];
            double L[kUnknowns][kUnknowns];
            stop = !damped_factor(sys, 0.0, sfmlm::kRankFloor, L);
        }
        // LM: thread 0 plans the next trial (or stops), everybody evaluates it, thread 0 accepts or rejects it
        for (;;) {
            if (tid == 0) {
                int next = kStop;
                while (!stop && !sfmlm::exhausted(round_steps, max_steps, lambda)) {
                    ++round_steps;
                    double delta[kUnknowns];
                    if (!damped_solve(sys, lambda, delta)) {
                        lambda = sfmlm::more_damping(lambda);
                        continue;
                    }
                    const double dn = sqrt(((delta[0] * delta[0] + delta[1] * delta[1]) + (delta[2] * delta[2] + delta[3] * delta[3])) +
                                           delta[4] * delta[4]);
                    if (sfmlm::small_step(dn, 1.0)) break;   // |t| = 1
                    apply_delta(pose, delta, trial);
                    build_model(trial, model);
                    next = kEvaluate;
                    break;
                }
                ctl = next;
            }
            __syncthreads();
            if (ctl == kStop) break;   // block-uniform
            accumulate(corr, first, last, mask, model, a);
            block_sum<kSums, kThreads>(a, part, total);
            if (tid == 0) {
                const double c_new = total[kSums - 1], c_old = sys[kSums - 1];
                if (sfmlm::improved(c_new, c_old)) {
#pragma unroll
                    for (int k = 0; k < kSums; ++k) sys[k] = total[k];
#pragma unroll
                    for (int k = 0; k < 12; ++k) pose[k] = trial[k];
                    lambda = sfmlm::less_damping(lambda);
                    stop = sfmlm::converged(c_old, c_new);
                } else {
                    lambda = sfmlm::more_damping(lambda);
                }
            }
        }
        steps += round_steps;
        // re-score every item under the LM result (the pose thread 0 left before the last barrier)
        essential_of(pose, pose + 9, E);
        c[0] = c[1] = c[2] = 0.0;
        for (int64_t i = first + tid; i < last; i += kThreads) {
            const Corr p = corr[i];
            const double e = sfm::sed_value(E, p.xa, p.ya, p.xb, p.yb);
            if (e <= thr) {
                c[0] += 1.0;
                c[1] += e;
                c[2] += e * e;
            }
        }
        block_sum<3, kThreads>(c, part, total);
        const double cnt = total[0];
        const double err = sfmfit::aggregate_error(aggregation, (int)cnt, total[1], total[2], 0);
        if (!sfmfit::refit_wins(cnt, err, best_cnt, best_err)) break;
        for (int64_t i = first + tid; i < last; i += kThreads) {
            const Corr p = corr[i];
            mask[i] = sfm::sed_value(E, p.xa, p.ya, p.xb, p.yb) <= thr ? 1 : 0;
        }
        if (tid < 12) best[tid] = pose[tid];
        if (tid < 9) pose_out[q].R[tid] = pose[tid];
        else if (tid < 12) pose_out[q].t[tid - 9] = pose[tid];
        best_cnt = cnt;
        best_err = err;
        ++accepted;
    }
    if (tid == 0)
        write_info(info + q, start_err, best_err, (int)start_cnt, (int)best_cnt, accepted, steps,
                   start_cnt >= (double)kMinItems ? SFM_PAIR_REFINE_OK : SFM_PAIR_REFINE_TOO_FEW);
}

}  // namespace

extern "C" {

int sfm_refine_pair_poses(const double* corr, int64_t n_total, const int64_t* offset, int64_t pairs, const sfm_pair_pose* pose_in,
                          double thr, int aggregation, int rounds, int max_steps, sfm_pair_pose* pose_out, uint8_t* mask_out,
                          sfm_pair_refine_info* info, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (n_total < 0 || pairs < 0 || rounds < 0 || max_steps < 0) return fail(SFM_EINVAL, "sfm_refine_pair_poses: negative size");
    if (n_total > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_refine_pair_poses: need fewer than 2^31 items");
    if (pairs > 65535) return fail(SFM_EINVAL, "sfm_refine_pair_poses: pairs > 65535");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail(SFM_EINVAL, "sfm_refine_pair_poses: unknown aggregation");
    if (pairs == 0) return SFM_OK;
    if (!offset || !pose_in || !pose_out || !info || (n_total > 0 && (!corr || !mask_out)))
        return fail(SFM_EINVAL, "sfm_refine_pair_poses: null pointer");
    if (pose_in == pose_out) return fail(SFM_EINVAL, "sfm_refine_pair_poses: pose_out must not alias pose_in");
    hipStream_t st = (hipStream_t)stream;
    const int64_t fill = n_total > pairs ? n_total : pairs;
    hipLaunchKernelGGL(pair_refine_fill_kernel, dim3(grid_stride(fill, kFillBlock, 2048)), dim3(kFillBlock), 0, st, n_total, pairs,
                       pose_in, pose_out, mask_out, info);
    hipLaunchKernelGGL(pair_refine_kernel, dim3((unsigned)pairs), dim3(kThreads), 0, st, (const Corr*)corr, n_total, offset, pose_in,
                       thr, aggregation, rounds, max_steps, pose_out, mask_out, info);
    return check_launch("sfm_refine_pair_poses");
}

}  // extern "C"
