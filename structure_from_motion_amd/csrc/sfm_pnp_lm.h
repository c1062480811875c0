// The refinement of one view's PnP winner on its inliers, as the device routine that sfm_pnp_refine (sfm_pnp_refine.hip) and the
// ragged registration of every view (sfm_register_views.hip) both wrap: moved here unchanged from
// sfm_pnp_refine.hip, so that both run the same operations in the same order.  The LM constants, the step rules and the 6 x 6
// Cholesky solve are those of sfm_lm.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_lm.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

namespace sfmpnp {

using sfm::block_sum;

constexpr int kRefineThreads = 512;
constexpr int kThreads = kRefineThreads;
constexpr int kWaves = kThreads / kWave;
constexpr int kSums = 28;  // H upper triangle (21, row-major) | g (6) | C
constexpr int kMinItems = 6;
constexpr int kStop = 0, kEvaluate = 1;

// This thread's share of C, H and g over the items with a non-zero mask, at model m.  e is pnp_score's value; an item
// behind the camera (c2 <= 0) makes C infinite and adds nothing to H or g.  J: the pose rows of sfmpnp::jacobians.
SFM_DEVICE void accumulate(const double* __restrict__ P, int n, const uint8_t* __restrict__ mask, const double m[12],
                           const PnPCamera& k, double (&a)[kSums]) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) a[j] = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        if (!mask[i]) continue;
        const double* q = P + (int64_t)i * kPnPFields;
        const double X = q[0], Y = q[1], Z = q[2], u = q[3], v = q[4];
        a[kSums - 1] += pnp_score(m, k, X, Y, Z, u, v);
        double res[2], J[2][6], Jp[2][3];
        if (!jacobians(m, k, X, Y, Z, J, Jp, res, u, v)) continue;
        int idx = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) a[idx++] += J[0][r] * J[0][c] + J[1][r] * J[1][c];
#pragma unroll
        for (int r = 0; r < 6; ++r) a[21 + r] += J[0][r] * res[0] + J[1][r] * res[1];
    }
}

// Cholesky factor L of H + lambda diag(H), H the upper triangle sys[0..21) in row-major order.  False when a pivot is
// not above rel times its diagonal entry (rel = 0: not positive), or not a number.
SFM_DEVICE bool damped_factor(const double* sys, double lambda, double rel, double (&L)[6][6]) {
    double A[6][6];
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) A[r][c] = A[c][r] = sys[idx++];
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lambda * A[i][i];
    return sfmlm::factor<6>(A, rel, L);
}

// Solves (H + lambda diag H) delta = -g.  False when the factorisation fails or delta is not finite.
SFM_DEVICE bool damped_solve(const double* sys, double lambda, double (&delta)[6]) {
    double L[6][6];
    if (!damped_factor(sys, lambda, 0.0, L)) return false;
    const double b[6] = {-sys[21], -sys[22], -sys[23], -sys[24], -sys[25], -sys[26]};
    return sfmlm::solve<6>(L, b, delta);
}

// The whole refinement of one view by one block of kThreads threads: P its n items, `min` its seed mask (non-zero = inlier; the
// sample items, marked 2 by sfm_pnp_inlier_mask, count as inliers) without item `excluded` (-1: none), model_in its 12 doubles
// and err_in their aggregated error; model_out (12 doubles, may be model_in), mout (n bytes) and info are written.
SFM_DEVICE void refine_view(const double* __restrict__ P, int n, const uint8_t* __restrict__ min, int excluded, const PnPCamera& cam,
                            const double* __restrict__ model_in, double err_in, double thr, int aggregation, int rounds,
                            int max_steps, double* __restrict__ model_out, uint8_t* __restrict__ mout,
                            sfm_pnp_refine_info* __restrict__ info) {
    __shared__ double part[kWaves * kSums];
    __shared__ double total[kSums];
    __shared__ double sys[kSums];  // H | g | C at the LM point (thread 0)
    __shared__ double best[12];    // the model kept so far
    __shared__ double pose[12];    // the LM point
    __shared__ double trial[12];   // the model the next pass evaluates
    __shared__ int ctl;

    const int tid = threadIdx.x;

    // start: the input model and its inliers (sample items, marked 2 by sfm_pnp_inlier_mask, count as inliers).  Every
    // pass maps item i to thread i % kThreads, so a thread only ever reads the mask entries it wrote itself.
    double v1[1] = {0.0};
    for (int i = tid; i < n; i += kThreads) {
        const uint8_t m = (min[i] != 0 && i != excluded) ? 1 : 0;
        mout[i] = m;
        v1[0] += (double)m;
    }
    if (tid < 12) {
        best[tid] = model_in[tid];
        model_out[tid] = best[tid];
    }
    block_sum<1, kThreads>(v1, part, total);
    double best_cnt = total[0];
    double best_err = err_in;
    int accepted = 0;
    int steps = 0;  // trial steps of every round (thread 0)

    for (int round = 0; round < rounds; ++round) {
        if (!(best_cnt >= (double)kMinItems)) break;  // block-uniform
        if (tid < 12) trial[tid] = pose[tid] = best[tid];
        __syncthreads();
        double a[kSums];
        double m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = trial[k];
        accumulate(P, n, mout, m, cam, a);
        block_sum<kSums, kThreads>(a, part, total);
        double lambda = sfmlm::kLambda0;
        bool stop = false;
        int round_steps = 0;
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) sys[k] = total[k];
            double L[6][6];
            stop = !damped_factor(sys, 0.0, sfmlm::kRankFloor, L);
        }
        // LM: thread 0 plans the next trial (or stops), everybody evaluates it, thread 0 accepts or rejects it
        for (;;) {
            if (tid == 0) {
                int next = kStop;
                while (!stop && !sfmlm::exhausted(round_steps, max_steps, lambda)) {
                    ++round_steps;
                    double delta[6];
                    if (!damped_solve(sys, lambda, delta)) {
                        lambda = sfmlm::more_damping(lambda);
                        continue;
                    }
                    const double dn = sqrt(((delta[0] * delta[0] + delta[1] * delta[1]) + (delta[2] * delta[2] + delta[3] * delta[3])) +
                                           (delta[4] * delta[4] + delta[5] * delta[5]));
                    const double tn = sqrt((pose[9] * pose[9] + pose[10] * pose[10]) + pose[11] * pose[11]);
                    if (sfmlm::small_step(dn, tn)) break;
                    apply_step(pose, delta, trial);
                    next = kEvaluate;
                    break;
                }
                ctl = next;
            }
            __syncthreads();
            if (ctl == kStop) break;  // block-uniform
#pragma unroll
            for (int k = 0; k < 12; ++k) m[k] = trial[k];
            accumulate(P, n, mout, m, cam, a);
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
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = pose[k];
        double c[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += kThreads) {
            const double* q = P + (int64_t)i * kPnPFields;
            const double e = pnp_score(m, cam, q[0], q[1], q[2], q[3], q[4]);
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
        for (int i = tid; i < n; i += kThreads) {
            const double* q = P + (int64_t)i * kPnPFields;
            mout[i] = pnp_score(m, cam, q[0], q[1], q[2], q[3], q[4]) <= thr ? 1 : 0;
        }
        if (tid < 12) {
            best[tid] = pose[tid];
            model_out[tid] = pose[tid];
        }
        best_cnt = cnt;
        best_err = err;
        ++accepted;
    }
    if (tid == 0) {
        info->error = best_err;
        info->count = (int32_t)best_cnt;
        info->accepted = accepted;
        info->lm_steps = steps;
        info->reserved = 0;
    }
}


}  // namespace sfmpnp
