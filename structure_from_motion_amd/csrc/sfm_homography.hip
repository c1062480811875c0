// RANSAC homography between two views: the four-point DLT solver of the shared fit kernel
// (sfmmin::minimal_fit_kernel, sfm_minimal_fit.h), symmetric-transfer-error scoring of every hypothesis over every
// correspondence, and the winner's inlier mask; the pass is sfmmin::ransac_pass and the selection sfm_select_best.  The RANSAC
// semantics are those of the other solvers: the four sample items enter the aggregate unconditionally, the other items when
// their error is at most the threshold, the lowest aggregated error among gated hypotheses wins, earliest first, NaN / inf never.
//
// Data item i of batch entry b: corr[b, i] = {xa, ya, xb, yb} in any one unit (the public route passes K-normalised
// coordinates).  Model: H[b, h] = 9 doubles row-major with x_b ~ H x_a, ||H||_F = 1 and det H >= 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_homography.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_for;
using sfmhost::grid_stride;

using sfmhg::adjugate;
using sfmhg::homography_solver;
using sfmhg::kHomographySample;
using sfmhg::transfer_error;

// --------------------------------------------------------------------------------------------------
// Scoring, with the structure of pnp_score_kernel (sfm_pnp.hip): one hypothesis per lane (H and adj(H) in registers), the
// correspondences staged through LDS in tiles that every lane of the block reads at the same address (broadcast).  cnt =
// non-sample items with e <= thr; s1 / s2 = sums of e / e^2 over the four sample items and those survivors (the layout
// sfm_select_best reads).  The tile loop counts every item; the four sample items are then corrected: one that passed the gate
// is taken out of the count (its value is already in the sums), one that did not is added to the sums.  All fp64 with true
// divisions: every value is the NumPy definition's bit for bit and only the summation order differs.  A NaN model gives NaN sums.
// --------------------------------------------------------------------------------------------------
constexpr int kHomographyScoreBlock = 256;
constexpr int kHomographyTile = 512;  // correspondences per tile: 512 x 32 B = 16 KiB of LDS

__global__ __launch_bounds__(kHomographyScoreBlock) void homography_score_kernel(const Corr* __restrict__ corr, int64_t n,
                                                                                 const double* __restrict__ model,
                                                                                 const int32_t* __restrict__ S, int64_t h_count,
                                                                                 double thr, int32_t* __restrict__ cnt,
                                                                                 double* __restrict__ s1, double* __restrict__ s2) {
    __shared__ Corr tile[kHomographyTile];
    const int64_t b = blockIdx.y;
    const int64_t h = (int64_t)blockIdx.x * kHomographyScoreBlock + threadIdx.x;
    const int64_t hc = h < h_count ? h : h_count - 1;  // lanes past the end score a valid hypothesis and store nothing
    const int64_t bh = b * h_count + hc;
    const Corr* P = corr + b * n;
    double m[9], g[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = model[bh * 9 + i];
    adjugate(m, g);
    int c = 0;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t base = 0; base < n; base += kHomographyTile) {
        const int count = (int)(n - base < kHomographyTile ? n - base : kHomographyTile);
        __syncthreads();  // the previous tile has been read by every lane
        for (int i = threadIdx.x; i < count; i += kHomographyScoreBlock) tile[i] = P[base + i];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < count; ++j) {
            const Corr t = tile[j];
            const double e = transfer_error(m, g, t.xa, t.ya, t.xb, t.yb);
            const bool in = e <= thr;
            c += in ? 1 : 0;
            a1 += in ? e : 0.0;
            a2 += in ? e * e : 0.0;
        }
    }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kHomographySample; ++k) {
        const Corr q = P[checked_index(S[bh * 8 + k], n, bad)];
        const double e = transfer_error(m, g, q.xa, q.ya, q.xb, q.yb);
        if (e <= thr) {
            --c;
        } else {
            a1 += e;
            a2 += e * e;
        }
    }
    if (h < h_count) {
        cnt[b * h_count + h] = c;
        s1[b * h_count + h] = a1;
        s2[b * h_count + h] = a2;
    }
}

// mask[b, i] = 2 for the four sample items of the winner, 1 for the other items with e <= thr, 0 otherwise (all 0 when the
// record holds no model).  Grid-stride over the items; every byte of the mask is written.
__global__ void homography_inlier_mask_kernel(const Corr* __restrict__ corr, int64_t n, const double* __restrict__ model,
                                              const int32_t* __restrict__ S, int64_t h_count,
                                              const sfm_select_result* __restrict__ result, double thr, uint8_t* __restrict__ mask) {
    const int64_t b = blockIdx.y;
    const int64_t best = result[b].best_h;
    const bool none = best < 0 || best >= h_count;
    const int64_t bh = b * h_count + (none ? 0 : best);
    const Corr* P = corr + b * n;
    uint8_t* out = mask + b * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (none) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = 0;
        return;
    }
    double m[9], g[9];
    int32_t smp[kHomographySample];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = model[bh * 9 + k];
    adjugate(m, g);
#pragma unroll
    for (int k = 0; k < kHomographySample; ++k) smp[k] = S[bh * 8 + k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const Corr q = P[i];
        const double e = transfer_error(m, g, q.xa, q.ya, q.xb, q.yb);
        bool in_sample = false;
#pragma unroll
        for (int k = 0; k < kHomographySample; ++k) in_sample |= (smp[k] == (int32_t)i);
        out[i] = in_sample ? 2 : ((e <= thr) ? 1 : 0);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// Every check of a call that depends on its sizes, before anything is launched: four items per sample, n at least that, and the
// grids of the fit and scoring launches.
int check_call(const char* fn, int64_t n, int64_t h_count, int64_t batch) {
    return sfmhost::check_sizes(fn, kHomographySample, n, h_count, batch, {kHomographyScoreBlock, sfmmin::kMinimalFitBlock});
}

int launch_fit(bool philox, uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n, int64_t h_count,
               int64_t batch, int32_t* S, double* H, int32_t* flags, hipStream_t st) {
    return sfmmin::launch_minimal_fit<homography_solver>((const Corr*)corr, philox, seed, seed_stride, h_begin, n, h_count, batch, S, H,
                                                       flags, st);
}

int launch_score(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch, double thr,
                 int32_t* cnt, double* s1, double* s2, hipStream_t st) {
    const dim3 grid(grid_for(h_count, kHomographyScoreBlock), (unsigned)batch);
    hipLaunchKernelGGL(homography_score_kernel, grid, dim3(kHomographyScoreBlock), 0, st, (const Corr*)corr, n, H, S, h_count, thr, cnt,
                       s1, s2);
    return check_launch("homography_score_kernel");
}

int launch_mask(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch,
                const sfm_select_result* result, double thr, uint8_t* mask, hipStream_t st) {
    const dim3 grid(grid_stride(n, 256, 1024), (unsigned)batch);
    hipLaunchKernelGGL(homography_inlier_mask_kernel, grid, dim3(256), 0, st, (const Corr*)corr, n, H, S, h_count, result, thr, mask);
    return check_launch("homography_inlier_mask_kernel");
}

}  // namespace

extern "C" {

int sfm_homography_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* H, int32_t* flags,
                       void* stream) {
    const char* fn = "sfm_homography_fit";
    const int rc = check_call(fn, n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !H || !flags) return fail_in(fn, "null pointer");
    return launch_fit(false, 0, 0, 0, corr, n, h_count, batch, const_cast<int32_t*>(S), H, flags, (hipStream_t)stream);
}

int sfm_homography_score(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch, double thr,
                         int32_t* cnt, double* s1, double* s2, void* stream) {
    const char* fn = "sfm_homography_score";
    const int rc = check_call(fn, n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !H || !S || !cnt || !s1 || !s2) return fail_in(fn, "null pointer");
    return launch_score(corr, n, H, S, h_count, batch, thr, cnt, s1, s2, (hipStream_t)stream);
}

int sfm_homography_inlier_mask(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch,
                               const sfm_select_result* result, double thr, uint8_t* mask, void* stream) {
    const char* fn = "sfm_homography_inlier_mask";
    const int rc = check_call(fn, n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (batch == 0) return SFM_OK;
    if (!corr || !H || !S || !result || !mask) return fail_in(fn, "null pointer");
    return launch_mask(corr, n, H, S, h_count, batch, result, thr, mask, (hipStream_t)stream);
}

int sfm_homography_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S, double* H,
                               int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                               void* stream) {
    const char* fn = "sfm_homography_ransac_pass";
    hipStream_t st = (hipStream_t)stream;
    return sfmmin::ransac_pass(
        fn, check_call(fn, n, h_count, batch), kHomographySample, h_begin, h_count, batch, min_extra, aggregation, corr,
        {S, H, flags, cnt, s1, s2, result, mask}, stream,
        [&] { return launch_fit(use_philox != 0, seed, seed_stride, h_begin, corr, n, h_count, batch, S, H, flags, st); },
        [&] { return launch_score(corr, n, H, S, h_count, batch, thr, cnt, s1, s2, st); },
        [&] { return launch_mask(corr, n, H, S, h_count, batch, result, thr, mask, st); });
}

}  // extern "C"
