// RANSAC essential matrix with the five-point minimal solver (sfm_five_point.h): the fit kernels (from a sample
// table, or with Philox sampling fused in), the candidate dump the tests read, and the pass (fit, six-item scoring, selection,
// mask).  Items 0-4 of a sample are solved for; item 5 picks the candidate with the smallest SED.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "sfm_common.h"
#include "sfm_five_point.h"
#include "sfm_math.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_fits;
using sfmhost::grid_for;

constexpr int kFiveSample = 6;   // five items solved for, the sixth picks the solution
constexpr int kFitBlock = 64;

// The items of one sample; bad when an index is out of range.
SFM_DEVICE void load_items(const Corr* __restrict__ pts, int64_t n, const int32_t (&idx)[8], double (&xa)[5], double (&ya)[5],
                           double (&xb)[5], double (&yb)[5], Corr& item5, bool& bad) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const Corr p = pts[checked_index(idx[i], n, bad)];
        xa[i] = p.xa;
        ya[i] = p.ya;
        xb[i] = p.xb;
        yb[i] = p.yb;
    }
    item5 = pts[checked_index(idx[5], n, bad)];
}

// Five-point fit of one hypothesis: SFM_FIT_DEGENERATE for a degenerate sample or an index out of range (E = 9 NaNs then),
// otherwise the candidate with the strictly smallest SED on item 5, or 9 NaNs when there is none (flag 0).
SFM_DEVICE int fit_one(const Corr* __restrict__ pts, int64_t n, const int32_t (&idx)[8], double (&out)[9]) {
    double xa[5], ya[5], xb[5], yb[5];
    Corr q;
    bool bad = false;
    load_items(pts, n, idx, xa, ya, xb, yb, q, bad);
    double best = INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = NAN;
    bool degenerate = true;
    if (!bad) {
        degenerate = sfm5::solve(xa, ya, xb, yb, [&](const double (&E)[9]) {
            const double sed = sfm::sed_value(E, q.xa, q.ya, q.xb, q.yb);
            const bool take = sed < best;
            best = take ? sed : best;
#pragma unroll
            for (int i = 0; i < 9; ++i) out[i] = take ? E[i] : out[i];
        });
    }
    return (bad || degenerate) ? SFM_FIT_DEGENERATE : 0;
}

__global__ __launch_bounds__(kFitBlock) void five_point_fit_kernel(const Corr* __restrict__ corr, int64_t n,
                                                                   const int32_t* __restrict__ S, int64_t h_count,
                                                                   double* __restrict__ E, int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= h_count) return;
    const int64_t b = blockIdx.y;
    const int64_t bh = b * h_count + h;
    int32_t idx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) idx[i] = i < kFiveSample ? S[bh * 8 + i] : 0;
    double out[9];
    const int flag = fit_one(corr + b * n, n, idx, out);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[bh * 9 + i] = out[i];
    flags[bh] = flag;
}

// Philox sampling fused into the fit: the first six of philox_sample8 are the sample; S receives all eight, with -1 at
// positions >= n (so n = 6 and 7 are valid).
__global__ __launch_bounds__(kFitBlock) void five_point_sample_fit_philox_kernel(uint64_t seed, uint64_t seed_stride, int64_t h_begin,
                                                                                 const Corr* __restrict__ corr, int64_t n,
                                                                                 int64_t h_count, int32_t* __restrict__ S,
                                                                                 double* __restrict__ E, int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= h_count) return;
    const int64_t b = blockIdx.y;
    const int64_t bh = b * h_count + h;
    int32_t idx[8];
    sfm::philox_sample8(seed + (uint64_t)b * seed_stride, (uint64_t)(h_begin + h), (uint32_t)n, idx);
#pragma unroll
    for (int i = kFiveSample; i < 8; ++i) idx[i] = i < n ? idx[i] : -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) S[bh * 8 + i] = idx[i];
    double out[9];
    const int flag = fit_one(corr + b * n, n, idx, out);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[bh * 9 + i] = out[i];
    flags[bh] = flag;
}

// Every candidate of each sample in ascending root order: out [batch, h, 10, 9] (NaN beyond the count), count [batch, h]
// (-1 for a degenerate sample or an index out of range).
__global__ __launch_bounds__(kFitBlock) void five_point_candidates_kernel(const Corr* __restrict__ corr, int64_t n,
                                                                          const int32_t* __restrict__ S, int64_t h_count,
                                                                          double* __restrict__ out, int32_t* __restrict__ count) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= h_count) return;
    const int64_t b = blockIdx.y;
    const int64_t bh = b * h_count + h;
    int32_t idx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) idx[i] = i < kFiveSample ? S[bh * 8 + i] : 0;
    double xa[5], ya[5], xb[5], yb[5];
    Corr q;
    bool bad = false;
    load_items(corr + b * n, n, idx, xa, ya, xb, yb, q, bad);
    double* dst = out + bh * (sfm5::kMaxCandidates * 9);
    for (int k = 0; k < sfm5::kMaxCandidates * 9; ++k) dst[k] = NAN;
    int c = 0;
    bool degenerate = true;
    if (!bad) {
        degenerate = sfm5::solve(xa, ya, xb, yb, [&](const double (&E)[9]) {
#pragma unroll
            for (int i = 0; i < 9; ++i) dst[c * 9 + i] = E[i];   // c < kMaxCandidates: the solver visits at most that many
            ++c;
        });
    }
    count[bh] = (bad || degenerate) ? -1 : c;
}

int check_fit(const char* fn, int64_t n, int64_t h_count, int64_t batch) {
    char msg[160];
    if (h_count < 0 || batch < 0 || n < 0) {
        snprintf(msg, sizeof msg, "%s: negative size", fn);
        return fail(SFM_EINVAL, msg);
    }
    if (n < kFiveSample) {
        snprintf(msg, sizeof msg, "%s: need at least 6 correspondences", fn);
        return fail(SFM_EINVAL, msg);
    }
    if (n > 0x7FFFFFFF || batch > 65535 || !grid_fits(h_count, kFitBlock, kFitBlock, batch)) {
        snprintf(msg, sizeof msg, "%s: size exceeds what one launch covers", fn);
        return fail(SFM_EINVAL, msg);
    }
    return SFM_OK;
}

}  // namespace

extern "C" {

int sfm_five_point_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* E, int32_t* flags,
                       void* stream) {
    const int rc = check_fit("sfm_five_point_fit", n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !E || !flags) return fail(SFM_EINVAL, "sfm_five_point_fit: null pointer");
    hipLaunchKernelGGL(five_point_fit_kernel, dim3(grid_for(h_count, kFitBlock), (unsigned)batch), dim3(kFitBlock), 0,
                       (hipStream_t)stream, (const Corr*)corr, n, S, h_count, E, flags);
    return check_launch("five_point_fit_kernel");
}

int sfm_five_point_sample_fit_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n,
                                     int64_t h_count, int64_t batch, int32_t* S, double* E, int32_t* flags, void* stream) {
    const int rc = check_fit("sfm_five_point_sample_fit_philox", n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_begin < 0) return fail(SFM_EINVAL, "sfm_five_point_sample_fit_philox: negative h_begin");
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !E || !flags) return fail(SFM_EINVAL, "sfm_five_point_sample_fit_philox: null pointer");
    hipLaunchKernelGGL(five_point_sample_fit_philox_kernel, dim3(grid_for(h_count, kFitBlock), (unsigned)batch), dim3(kFitBlock), 0,
                       (hipStream_t)stream, seed, seed_stride, h_begin, (const Corr*)corr, n, h_count, S, E, flags);
    return check_launch("five_point_sample_fit_philox_kernel");
}

int sfm_five_point_candidates(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* out,
                              int32_t* count, void* stream) {
    const int rc = check_fit("sfm_five_point_candidates", n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !out || !count) return fail(SFM_EINVAL, "sfm_five_point_candidates: null pointer");
    hipLaunchKernelGGL(five_point_candidates_kernel, dim3(grid_for(h_count, kFitBlock), (unsigned)batch), dim3(kFitBlock), 0,
                       (hipStream_t)stream, (const Corr*)corr, n, S, h_count, out, count);
    return check_launch("five_point_candidates_kernel");
}

int sfm_five_point_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S, double* E,
                               int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                               void* stream) {
    // every argument and grid is checked before the first launch: a refused call has enqueued nothing
    int rc = check_fit("sfm_five_point_ransac_pass", n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail(SFM_EINVAL, "sfm_five_point_ransac_pass: unknown aggregation");
    if (h_begin < 0) return fail(SFM_EINVAL, "sfm_five_point_ransac_pass: negative h_begin");
    if (h_count > 0x3FFFFFFF) return fail(SFM_EINVAL, "sfm_five_point_ransac_pass: size too large");
    if (batch == 0) return SFM_OK;
    if (!corr || !S || !E || !flags || !cnt || !s1 || !s2 || !result) return fail(SFM_EINVAL, "sfm_five_point_ransac_pass: null pointer");
    if (!sfmhost::grid_fits((h_count + 3) / 4, 4, 256, batch) || !grid_fits(n, 256, 256, batch))
        return fail(SFM_EINVAL, "sfm_five_point_ransac_pass: size exceeds what one launch covers");
    if (h_count > 0) {
        rc = use_philox ? sfm_five_point_sample_fit_philox(seed, seed_stride, h_begin, corr, n, h_count, batch, S, E, flags, stream)
                        : sfm_five_point_fit(corr, n, S, h_count, batch, E, flags, stream);
        if (rc != SFM_OK) return rc;
        rc = sfm_score_sed_sample_ex(corr, n, E, S, h_count, batch, thr, kFiveSample, cnt, s1, s2, stream);
        if (rc != SFM_OK) return rc;
    }
    rc = sfm_select_best(cnt, s1, s2, flags, h_count, batch, min_extra, aggregation, 0, kFiveSample, result, stream);
    if (rc != SFM_OK || mask == nullptr) return rc;
    return sfm_inlier_mask(corr, n, E, S, h_count, batch, result, thr, kFiveSample, mask, stream);
}

}  // extern "C"
