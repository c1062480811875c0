// RANSAC essential matrix with the five-point minimal solver (sfm_five_point.h): the solver of the fit kernel
// (sfmmin::minimal_fit_kernel, sfm_minimal_fit.h: from a sample table, or with Philox sampling fused in), the candidate dump the
// tests read, and the pass (fit, six-item scoring, selection, mask).  Items 0-4 of a sample are solved for; item 5 picks the candidate with the smallest SED.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "sfm_common.h"
#include "sfm_five_point.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_fits;
using sfmhost::grid_for;

using sfm5::five_point_solver;
using sfm5::kFiveSample;
using sfm5::load_items;
constexpr int kFitBlock = sfmmin::kMinimalFitBlock;

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
    return sfmhost::check_sizes(fn, kFiveSample, n, h_count, batch, {kFitBlock});
}

int fit_entry(const char* fn, bool philox, uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n,
              int64_t h_count, int64_t batch, int32_t* S, double* E, int32_t* flags, void* stream) {
    const int rc = check_fit(fn, n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_begin < 0) return fail_in(fn, "negative h_begin");
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !E || !flags) return fail_in(fn, "null pointer");
    return sfmmin::launch_minimal_fit<five_point_solver>((const Corr*)corr, philox, seed, seed_stride, h_begin, n, h_count, batch, S, E,
                                                       flags, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int sfm_five_point_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* E, int32_t* flags,
                       void* stream) {
    return fit_entry("sfm_five_point_fit", false, 0, 0, 0, corr, n, h_count, batch, const_cast<int32_t*>(S), E, flags, stream);
}

int sfm_five_point_sample_fit_philox(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n,
                                     int64_t h_count, int64_t batch, int32_t* S, double* E, int32_t* flags, void* stream) {
    return fit_entry("sfm_five_point_sample_fit_philox", true, seed, seed_stride, h_begin, corr, n, h_count, batch, S, E, flags, stream);
}

int sfm_five_point_candidates(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* out,
                              int32_t* count, void* stream) {
    const int rc = check_fit("sfm_five_point_candidates", n, h_count, batch);
    if (rc != SFM_OK) return rc;
    if (h_count == 0 || batch == 0) return SFM_OK;
    if (!corr || !S || !out || !count) return fail_in("sfm_five_point_candidates", "null pointer");
    hipLaunchKernelGGL(five_point_candidates_kernel, dim3(grid_for(h_count, kFitBlock), (unsigned)batch), dim3(kFitBlock), 0,
                       (hipStream_t)stream, (const Corr*)corr, n, S, h_count, out, count);
    return check_launch("five_point_candidates_kernel");
}

int sfm_five_point_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S, double* E,
                               int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                               void* stream) {
    const char* fn = "sfm_five_point_ransac_pass";
    // with the fit's: what the scoring launch (four hypotheses per 256-thread block) and the mask launch need
    int sizes = check_fit(fn, n, h_count, batch);
    if (sizes == SFM_OK && h_count > 0x3FFFFFFF) sizes = fail_in(fn, "size too large");
    if (sizes == SFM_OK && batch > 0 && (!grid_fits((h_count + 3) / 4, 4, 256, batch) || !grid_fits(n, 256, 256, batch)))
        sizes = fail_in(fn, "size exceeds what one launch covers");
    return sfmmin::ransac_pass(
        fn, sizes, kFiveSample, h_begin, h_count, batch, min_extra, aggregation, corr, {S, E, flags, cnt, s1, s2, result, mask}, stream,
        [&] {
            return sfmmin::launch_minimal_fit<five_point_solver>((const Corr*)corr, use_philox != 0, seed, seed_stride, h_begin, n, h_count,
                                                               batch, S, E, flags, (hipStream_t)stream);
        },
        [&] { return sfm_score_sed_sample_ex(corr, n, E, S, h_count, batch, thr, kFiveSample, cnt, s1, s2, stream); },
        [&] { return sfm_inlier_mask(corr, n, E, S, h_count, batch, result, thr, kFiveSample, mask, stream); });
}

}  // extern "C"
