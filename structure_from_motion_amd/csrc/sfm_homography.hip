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
#include "sfm_minimal_score.h"

namespace {

using sfmhg::homography_model;
using sfmhg::homography_solver;
using sfmhg::kHomographySample;
using sfmhost::checked_entry;

// ---- host side ---------------------------------------------------------------------------------------------------------
// Every check of a call that depends on its sizes, before anything is launched: four items per sample, n at least that, and the
// grids of the fit and scoring launches.
int check_call(const char* fn, int64_t n, int64_t h_count, int64_t batch) {
    return sfmhost::check_sizes(fn, kHomographySample, n, h_count, batch, {sfmmin::kScoreBlock, sfmmin::kMinimalFitBlock});
}

int launch_fit(bool philox, uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n, int64_t h_count,
               int64_t batch, int32_t* S, double* H, int32_t* flags, hipStream_t st) {
    return sfmmin::launch_minimal_fit<homography_solver>((const Corr*)corr, philox, seed, seed_stride, h_begin, n, h_count, batch, S, H,
                                                       flags, st);
}

// Scoring and the winner's mask are the kernels of sfm_minimal_score.h over homography_model, with a sample of four: all fp64
// with true divisions, so every value is the NumPy definition's bit for bit and only the summation order differs.
constexpr auto launch_score = sfmmin::launch_score<kHomographySample, homography_model>;
constexpr auto launch_mask = sfmmin::launch_mask<kHomographySample, homography_model>;

}  // namespace

extern "C" {

int sfm_homography_fit(const double* corr, int64_t n, const int32_t* S, int64_t h_count, int64_t batch, double* H, int32_t* flags,
                       void* stream) {
    const char* fn = "sfm_homography_fit";
    return checked_entry(fn, check_call(fn, n, h_count, batch), h_count == 0 || batch == 0, !corr || !S || !H || !flags, [&] {
        return launch_fit(false, 0, 0, 0, corr, n, h_count, batch, const_cast<int32_t*>(S), H, flags, (hipStream_t)stream);
    });
}

int sfm_homography_score(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch, double thr,
                         int32_t* cnt, double* s1, double* s2, void* stream) {
    const char* fn = "sfm_homography_score";
    return checked_entry(fn, check_call(fn, n, h_count, batch), h_count == 0 || batch == 0, !corr || !H || !S || !cnt || !s1 || !s2, [&] {
        return launch_score((const Corr*)corr, n, H, S, h_count, batch, thr, cnt, s1, s2, (hipStream_t)stream);
    });
}

int sfm_homography_inlier_mask(const double* corr, int64_t n, const double* H, const int32_t* S, int64_t h_count, int64_t batch,
                               const sfm_select_result* result, double thr, uint8_t* mask, void* stream) {
    const char* fn = "sfm_homography_inlier_mask";
    return checked_entry(fn, check_call(fn, n, h_count, batch), batch == 0, !corr || !H || !S || !result || !mask, [&] {
        return launch_mask((const Corr*)corr, n, H, S, h_count, batch, result, thr, mask, (hipStream_t)stream);
    });
}

int sfm_homography_ransac_pass(uint64_t seed, uint64_t seed_stride, int use_philox, int64_t h_begin, const double* corr, int64_t n,
                               int64_t h_count, int64_t batch, double thr, double min_extra, int aggregation, int32_t* S, double* H,
                               int32_t* flags, int32_t* cnt, double* s1, double* s2, sfm_select_result* result, uint8_t* mask,
                               void* stream) {
    const char* fn = "sfm_homography_ransac_pass";
    hipStream_t st = (hipStream_t)stream;
    const Corr* items = (const Corr*)corr;
    return sfmmin::ransac_pass(
        fn, check_call(fn, n, h_count, batch), kHomographySample, h_begin, h_count, batch, min_extra, aggregation, corr,
        {S, H, flags, cnt, s1, s2, result, mask}, stream,
        [&] { return launch_fit(use_philox != 0, seed, seed_stride, h_begin, corr, n, h_count, batch, S, H, flags, st); },
        [&] { return launch_score(items, n, H, S, h_count, batch, thr, cnt, s1, s2, st); },
        [&] { return launch_mask(items, n, H, S, h_count, batch, result, thr, mask, st); });
}

}  // extern "C"
