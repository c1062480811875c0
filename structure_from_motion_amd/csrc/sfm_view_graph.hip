// Two-view verification of every image pair of a match graph in one call: the homography pass and the
// five-point essential pass of each pair, over the pairs' concatenated correspondences ("ragged": pair q owns items
// offset[q] .. offset[q+1]-1, any count per pair), their two selections, both winners' masks and a verdict per pair.  Pair q's
// outputs are what sfm_homography_ransac_pass(seed + q * seed_stride, use_philox = 1) followed by sfm_five_point_ransac_pass on
// the same rows of S (use_philox = 0) give on that pair alone: the solvers (sfm_homography.h, sfm_five_point.h), the transfer
// error, sfm::sed_value, the selection (sfmsel::block_select) and the mask values are the same device routines.
//
// Seven launches whatever the number of pairs, nothing read back; all but the last are the ragged pass of sfm_ragged_pass.h,
// behind a wrapper of this file where both models share a launch:
//   1. sfmrag::ragged_offsets_kernel   the offset table is non-decreasing within [0, N], or every verdict is
//                                      SFM_PAIR_BAD_OFFSETS; the later launches read that mark and then treat every pair as
//                                      empty, so nothing is indexed by it
//   2. sfmrag::ragged_fit_kernel<homography_solver, true>    grid (h / 64, pairs): one hypothesis per lane, the homography fit
//                                      (draws the Philox sample, fills S)
//   3. sfmrag::ragged_fit_kernel<five_point_solver, false>   the five-point fit of the same samples
//   4. verify_score_kernel             grid (h / 256, pairs, 2): sfmrag::score_block, one hypothesis per lane, the pair's items
//                                      staged through LDS in tiles of 512, the sample items corrected after the tile loop;
//                                      z = 0 the homographies, z = 1 the essentials
//   5. verify_select_kernel            grid (pairs, 2): sfmrag::select_block with the pair's own min_extra
//   6. verify_mask_kernel              both masks (sfmrag::winner_mask_value), a grid-stride walk over all N items (an item
//                                      finds its pair by bisection)
//   7. verdict_kernel                  counts, ratio and kind of each pair
// A pair with fewer items than a model's sample (4, 6) gets that model's filler: rows of S all -1 (n < 4 only: the homography
// fit owns S), models of 9 NaNs, flags SFM_FIT_DEGENERATE, cnt 0, s1 = s2 = NaN, and so a record without a winner whose
// n_flagged is h_count.  Every sum runs in item order in one lane: no atomics, and a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_five_point.h"
#include "sfm_homography.h"
#include "sfm_math.h"
#include "sfm_ragged_pass.h"

static_assert(sizeof(sfm_pair_verdict) == 24 && offsetof(sfm_pair_verdict, kind) == 0, "sfm_pair_verdict: 24 bytes, the kind first");

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_for;
using sfmhost::grid_stride;
using sfmrag::kScoreBlock;
using sfmrag::kSelectBlock;
using sfmrag::Mark;

constexpr int kHSample = sfmhg::kHomographySample, kESample = sfm5::kFiveSample;
using HScorer = sfmrag::model_scorer<kHSample, sfmhg::homography_model>;
using EScorer = sfmrag::model_scorer<kESample, sfm5::essential_model>;

// The mark of pair q is the kind of its verdict, whose other fields are written by verdict_kernel.
Mark mark_of(sfm_pair_verdict* verdict) { return Mark{&verdict->kind, (int64_t)(sizeof(sfm_pair_verdict) / sizeof(int32_t))}; }

// One hypothesis per lane over its pair's items, with the model that z selected.
__global__ __launch_bounds__(kScoreBlock) void verify_score_kernel(const Corr* __restrict__ corr, const int64_t* __restrict__ offset,
                                                                   Mark mark, const int32_t* __restrict__ S, const double* __restrict__ H,
                                                                   const double* __restrict__ E, int64_t h_count, double thr,
                                                                   int32_t* __restrict__ h_cnt, double* __restrict__ h_s1,
                                                                   double* __restrict__ h_s2, int32_t* __restrict__ e_cnt,
                                                                   double* __restrict__ e_s1, double* __restrict__ e_s2) {
    __shared__ Corr tile[sfmmin::kScoreTile];
    const int64_t q = blockIdx.y;
    const sfmrag::Range r = sfmrag::range_of(offset, mark, q);
    if (blockIdx.z != 0) sfmrag::score_block<EScorer>(tile, corr, r, q, E, S, h_count, thr, e_cnt, e_s1, e_s2);
    else sfmrag::score_block<HScorer>(tile, corr, r, q, H, S, h_count, thr, h_cnt, h_s1, h_s2);
}

// Block (q, model) selects over pair q's h_count rows of that model.
__global__ __launch_bounds__(kSelectBlock) void verify_select_kernel(const int32_t* __restrict__ h_cnt, const double* __restrict__ h_s1,
                                                                     const double* __restrict__ h_s2, const int32_t* __restrict__ h_flags,
                                                                     const int32_t* __restrict__ e_cnt, const double* __restrict__ e_s1,
                                                                     const double* __restrict__ e_s2, const int32_t* __restrict__ e_flags,
                                                                     int64_t h_count, const double* __restrict__ min_extra, int aggregation,
                                                                     sfm_select_result* __restrict__ h_result,
                                                                     sfm_select_result* __restrict__ e_result) {
    __shared__ sfmsel::SelectScratch<kSelectBlock> scratch;
    __shared__ int64_t winner;
    if (blockIdx.y == 0)
        sfmrag::select_block(kHSample, h_cnt, h_s1, h_s2, h_flags, h_count, min_extra, aggregation, h_result, scratch, &winner);
    else
        sfmrag::select_block(kESample, e_cnt, e_s1, e_s2, e_flags, h_count, min_extra, aggregation, e_result, scratch, &winner);
}

// Both masks of every item: 2 for the sample items of the pair's winner, 1 for its other items within the threshold, 0 otherwise,
// and 0 for an item no pair owns or whose pair has no winner.
__global__ void verify_mask_kernel(const Corr* __restrict__ corr, int64_t n_total, const int64_t* __restrict__ offset, int64_t pairs,
                                   Mark mark, const int32_t* __restrict__ S, const double* __restrict__ H, const double* __restrict__ E,
                                   int64_t h_count, const sfm_select_result* __restrict__ h_result,
                                   const sfm_select_result* __restrict__ e_result, double thr, uint8_t* __restrict__ h_mask,
                                   uint8_t* __restrict__ e_mask) {
    const bool bad = mark.bad(0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        const int64_t q = bad ? -1 : pair_of_item(offset, pairs, i);
        uint8_t hm = 0, em = 0;
        if (q >= 0) {
            hm = sfmrag::winner_mask_value<kHSample, sfmhg::homography_model>(corr, i, offset, mark, q, S, H, h_count, h_result, thr);
            em = sfmrag::winner_mask_value<kESample, sfm5::essential_model>(corr, i, offset, mark, q, S, E, h_count, e_result, thr);
        }
        h_mask[i] = hm;
        e_mask[i] = em;
    }
}

// count = the winner's sample size plus its extra inliers, 0 without a winner; ratio = homography / essential count, inf when
// the latter is 0; kind: none without any winner, homography when E has none or ratio > max_ratio, else essential.
__global__ void verdict_kernel(const sfm_select_result* __restrict__ h_result, const sfm_select_result* __restrict__ e_result,
                               int64_t pairs, double max_ratio, sfm_pair_verdict* __restrict__ verdict) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pairs) return;
    const bool bad = verdict[q].kind == SFM_PAIR_BAD_OFFSETS;
    const int32_t hc = (!bad && h_result[q].best_h >= 0) ? kHSample + h_result[q].best_cnt : 0;
    const int32_t ec = (!bad && e_result[q].best_h >= 0) ? kESample + e_result[q].best_cnt : 0;
    const double ratio = ec == 0 ? INFINITY : (double)hc / (double)ec;
    sfm_pair_verdict v;
    v.kind = bad ? SFM_PAIR_BAD_OFFSETS
                 : ((hc == 0 && ec == 0) ? SFM_PAIR_NONE : ((ec == 0 || ratio > max_ratio) ? SFM_PAIR_HOMOGRAPHY : SFM_PAIR_ESSENTIAL));
    v.homography_count = hc;
    v.essential_count = ec;
    v.reserved = 0;
    v.ratio = ratio;
    verdict[q] = v;
}

}  // namespace

extern "C" {

int sfm_verify_pairs(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* corr, int64_t n_total, const int64_t* offset,
                     int64_t pairs, const double* min_extra, int64_t h_count, double thr, int aggregation, double max_ratio, int32_t* S,
                     double* H, double* E, int32_t* h_flags, int32_t* h_cnt, double* h_s1, double* h_s2, int32_t* e_flags,
                     int32_t* e_cnt, double* e_s1, double* e_s2, sfm_select_result* h_result, sfm_select_result* e_result,
                     uint8_t* h_mask, uint8_t* e_mask, sfm_pair_verdict* verdict, void* stream) {
    const char* fn = "sfm_verify_pairs";
    // every check before the first launch: a refused call has enqueued nothing
    const int rc = sfmrag::check_sizes(fn, n_total, pairs, h_count, 0, 2, aggregation, h_begin);
    if (rc != SFM_OK) return rc;
    if (pairs == 0) return SFM_OK;
    if (!offset || !min_extra || !h_result || !e_result || !verdict || (n_total > 0 && (!corr || !h_mask || !e_mask)) ||
        (h_count > 0 && (!S || !H || !E || !h_flags || !h_cnt || !h_s1 || !h_s2 || !e_flags || !e_cnt || !e_s1 || !e_s2)))
        return fail_in(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Corr* items = (const Corr*)corr;
    const Mark mark = mark_of(verdict);
    hipLaunchKernelGGL(sfmrag::ragged_offsets_kernel, dim3(1), dim3(sfmrag::kCheckBlock), 0, st, offset, pairs, n_total, n_total, mark,
                       SFM_PAIR_NONE);
    if (h_count > 0) {
        const dim3 fit_grid(grid_for(h_count, sfmrag::kFitBlock), (unsigned)pairs), fit_block(sfmrag::kFitBlock);
        hipLaunchKernelGGL((sfmrag::ragged_fit_kernel<sfmhg::homography_solver, true>), fit_grid, fit_block, 0, st, items, offset, mark, seed,
                           seed_stride, h_begin, h_count, S, H, h_flags);
        hipLaunchKernelGGL((sfmrag::ragged_fit_kernel<sfm5::five_point_solver, false>), fit_grid, fit_block, 0, st, items, offset, mark, seed,
                           seed_stride, h_begin, h_count, S, E, e_flags);
        hipLaunchKernelGGL(verify_score_kernel, dim3(grid_for(h_count, kScoreBlock), (unsigned)pairs, 2), dim3(kScoreBlock), 0, st, items,
                           offset, mark, S, H, E, h_count, thr, h_cnt, h_s1, h_s2, e_cnt, e_s1, e_s2);
    }
    hipLaunchKernelGGL(verify_select_kernel, dim3((unsigned)pairs, 2), dim3(kSelectBlock), 0, st, h_cnt, h_s1, h_s2, h_flags, e_cnt, e_s1,
                       e_s2, e_flags, h_count, min_extra, aggregation, h_result, e_result);
    if (n_total > 0)
        hipLaunchKernelGGL(verify_mask_kernel, dim3(grid_stride(n_total, sfmrag::kMaskBlock, sfmrag::kMaskBlocks)), dim3(sfmrag::kMaskBlock),
                           0, st, items, n_total, offset, pairs, mark, S, H, E, h_count, h_result, e_result, thr, h_mask, e_mask);
    hipLaunchKernelGGL(verdict_kernel, dim3(grid_for(pairs, 256)), dim3(256), 0, st, h_result, e_result, pairs, max_ratio, verdict);
    return check_launch(fn);
}

}  // extern "C"
