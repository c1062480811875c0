// Two-view verification of every image pair of a match graph in one call: the homography pass and the
// five-point essential pass of each pair, over the pairs' concatenated correspondences ("ragged": pair q owns items
// offset[q] .. offset[q+1]-1, any count per pair), their two selections, both winners' masks and a verdict per pair.  Pair q's
// outputs are what sfm_homography_ransac_pass(seed + q * seed_stride, use_philox = 1) followed by sfm_five_point_ransac_pass on
// the same rows of S (use_philox = 0) give on that pair alone: the solvers (sfm_homography.h, sfm_five_point.h), the transfer
// error, sfm::sed_value, the selection (sfmsel::block_select) and the mask values are the same device routines.
//
// Seven launches whatever the number of pairs, nothing read back:
//   1. offsets_check_kernel   the offset table is non-decreasing within [0, N], or every verdict is SFM_PAIR_BAD_OFFSETS; the
//                             later launches read that mark and then treat every pair as empty, so nothing is indexed by it
//   2. ragged_fit_kernel<0>   grid (h / 64, pairs): one hypothesis per lane, the homography fit (draws the Philox sample, fills S)
//   3. ragged_fit_kernel<1>   the five-point fit of the same samples
//   4. ragged_score_kernel    grid (h / 256, pairs, 2): one hypothesis per lane, the pair's items staged through LDS in tiles of
//                             512, the sample items corrected after the tile loop; z = 0 the homographies, z = 1 the essentials
//   5. ragged_select_kernel   grid (pairs, 2): sfmsel::block_select with the pair's own min_extra
//   6. ragged_mask_kernel     both masks, a grid-stride walk over all N items (an item finds its pair by bisection)
//   7. verdict_kernel         counts, ratio and kind of each pair
// A pair with fewer items than a model's sample (4, 6) gets that model's filler: rows of S all -1 (n < 4 only: the homography
// fit owns S), models of 9 NaNs, flags SFM_FIT_DEGENERATE, cnt 0, s1 = s2 = NaN, and so a record without a winner whose
// n_flagged is h_count.  Every sum runs in item order in one lane: no atomics, and a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_five_point.h"
#include "sfm_homography.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_select.h"

static_assert(sizeof(sfm_pair_verdict) == 24, "sfm_pair_verdict is 24 bytes");

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_fits;
using sfmhost::grid_for;
using sfmhost::grid_stride;

constexpr int kFitBlock = sfmmin::kMinimalFitBlock;
using sfmmin::kScoreBlock;
constexpr int kSelectBlock = 1024;
constexpr int kCheckBlock = 1024;
constexpr int kHSample = sfmhg::kHomographySample, kESample = sfm5::kFiveSample;

// The items of pair q: none when the offset table was refused (the table itself always holds pairs + 1 entries).
struct PairItems {
    const Corr* pts;
    int64_t first, n;
};
SFM_DEVICE PairItems pair_items(const Corr* __restrict__ corr, const int64_t* __restrict__ offset,
                                const sfm_pair_verdict* __restrict__ verdict, int64_t q) {
    const bool bad = verdict[q].kind == SFM_PAIR_BAD_OFFSETS;
    const int64_t lo = bad ? 0 : offset[q], hi = bad ? 0 : offset[q + 1];
    return PairItems{corr + lo, lo, hi - lo};
}

// One block: 0 <= offset[0] <= offset[1] <= ... <= offset[pairs] <= n_total, or every verdict SFM_PAIR_BAD_OFFSETS.  The other
// fields of the records are written by verdict_kernel.
__global__ __launch_bounds__(kCheckBlock) void offsets_check_kernel(const int64_t* __restrict__ offset, int64_t pairs, int64_t n_total,
                                                                    sfm_pair_verdict* __restrict__ verdict) {
    bool ok = true;
    for (int64_t k = threadIdx.x; k <= pairs; k += kCheckBlock) {
        const int64_t v = offset[k];
        ok = ok && v >= 0 && v <= n_total && (k == 0 || offset[k - 1] <= v);
    }
    const int kind = __syncthreads_and(ok ? 1 : 0) ? SFM_PAIR_NONE : SFM_PAIR_BAD_OFFSETS;
    for (int64_t q = threadIdx.x; q < pairs; q += kCheckBlock) verdict[q].kind = kind;
}

// ESSENTIAL false: the homography fit, which draws the sample and stores its row of S; true: the five-point fit of the same
// sample.  Two launches of one body: a lane of the five-point solver needs every register there is (and spills, as in its
// single-pair kernel), and the homography fit should not inherit that.
template <bool ESSENTIAL>
__global__ __launch_bounds__(kFitBlock) void ragged_fit_kernel(const Corr* __restrict__ corr, const int64_t* __restrict__ offset,
                                                               const sfm_pair_verdict* __restrict__ verdict, uint64_t seed,
                                                               uint64_t seed_stride, int64_t h_begin, int64_t h_count,
                                                               int32_t* __restrict__ S, double* __restrict__ model_out,
                                                               int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * kFitBlock + threadIdx.x;
    if (h >= h_count) return;
    const int64_t q = blockIdx.y;
    const int64_t qh = q * h_count + h;
    const PairItems p = pair_items(corr, offset, verdict, q);
    double* __restrict__ model = model_out + qh * 9;
    int32_t* __restrict__ flag = flags + qh;
    if (p.n < (ESSENTIAL ? kESample : kHSample)) {   // the filler of a pair too small for this model
#pragma unroll
        for (int i = 0; i < 9; ++i) model[i] = NAN;
        *flag = SFM_FIT_DEGENERATE;
        if constexpr (!ESSENTIAL) {
#pragma unroll
            for (int i = 0; i < 8; ++i) S[qh * 8 + i] = -1;
        }
        return;
    }
    int32_t idx[8];
    sfm::philox_sample8(seed + (uint64_t)q * seed_stride, (uint64_t)(h_begin + h), (uint32_t)p.n, idx);
    double out[9];
    int fit_flag;
    if constexpr (ESSENTIAL) {   // positions 0-5 of the row the homography fit stores: all below n, since n >= 6
        fit_flag = sfm5::five_point_solver::fit(p.pts, 0, p.n, idx, out);
    } else {
#pragma unroll
        for (int i = kHSample; i < 8; ++i) idx[i] = i < p.n ? idx[i] : -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) S[qh * 8 + i] = idx[i];
        fit_flag = sfmhg::homography_solver::fit(p.pts, 0, p.n, idx, out);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) model[i] = out[i];
    *flag = fit_flag;
}

// One hypothesis per lane over its pair's items: sfmmin::score_hypothesis (sfm_minimal_score.h) with the pair's items, the
// lane's row of S and the model that z selected.
template <class Model, int SAMPLE>
SFM_DEVICE void score_pair(Corr* tile, const PairItems& p, const double* __restrict__ model, const int32_t* __restrict__ S, int64_t q,
                           int64_t h_count, double thr, int32_t* __restrict__ cnt, double* __restrict__ s1, double* __restrict__ s2) {
    const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    const int64_t hc = h < h_count ? h : h_count - 1;   // lanes past the end score a valid hypothesis and store nothing
    const int64_t qh = q * h_count + hc;
    const sfmmin::HypothesisScore r = sfmmin::score_hypothesis<SAMPLE>(tile, Model(model + qh * 9), p.pts, p.n, S + qh * 8, thr);
    if (h < h_count) {
        cnt[q * h_count + h] = r.c;
        s1[q * h_count + h] = r.a1;
        s2[q * h_count + h] = r.a2;
    }
}

__global__ __launch_bounds__(kScoreBlock) void ragged_score_kernel(const Corr* __restrict__ corr, const int64_t* __restrict__ offset,
                                                                   const sfm_pair_verdict* __restrict__ verdict,
                                                                   const int32_t* __restrict__ S, const double* __restrict__ H,
                                                                   const double* __restrict__ E, int64_t h_count, double thr,
                                                                   int32_t* __restrict__ h_cnt, double* __restrict__ h_s1,
                                                                   double* __restrict__ h_s2, int32_t* __restrict__ e_cnt,
                                                                   double* __restrict__ e_s1, double* __restrict__ e_s2) {
    __shared__ Corr tile[sfmmin::kScoreTile];
    const int64_t q = blockIdx.y;
    const bool essential = blockIdx.z != 0;   // uniform over the block, like everything tested before a barrier below
    const PairItems p = pair_items(corr, offset, verdict, q);
    if (p.n < (essential ? kESample : kHSample)) {
        const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
        if (h < h_count) {
            (essential ? e_cnt : h_cnt)[q * h_count + h] = 0;
            (essential ? e_s1 : h_s1)[q * h_count + h] = NAN;
            (essential ? e_s2 : h_s2)[q * h_count + h] = NAN;
        }
        return;
    }
    if (essential) score_pair<sfm5::essential_model, kESample>(tile, p, E, S, q, h_count, thr, e_cnt, e_s1, e_s2);
    else score_pair<sfmhg::homography_model, kHSample>(tile, p, H, S, q, h_count, thr, h_cnt, h_s1, h_s2);
}

// The per-pair form of the selection: block (q, model) runs the one definition of sfm_select.h over pair q's h_count rows
// with min_extra[q].
__global__ __launch_bounds__(kSelectBlock) void ragged_select_kernel(const int32_t* __restrict__ h_cnt, const double* __restrict__ h_s1,
                                                                     const double* __restrict__ h_s2, const int32_t* __restrict__ h_flags,
                                                                     const int32_t* __restrict__ e_cnt, const double* __restrict__ e_s1,
                                                                     const double* __restrict__ e_s2, const int32_t* __restrict__ e_flags,
                                                                     int64_t h_count, const double* __restrict__ min_extra, int aggregation,
                                                                     sfm_select_result* __restrict__ h_result,
                                                                     sfm_select_result* __restrict__ e_result) {
    __shared__ sfmsel::SelectScratch<kSelectBlock> scratch;
    __shared__ int64_t winner;
    const int64_t q = blockIdx.x, first = q * h_count;
    const double gate = min_extra[q];
    if (blockIdx.y == 0)
        sfmsel::block_select<kSelectBlock>(h_cnt + first, h_s1 + first, h_s2 + first, h_flags + first, h_count, 0, gate, aggregation,
                                           h_result + q, scratch, &winner, kHSample);
    else
        sfmsel::block_select<kSelectBlock>(e_cnt + first, e_s1 + first, e_s2 + first, e_flags + first, h_count, 0, gate, aggregation,
                                           e_result + q, scratch, &winner, kESample);
}

// Both masks of every item: 2 for the sample items of the pair's winner, 1 for its other items within the threshold, 0 otherwise,
// and 0 for an item no pair owns or whose pair has no winner.
__global__ void ragged_mask_kernel(const Corr* __restrict__ corr, int64_t n_total, const int64_t* __restrict__ offset, int64_t pairs,
                                   const sfm_pair_verdict* __restrict__ verdict, const int32_t* __restrict__ S,
                                   const double* __restrict__ H, const double* __restrict__ E, int64_t h_count,
                                   const sfm_select_result* __restrict__ h_result, const sfm_select_result* __restrict__ e_result,
                                   double thr, uint8_t* __restrict__ h_mask, uint8_t* __restrict__ e_mask) {
    const bool bad = verdict[0].kind == SFM_PAIR_BAD_OFFSETS;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        const int64_t q = bad ? -1 : pair_of_item(offset, pairs, i);
        uint8_t hm = 0, em = 0;
        if (q >= 0) {
            const int64_t local = i - offset[q];
            const Corr t = corr[i];
            const int64_t hb = h_result[q].best_h, eb = e_result[q].best_h;
            if (hb >= 0 && hb < h_count) {
                const int64_t qh = q * h_count + hb;
                hm = sfmmin::mask_value<kHSample>(sfmhg::homography_model(H + qh * 9), S + qh * 8, t, local, thr);
            }
            if (eb >= 0 && eb < h_count) {
                const int64_t qh = q * h_count + eb;
                em = sfmmin::mask_value<kESample>(sfm5::essential_model(E + qh * 9), S + qh * 8, t, local, thr);
            }
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
    if (n_total < 0 || pairs < 0 || h_count < 0) return fail_in(fn, "negative size");
    if (n_total > 0x7FFFFFFF) return fail_in(fn, "need fewer than 2^31 items");
    if (pairs > 65535) return fail_in(fn, "pairs > 65535");
    if (h_count > 0x3FFFFFFF || !grid_fits(h_count, kFitBlock, kFitBlock, pairs) || !grid_fits(h_count, kScoreBlock, kScoreBlock, pairs, 2))
        return fail_in(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail_in(fn, "unknown aggregation");
    if (h_begin < 0) return fail_in(fn, "negative h_begin");
    if (pairs == 0) return SFM_OK;
    if (!offset || !min_extra || !h_result || !e_result || !verdict || (n_total > 0 && (!corr || !h_mask || !e_mask)) ||
        (h_count > 0 && (!S || !H || !E || !h_flags || !h_cnt || !h_s1 || !h_s2 || !e_flags || !e_cnt || !e_s1 || !e_s2)))
        return fail_in(fn, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Corr* items = (const Corr*)corr;
    hipLaunchKernelGGL(offsets_check_kernel, dim3(1), dim3(kCheckBlock), 0, st, offset, pairs, n_total, verdict);
    if (h_count > 0) {
        const dim3 fit_grid(grid_for(h_count, kFitBlock), (unsigned)pairs);
        hipLaunchKernelGGL(ragged_fit_kernel<false>, fit_grid, dim3(kFitBlock), 0, st, items, offset, verdict, seed, seed_stride, h_begin,
                           h_count, S, H, h_flags);
        hipLaunchKernelGGL(ragged_fit_kernel<true>, fit_grid, dim3(kFitBlock), 0, st, items, offset, verdict, seed, seed_stride, h_begin,
                           h_count, S, E, e_flags);
        hipLaunchKernelGGL(ragged_score_kernel, dim3(grid_for(h_count, kScoreBlock), (unsigned)pairs, 2), dim3(kScoreBlock), 0, st, items,
                           offset, verdict, S, H, E, h_count, thr, h_cnt, h_s1, h_s2, e_cnt, e_s1, e_s2);
    }
    hipLaunchKernelGGL(ragged_select_kernel, dim3((unsigned)pairs, 2), dim3(kSelectBlock), 0, st, h_cnt, h_s1, h_s2, h_flags, e_cnt, e_s1,
                       e_s2, e_flags, h_count, min_extra, aggregation, h_result, e_result);
    if (n_total > 0)
        hipLaunchKernelGGL(ragged_mask_kernel, dim3(grid_stride(n_total, 256, 1024)), dim3(256), 0, st, items, n_total, offset, pairs, verdict,
                           S, H, E, h_count, h_result, e_result, thr, h_mask, e_mask);
    hipLaunchKernelGGL(verdict_kernel, dim3(grid_for(pairs, 256)), dim3(256), 0, st, h_result, e_result, pairs, max_ratio, verdict);
    return check_launch(fn);
}

}  // extern "C"
