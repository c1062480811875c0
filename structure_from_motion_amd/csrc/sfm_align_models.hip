// Similarity alignment of every overlapping pair of sub-models in one call: the RANSAC pass and the refinement
// of its winner for each pair, over the pairs' concatenated 3-D / 3-D items ("ragged": pair q owns items
// offset[q] .. offset[q+1]-1, any count per pair).  Pair q's outputs are what sfm_similarity_ransac_pass(seed + q * seed_stride,
// use_philox = 1, thr[q], min_extra[q]) with a mask, followed by sfm_similarity_refine on its winner, give on that pair alone:
// the solver, the error and the mask model (sfm_similarity.h), the scoring loop (sfm_minimal_score.h), the selection
// (sfmsel::block_select) and the reduction passes of the refinement (sfm_similarity_reduce.h) are the same device routines.
//
// 7 + 4 * refine_rounds launches whatever the number of pairs, nothing read back:
//   1. align_offsets_kernel   the offset table is non-decreasing within [0, N] and no pair has more than max_items items, or
//                             every status is SFM_ALIGN_BAD_OFFSETS; the later launches read that mark before the table and then
//                             treat every pair as empty, so nothing is indexed by it
//   2. align_fit_kernel       grid (h / 64, pairs): one hypothesis per lane, draws the Philox sample, fills S, the three-item fit
//   3. align_score_kernel     grid (h / 256, pairs): one hypothesis per lane, the pair's items staged through LDS in tiles of
//                             512 (24 KiB), the sample items corrected after the tile loop
//   4. align_select_kernel    grid (pairs): sfmsel::block_select with the pair's own min_extra, sample size 3
//   5. align_mask_kernel      the winners' masks, a grid-stride walk over all N items (an item finds its pair by bisection);
//                             both masks of an item no pair owns are 0
//   6. align_begin_kernel     the start of the refinement, or the filler of a pair without a winner
//   7. per round: align_sums_kernel, align_moments_kernel, align_score_round_kernel, align_accept_kernel
//   8. align_end_kernel       grid (pairs): the record and the status
// The launches of 6 and 7 have the grid (blocks_for(max_items), pairs); pair q is reduced by its first blocks_for(n_q) blocks
// with the walk of a launch of that many, and a block beyond them returns at once, so its partial records and their order are
// those of the single-pair call.  A pair with fewer than 3 items gets the filler: rows of S all -1, models of 13 NaNs, flags
// SFM_FIT_DEGENERATE, cnt 0, s1 = s2 = NaN, and so a record without a winner whose n_flagged is h_count.  Every sum runs in a
// fixed order: no atomics, and a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_select.h"
#include "sfm_similarity.h"
#include "sfm_similarity_reduce.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_fits;
using sfmhost::grid_for;
using sfmhost::grid_stride;
using sfmmin::kScoreBlock;
using sfmsim::blocks_for;
using sfmsim::kMoments;
using sfmsim::kScores;
using sfmsim::kSimilarityModel;
using sfmsim::kSimilaritySample;
using sfmsim::kSums;
using sfmsim::RefineState;
using sfmsim::similarity_model;
using sfmsim::SimPair;

constexpr int kFitBlock = sfmmin::kMinimalFitBlock;
constexpr int kSelectBlock = 1024;
constexpr int kCheckBlock = 1024;
constexpr int kBlock = sfmsim::kReduceBlock;

// The items of pair q: none when the offset table was refused (the table itself always holds pairs + 1 entries).
struct PairItems {
    const SimPair* P;
    int64_t first, n;
};
SFM_DEVICE PairItems pair_items(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                const int32_t* __restrict__ status, int64_t q) {
    const bool bad = status[q] == SFM_ALIGN_BAD_OFFSETS;
    const int64_t lo = bad ? 0 : offset[q], hi = bad ? 0 : offset[q + 1];
    return PairItems{items + lo, lo, hi - lo};
}

// The winner of pair q, or -1: what the launches behind the selection refine.
SFM_DEVICE int64_t winner_of(const sfm_select_result* __restrict__ result, int64_t q, int64_t n, int64_t h_count) {
    const int64_t best = result[q].best_h;
    return (n >= kSimilaritySample && best >= 0 && best < h_count) ? best : -1;
}

// The slots of a workspace: `records` partial records per pair (blocks_for(max_items)), pair q's own at the front of its share.
struct Workspace {
    double *part1, *part2, *part0, *part3, *trial;
    int32_t* trial_flag;
    RefineState* state;   // [2, pairs]
    int64_t records, bytes;
};

Workspace carve(void* base, int64_t pairs, int64_t max_items) {
    sfmhost::Carver c{(uintptr_t)base, 0};
    Workspace w{};
    w.records = blocks_for(max_items);
    const int64_t records = pairs * w.records;
    w.part1 = c.take<double>(records * kSums);
    w.part2 = c.take<double>(records * kMoments);
    w.part0 = c.take<double>(records);
    w.part3 = c.take<double>(records * kScores);
    w.trial = c.take<double>(pairs * kSimilarityModel);
    w.trial_flag = c.take<int32_t>(pairs);
    w.state = c.take<RefineState>(2 * pairs);
    w.bytes = c.at;
    return w;
}

bool sizes_ok(int64_t n_total, int64_t pairs, int64_t max_items) {
    return n_total >= 0 && n_total <= 0x7FFFFFFF && pairs >= 0 && pairs <= 65535 && max_items >= 0 && max_items <= n_total;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One block: 0 <= offset[0] <= offset[1] <= ... <= offset[pairs] <= n_total and every n_q <= max_items, or every status
// SFM_ALIGN_BAD_OFFSETS.  The status of a pair of an accepted table is written by align_end_kernel.
__global__ __launch_bounds__(kCheckBlock) void align_offsets_kernel(const int64_t* __restrict__ offset, int64_t pairs, int64_t n_total,
                                                                    int64_t max_items, int32_t* __restrict__ status) {
    bool ok = true;
    for (int64_t k = threadIdx.x; k <= pairs; k += kCheckBlock) {
        const int64_t v = offset[k];
        ok = ok && v >= 0 && v <= n_total && (k == 0 || (offset[k - 1] <= v && v - offset[k - 1] <= max_items));
    }
    const int mark = __syncthreads_and(ok ? 1 : 0) ? SFM_ALIGN_OK : SFM_ALIGN_BAD_OFFSETS;
    for (int64_t q = threadIdx.x; q < pairs; q += kCheckBlock) status[q] = mark;
}

// sfmmin::minimal_fit_kernel<similarity_solver, true> over the pair's own items: draws the sample and stores its row of S.
__global__ __launch_bounds__(kFitBlock) void align_fit_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                              const int32_t* __restrict__ status, uint64_t seed, uint64_t seed_stride,
                                                              int64_t h_begin, int64_t h_count, int32_t* __restrict__ S,
                                                              double* __restrict__ model, int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * kFitBlock + threadIdx.x;
    if (h >= h_count) return;
    const int64_t q = blockIdx.y;
    const int64_t qh = q * h_count + h;
    const PairItems p = pair_items(items, offset, status, q);
    if (p.n < kSimilaritySample) {   // the filler of a pair too small for a sample
#pragma unroll
        for (int i = 0; i < kSimilarityModel; ++i) model[qh * kSimilarityModel + i] = NAN;
        flags[qh] = SFM_FIT_DEGENERATE;
#pragma unroll
        for (int i = 0; i < 8; ++i) S[qh * 8 + i] = -1;
        return;
    }
    int32_t idx[8];
    sfm::philox_sample8(seed + (uint64_t)q * seed_stride, (uint64_t)(h_begin + h), (uint32_t)p.n, idx);
#pragma unroll
    for (int i = kSimilaritySample; i < 8; ++i) idx[i] = i < p.n ? idx[i] : -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) S[qh * 8 + i] = idx[i];
    double out[kSimilarityModel];
    const int flag = sfmsim::similarity_solver::fit(p.P, 0, p.n, idx, out);
#pragma unroll
    for (int i = 0; i < kSimilarityModel; ++i) model[qh * kSimilarityModel + i] = out[i];
    flags[qh] = flag;
}

// One hypothesis per lane over its pair's items: sfmmin::score_hypothesis with the lane's model, its row of S and thr[q].
__global__ __launch_bounds__(kScoreBlock) void align_score_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                                  const int32_t* __restrict__ status, const double* __restrict__ thr,
                                                                  const double* __restrict__ model, const int32_t* __restrict__ S,
                                                                  int64_t h_count, int32_t* __restrict__ cnt, double* __restrict__ s1,
                                                                  double* __restrict__ s2) {
    __shared__ SimPair tile[sfmmin::kScoreTile];
    const int64_t q = blockIdx.y;
    const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    const PairItems p = pair_items(items, offset, status, q);   // uniform over the block, like everything tested before a barrier
    if (p.n < kSimilaritySample) {
        if (h < h_count) {
            cnt[q * h_count + h] = 0;
            s1[q * h_count + h] = NAN;
            s2[q * h_count + h] = NAN;
        }
        return;
    }
    const int64_t hc = h < h_count ? h : h_count - 1;   // lanes past the end score a valid hypothesis and store nothing
    const int64_t qh = q * h_count + hc;
    const sfmmin::HypothesisScore r = sfmmin::score_hypothesis<kSimilaritySample>(tile, similarity_model(model + qh * kSimilarityModel),
                                                                                  p.P, p.n, S + qh * 8, thr[q]);
    if (h < h_count) {
        cnt[q * h_count + h] = r.c;
        s1[q * h_count + h] = r.a1;
        s2[q * h_count + h] = r.a2;
    }
}

// The per-pair form of the selection: block q runs the one definition of sfm_select.h over pair q's h_count rows with
// min_extra[q].
__global__ __launch_bounds__(kSelectBlock) void align_select_kernel(const int32_t* __restrict__ cnt, const double* __restrict__ s1,
                                                                    const double* __restrict__ s2, const int32_t* __restrict__ flags,
                                                                    int64_t h_count, const double* __restrict__ min_extra, int aggregation,
                                                                    sfm_select_result* __restrict__ result) {
    __shared__ sfmsel::SelectScratch<kSelectBlock> scratch;
    __shared__ int64_t winner;
    const int64_t q = blockIdx.x, first = q * h_count;
    sfmsel::block_select<kSelectBlock>(cnt + first, s1 + first, s2 + first, flags + first, h_count, 0, min_extra[q], aggregation,
                                       result + q, scratch, &winner, kSimilaritySample);
}

// The winner's mask of every item: 2 for the sample items of the pair's winner, 1 for its other items within the threshold, 0
// otherwise, and 0 for an item no pair owns or whose pair has no winner.  mask_out of an item no pair owns is 0 as well (the
// others are written by their pair's blocks of align_begin_kernel).
__global__ void align_mask_kernel(const SimPair* __restrict__ items, int64_t n_total, const int64_t* __restrict__ offset, int64_t pairs,
                                  const int32_t* __restrict__ status, const double* __restrict__ thr, const int32_t* __restrict__ S,
                                  const double* __restrict__ model, int64_t h_count, const sfm_select_result* __restrict__ result,
                                  uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_out) {
    const bool bad = status[0] == SFM_ALIGN_BAD_OFFSETS;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        const int64_t q = bad ? -1 : pair_of_item(offset, pairs, i);
        uint8_t m = 0;
        if (q >= 0) {
            const int64_t best = winner_of(result, q, offset[q + 1] - offset[q], h_count);
            if (best >= 0) {
                const int64_t qh = q * h_count + best;
                m = sfmmin::mask_value<kSimilaritySample>(similarity_model(model + qh * kSimilarityModel), S + qh * 8, items[i],
                                                          i - offset[q], thr[q]);
            }
        } else {
            mask_out[i] = 0;
        }
        mask[i] = m;
    }
}

// What the blocks of the refinement's launches share: the pair of the block, its items, its block count and its slots.
struct PairBlock {
    PairItems p;
    int64_t q;
    int blocks, block;   // block >= blocks: nothing to do
};
SFM_DEVICE PairBlock pair_block(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                const int32_t* __restrict__ status) {
    const int64_t q = blockIdx.y;
    const PairItems p = pair_items(items, offset, status, q);
    return PairBlock{p, q, blocks_for(p.n), (int)blockIdx.x};
}

// The start of the refinement of pair q from its winner's row (sfmsim::refine_begin_block), or, without a winner, the filler:
// model_out 13 NaNs, the pair's mask_out bytes 0 and a closed state.
__global__ __launch_bounds__(kBlock) void align_begin_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                             const int32_t* __restrict__ status, const double* __restrict__ model,
                                                             int64_t h_count, const sfm_select_result* __restrict__ result,
                                                             const uint8_t* __restrict__ mask, double* __restrict__ model_out,
                                                             uint8_t* __restrict__ mask_out, double* __restrict__ part0,
                                                             RefineState* __restrict__ state) {
    const PairBlock k = pair_block(items, offset, status);
    if (k.block >= k.blocks) return;   // block-uniform
    const int64_t best = winner_of(result, k.q, k.p.n, h_count);
    if (best < 0) {   // block-uniform
        const int64_t stride = (int64_t)k.blocks * kBlock;
        for (int64_t i = (int64_t)k.block * kBlock + threadIdx.x; i < k.p.n; i += stride) mask_out[k.p.first + i] = 0;
        if (k.block == 0) {
            if (threadIdx.x < kSimilarityModel) model_out[k.q * kSimilarityModel + threadIdx.x] = NAN;
            if (threadIdx.x == 0) state[k.q] = RefineState{INFINITY, 0.0, 0, 0, 0, 0};
        }
        return;
    }
    sfmsim::refine_begin_block(k.p.n, k.blocks, k.block, model + (k.q * h_count + best) * kSimilarityModel, mask + k.p.first,
                               &result[k.q].best_err, model_out + k.q * kSimilarityModel, mask_out + k.p.first,
                               part0 + k.q * gridDim.x, state + k.q);
}

__global__ __launch_bounds__(kBlock) void align_sums_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                            const int32_t* __restrict__ status, const uint8_t* __restrict__ mask_out,
                                                            const RefineState* __restrict__ gate, double* __restrict__ part1) {
    const PairBlock k = pair_block(items, offset, status);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::sums_block(k.p.P, k.p.n, k.blocks, k.block, mask_out + k.p.first, gate + k.q, part1 + k.q * gridDim.x * kSums);
}

__global__ __launch_bounds__(kBlock) void align_moments_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                               const int32_t* __restrict__ status, const uint8_t* __restrict__ mask_out,
                                                               const RefineState* __restrict__ gate, const double* __restrict__ part1,
                                                               double* __restrict__ part2) {
    const PairBlock k = pair_block(items, offset, status);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::moments_block(k.p.P, k.p.n, k.blocks, k.block, mask_out + k.p.first, gate + k.q, part1 + k.q * gridDim.x * kSums,
                          part2 + k.q * gridDim.x * kMoments);
}

__global__ __launch_bounds__(kBlock) void align_score_round_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                                   const int32_t* __restrict__ status, const double* __restrict__ thr,
                                                                   const RefineState* __restrict__ gate, const double* __restrict__ part1,
                                                                   const double* __restrict__ part2, double* __restrict__ trial,
                                                                   int32_t* __restrict__ trial_flag, double* __restrict__ part3) {
    const PairBlock k = pair_block(items, offset, status);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::refine_score_block(k.p.P, k.p.n, k.blocks, k.block, gate + k.q, part1 + k.q * gridDim.x * kSums,
                               part2 + k.q * gridDim.x * kMoments, thr[k.q], trial + k.q * kSimilarityModel, trial_flag + k.q,
                               part3 + k.q * gridDim.x * kScores);
}

__global__ __launch_bounds__(kBlock) void align_accept_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                              const int32_t* __restrict__ status, const double* __restrict__ thr,
                                                              const RefineState* __restrict__ state_in, RefineState* __restrict__ state_out,
                                                              const double* __restrict__ part1, const double* __restrict__ part3,
                                                              const double* __restrict__ trial, const int32_t* __restrict__ trial_flag,
                                                              int aggregation, double* __restrict__ model_out,
                                                              uint8_t* __restrict__ mask_out) {
    const PairBlock k = pair_block(items, offset, status);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::refine_accept_block(k.p.P, k.p.n, k.blocks, k.block, state_in + k.q, state_out + k.q, part1 + k.q * gridDim.x * kSums,
                                part3 + k.q * gridDim.x * kScores, trial + k.q * kSimilarityModel, trial_flag + k.q, thr[k.q],
                                aggregation, model_out + k.q * kSimilarityModel, mask_out + k.p.first);
}

// One wave per pair: the record of the refinement (sfmsim::refine_end_entry), or {+inf, 0, 0, 0, 0} without a winner, and the
// status.
__global__ __launch_bounds__(kWave) void align_end_kernel(const int64_t* __restrict__ offset, int64_t h_count,
                                                          const sfm_select_result* __restrict__ result,
                                                          const RefineState* __restrict__ state, const double* __restrict__ part0,
                                                          int64_t records, sfm_similarity_refine_info* __restrict__ info,
                                                          int32_t* __restrict__ status) {
    const int64_t q = blockIdx.x;
    const bool bad = status[q] == SFM_ALIGN_BAD_OFFSETS;   // read by every thread before thread 0 replaces it below
    const int64_t n = bad ? 0 : offset[q + 1] - offset[q];
    const int64_t best = winner_of(result, q, n, h_count);   // block-uniform
    __syncthreads();
    if (best < 0) {
        if (threadIdx.x == 0) {
            sfm_similarity_refine_info r;
            r.error = INFINITY;
            r.count = r.accepted = r.rounds_run = r.reserved = 0;
            info[q] = r;
            status[q] = bad ? SFM_ALIGN_BAD_OFFSETS : (n < kSimilaritySample ? SFM_ALIGN_TOO_FEW : SFM_ALIGN_NO_MODEL);
        }
        return;
    }
    sfmsim::refine_end_entry(state + q, part0 + q * records, blocks_for(n), info + q);
    if (threadIdx.x == 0) status[q] = SFM_ALIGN_OK;
}

}  // namespace

extern "C" {

int64_t sfm_align_models_workspace_bytes(int64_t n_total, int64_t pairs, int64_t max_items) {
    return sizes_ok(n_total, pairs, max_items) ? carve(nullptr, pairs, max_items).bytes : -1;
}

int sfm_align_models(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pairs, int64_t n_total, const int64_t* offset,
                     int64_t pair_count, int64_t max_items, const double* thr, const double* min_extra, int64_t h_count,
                     int aggregation, int refine_rounds, int32_t* S, double* model, int32_t* flags, int32_t* cnt, double* s1, double* s2,
                     sfm_select_result* result, uint8_t* mask, double* model_out, uint8_t* mask_out, sfm_similarity_refine_info* info,
                     int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "sfm_align_models";
    // every check before the first launch: a refused call has enqueued nothing
    if (n_total < 0 || pair_count < 0 || max_items < 0 || refine_rounds < 0) return fail_in(fn, "negative size");
    if (n_total > 0x7FFFFFFF) return fail_in(fn, "need fewer than 2^31 items");
    if (pair_count > 65535) return fail_in(fn, "pairs > 65535");
    if (max_items > n_total) return fail_in(fn, "max_items exceeds n_total");
    if (h_count < 1) return fail_in(fn, "need at least one hypothesis per pair");
    if (h_count > 0x3FFFFFFF || !grid_fits(h_count, kFitBlock, kFitBlock, pair_count) ||
        !grid_fits(h_count, kScoreBlock, kScoreBlock, pair_count))
        return fail_in(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail_in(fn, "unknown aggregation");
    if (h_begin < 0) return fail_in(fn, "negative h_begin");
    if (pair_count == 0) return SFM_OK;
    if (!offset || !thr || !min_extra || !S || !model || !flags || !cnt || !s1 || !s2 || !result || !model_out || !info || !status ||
        !workspace || (n_total > 0 && (!pairs || !mask || !mask_out)))
        return fail_in(fn, "null pointer");
    if (!aligned16(pairs) || !aligned16(workspace)) return fail_in(fn, "pairs and workspace must be 16-byte aligned");
    if (mask != nullptr && mask == mask_out) return fail_in(fn, "mask_out must not alias mask");
    const Workspace w = carve(workspace, pair_count, max_items);
    if (workspace_bytes < w.bytes) return fail_in(fn, "workspace too small (sfm_align_models_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const SimPair* items = (const SimPair*)pairs;
    const unsigned Q = (unsigned)pair_count;
    hipLaunchKernelGGL(align_offsets_kernel, dim3(1), dim3(kCheckBlock), 0, st, offset, pair_count, n_total, max_items, status);
    hipLaunchKernelGGL(align_fit_kernel, dim3(grid_for(h_count, kFitBlock), Q), dim3(kFitBlock), 0, st, items, offset, status, seed,
                       seed_stride, h_begin, h_count, S, model, flags);
    hipLaunchKernelGGL(align_score_kernel, dim3(grid_for(h_count, kScoreBlock), Q), dim3(kScoreBlock), 0, st, items, offset, status, thr,
                       model, S, h_count, cnt, s1, s2);
    hipLaunchKernelGGL(align_select_kernel, dim3(Q), dim3(kSelectBlock), 0, st, cnt, s1, s2, flags, h_count, min_extra, aggregation,
                       result);
    hipLaunchKernelGGL(align_mask_kernel, dim3(grid_stride(n_total, 256, 1024)), dim3(256), 0, st, items, n_total, offset, pair_count,
                       status, thr, S, model, h_count, result, mask, mask_out);
    const dim3 grid((unsigned)w.records, Q);
    hipLaunchKernelGGL(align_begin_kernel, grid, dim3(kBlock), 0, st, items, offset, status, model, h_count, result, mask, model_out,
                       mask_out, w.part0, w.state);
    for (int round = 0; round < refine_rounds; ++round) {
        const RefineState* now = w.state + (round & 1) * pair_count;
        RefineState* next = w.state + ((round + 1) & 1) * pair_count;
        hipLaunchKernelGGL(align_sums_kernel, grid, dim3(kBlock), 0, st, items, offset, status, mask_out, now, w.part1);
        hipLaunchKernelGGL(align_moments_kernel, grid, dim3(kBlock), 0, st, items, offset, status, mask_out, now,
                           (const double*)w.part1, w.part2);
        hipLaunchKernelGGL(align_score_round_kernel, grid, dim3(kBlock), 0, st, items, offset, status, thr, now, (const double*)w.part1,
                           (const double*)w.part2, w.trial, w.trial_flag, w.part3);
        hipLaunchKernelGGL(align_accept_kernel, grid, dim3(kBlock), 0, st, items, offset, status, thr, now, next, (const double*)w.part1,
                           (const double*)w.part3, (const double*)w.trial, (const int32_t*)w.trial_flag, aggregation, model_out,
                           mask_out);
    }
    hipLaunchKernelGGL(align_end_kernel, dim3(Q), dim3(kWave), 0, st, offset, h_count, result,
                       (const RefineState*)(w.state + (refine_rounds & 1) * pair_count), (const double*)w.part0, w.records, info,
                       status);
    return check_launch(fn);
}

}  // extern "C"
