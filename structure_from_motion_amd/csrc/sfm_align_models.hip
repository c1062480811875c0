// Similarity alignment of every overlapping pair of sub-models in one call: the RANSAC pass and the refinement
// of its winner for each pair, over the pairs' concatenated 3-D / 3-D items ("ragged": pair q owns items
// offset[q] .. offset[q+1]-1, any count per pair).  Pair q's outputs are what sfm_similarity_ransac_pass(seed + q * seed_stride,
// use_philox = 1, thr[q], min_extra[q]) with a mask, followed by sfm_similarity_refine on its winner, give on that pair alone:
// the solver, the error and the mask model (sfm_similarity.h), the scoring loop (sfm_minimal_score.h), the selection
// (sfmsel::block_select) and the reduction passes of the refinement (sfm_similarity_reduce.h) are the same device routines.
//
// 7 + 4 * refine_rounds launches whatever the number of pairs, nothing read back; the first five are the ragged pass of
// sfm_ragged_pass.h:
//   1. sfmrag::ragged_offsets_kernel   the offset table is non-decreasing within [0, N] and no pair has more than max_items
//                                      items, or every status is SFM_ALIGN_BAD_OFFSETS; the later launches read that mark before
//                                      the table and then treat every pair as empty, so nothing is indexed by it
//   2. sfmrag::ragged_fit_kernel<similarity_solver, true>   grid (h / 64, pairs): one hypothesis per lane, draws the Philox
//                                      sample, fills S, the three-item fit
//   3. sfmrag::ragged_score_kernel     grid (h / 256, pairs): one hypothesis per lane, the pair's items staged through LDS in
//                                      tiles of 512 (24 KiB), the sample items corrected after the tile loop
//   4. sfmrag::ragged_select_kernel<3> grid (pairs): sfmsel::block_select with the pair's own min_extra
//   5. sfmrag::ragged_mask_kernel      the winners' masks, a grid-stride walk over all N items (an item finds its pair by
//                                      bisection); both masks of an item no pair owns are 0
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
#include "sfm_ragged_pass.h"
#include "sfm_similarity.h"
#include "sfm_similarity_reduce.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_for;
using sfmhost::grid_stride;
using sfmrag::Mark;
using sfmrag::Range;
using sfmsim::blocks_for;
using sfmsim::kMoments;
using sfmsim::kScores;
using sfmsim::kSimilarityModel;
using sfmsim::kSimilaritySample;
using sfmsim::kSums;
using sfmsim::RefineState;
using sfmsim::similarity_model;
using sfmsim::SimPair;

constexpr int kBlock = sfmsim::kReduceBlock;
using Scorer = sfmrag::model_scorer<kSimilaritySample, similarity_model>;   // sfmmin::score_hypothesis with thr[q]

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

// What the blocks of the refinement's launches share: the pair of the block, its items, its block count and its slots.
struct PairBlock {
    const SimPair* P;
    int64_t first, n, q;
    int blocks, block;   // block >= blocks: nothing to do
};
SFM_DEVICE PairBlock pair_block(const SimPair* __restrict__ items, const int64_t* __restrict__ offset, const Mark& mark) {
    const int64_t q = blockIdx.y;
    const Range r = sfmrag::range_of(offset, mark, q);
    return PairBlock{items + r.first, r.first, r.n, q, blocks_for(r.n), (int)blockIdx.x};
}

// The start of the refinement of pair q from its winner's row (sfmsim::refine_begin_block), or, without a winner, the filler:
// model_out 13 NaNs, the pair's mask_out bytes 0 and a closed state.
__global__ __launch_bounds__(kBlock) void align_begin_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                             Mark mark, const double* __restrict__ model, int64_t h_count,
                                                             const sfm_select_result* __restrict__ result,
                                                             const uint8_t* __restrict__ mask, double* __restrict__ model_out,
                                                             uint8_t* __restrict__ mask_out, double* __restrict__ part0,
                                                             RefineState* __restrict__ state) {
    const PairBlock k = pair_block(items, offset, mark);
    if (k.block >= k.blocks) return;   // block-uniform
    const int64_t best = sfmrag::winner_of<kSimilaritySample>(result, k.q, k.n, h_count);
    if (best < 0) {   // block-uniform
        const int64_t stride = (int64_t)k.blocks * kBlock;
        for (int64_t i = (int64_t)k.block * kBlock + threadIdx.x; i < k.n; i += stride) mask_out[k.first + i] = 0;
        if (k.block == 0) {
            if (threadIdx.x < kSimilarityModel) model_out[k.q * kSimilarityModel + threadIdx.x] = NAN;
            if (threadIdx.x == 0) state[k.q] = RefineState{INFINITY, 0.0, 0, 0, 0, 0};
        }
        return;
    }
    sfmsim::refine_begin_block(k.n, k.blocks, k.block, model + (k.q * h_count + best) * kSimilarityModel, mask + k.first,
                               &result[k.q].best_err, model_out + k.q * kSimilarityModel, mask_out + k.first,
                               part0 + k.q * gridDim.x, state + k.q);
}

__global__ __launch_bounds__(kBlock) void align_sums_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                            Mark mark, const uint8_t* __restrict__ mask_out,
                                                            const RefineState* __restrict__ gate, double* __restrict__ part1) {
    const PairBlock k = pair_block(items, offset, mark);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::sums_block(k.P, k.n, k.blocks, k.block, mask_out + k.first, gate + k.q, part1 + k.q * gridDim.x * kSums);
}

__global__ __launch_bounds__(kBlock) void align_moments_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                               Mark mark, const uint8_t* __restrict__ mask_out,
                                                               const RefineState* __restrict__ gate, const double* __restrict__ part1,
                                                               double* __restrict__ part2) {
    const PairBlock k = pair_block(items, offset, mark);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::moments_block(k.P, k.n, k.blocks, k.block, mask_out + k.first, gate + k.q, part1 + k.q * gridDim.x * kSums,
                          part2 + k.q * gridDim.x * kMoments);
}

__global__ __launch_bounds__(kBlock) void align_score_round_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                                   Mark mark, const double* __restrict__ thr,
                                                                   const RefineState* __restrict__ gate, const double* __restrict__ part1,
                                                                   const double* __restrict__ part2, double* __restrict__ trial,
                                                                   int32_t* __restrict__ trial_flag, double* __restrict__ part3) {
    const PairBlock k = pair_block(items, offset, mark);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::refine_score_block(k.P, k.n, k.blocks, k.block, gate + k.q, part1 + k.q * gridDim.x * kSums,
                               part2 + k.q * gridDim.x * kMoments, thr[k.q], trial + k.q * kSimilarityModel, trial_flag + k.q,
                               part3 + k.q * gridDim.x * kScores);
}

__global__ __launch_bounds__(kBlock) void align_accept_kernel(const SimPair* __restrict__ items, const int64_t* __restrict__ offset,
                                                              Mark mark, const double* __restrict__ thr,
                                                              const RefineState* __restrict__ state_in, RefineState* __restrict__ state_out,
                                                              const double* __restrict__ part1, const double* __restrict__ part3,
                                                              const double* __restrict__ trial, const int32_t* __restrict__ trial_flag,
                                                              int aggregation, double* __restrict__ model_out,
                                                              uint8_t* __restrict__ mask_out) {
    const PairBlock k = pair_block(items, offset, mark);
    if (k.block >= k.blocks) return;   // block-uniform
    sfmsim::refine_accept_block(k.P, k.n, k.blocks, k.block, state_in + k.q, state_out + k.q, part1 + k.q * gridDim.x * kSums,
                                part3 + k.q * gridDim.x * kScores, trial + k.q * kSimilarityModel, trial_flag + k.q, thr[k.q],
                                aggregation, model_out + k.q * kSimilarityModel, mask_out + k.first);
}

// One wave per pair: the record of the refinement (sfmsim::refine_end_entry), or {+inf, 0, 0, 0, 0} without a winner, and the
// status.
__global__ __launch_bounds__(kWave) void align_end_kernel(const int64_t* __restrict__ offset, int64_t h_count,
                                                          const sfm_select_result* __restrict__ result,
                                                          const RefineState* __restrict__ state, const double* __restrict__ part0,
                                                          int64_t records, sfm_similarity_refine_info* __restrict__ info,
                                                          int32_t* __restrict__ status) {
    const int64_t q = blockIdx.x;
    const Mark mark{status, 1};
    const bool bad = mark.bad(q);   // read by every thread before thread 0 replaces it below
    const int64_t n = sfmrag::range_of(offset, mark, q).n;
    const int64_t best = sfmrag::winner_of<kSimilaritySample>(result, q, n, h_count);   // block-uniform
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
    const int rc = sfmrag::check_sizes(fn, n_total, pair_count, h_count, 1, 1, aggregation, h_begin, {max_items, refine_rounds});
    if (rc != SFM_OK) return rc;
    if (max_items > n_total) return fail_in(fn, "max_items exceeds n_total");
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
    const Mark mark{status, 1};
    const sfmrag::RangeThreshold gate{thr};
    hipLaunchKernelGGL(sfmrag::ragged_offsets_kernel, dim3(1), dim3(sfmrag::kCheckBlock), 0, st, offset, pair_count, n_total, max_items,
                       mark, SFM_ALIGN_OK);
    hipLaunchKernelGGL((sfmrag::ragged_fit_kernel<sfmsim::similarity_solver, true>), dim3(grid_for(h_count, sfmrag::kFitBlock), Q),
                       dim3(sfmrag::kFitBlock), 0, st, items, offset, mark, seed, seed_stride, h_begin, h_count, S, model, flags);
    hipLaunchKernelGGL((sfmrag::ragged_score_kernel<Scorer, sfmrag::RangeThreshold>), dim3(grid_for(h_count, sfmrag::kScoreBlock), Q),
                       dim3(sfmrag::kScoreBlock), 0, st, items, offset, mark, (const double*)model, (const int32_t*)S, h_count, gate, cnt,
                       s1, s2);
    hipLaunchKernelGGL(sfmrag::ragged_select_kernel<kSimilaritySample>, dim3(Q), dim3(sfmrag::kSelectBlock), 0, st, (const int32_t*)cnt,
                       (const double*)s1, (const double*)s2, (const int32_t*)flags, h_count, min_extra, aggregation, result);
    hipLaunchKernelGGL((sfmrag::ragged_mask_kernel<kSimilaritySample, similarity_model, sfmrag::RangeThreshold>),
                       dim3(grid_stride(n_total, sfmrag::kMaskBlock, sfmrag::kMaskBlocks)), dim3(sfmrag::kMaskBlock), 0, st, items, n_total,
                       offset, pair_count, mark, (const int32_t*)S, (const double*)model, h_count, (const sfm_select_result*)result, gate,
                       mask, mask_out);
    const dim3 grid((unsigned)w.records, Q);
    hipLaunchKernelGGL(align_begin_kernel, grid, dim3(kBlock), 0, st, items, offset, mark, model, h_count, result, mask, model_out,
                       mask_out, w.part0, w.state);
    for (int round = 0; round < refine_rounds; ++round) {
        const RefineState* now = w.state + (round & 1) * pair_count;
        RefineState* next = w.state + ((round + 1) & 1) * pair_count;
        hipLaunchKernelGGL(align_sums_kernel, grid, dim3(kBlock), 0, st, items, offset, mark, mask_out, now, w.part1);
        hipLaunchKernelGGL(align_moments_kernel, grid, dim3(kBlock), 0, st, items, offset, mark, mask_out, now,
                           (const double*)w.part1, w.part2);
        hipLaunchKernelGGL(align_score_round_kernel, grid, dim3(kBlock), 0, st, items, offset, mark, thr, now, (const double*)w.part1,
                           (const double*)w.part2, w.trial, w.trial_flag, w.part3);
        hipLaunchKernelGGL(align_accept_kernel, grid, dim3(kBlock), 0, st, items, offset, mark, thr, now, next, (const double*)w.part1,
                           (const double*)w.part3, (const double*)w.trial, (const int32_t*)w.trial_flag, aggregation, model_out,
                           mask_out);
    }
    hipLaunchKernelGGL(align_end_kernel, dim3(Q), dim3(kWave), 0, st, offset, h_count, result,
                       (const RefineState*)(w.state + (refine_rounds & 1) * pair_count), (const double*)w.part0, w.records, info,
                       status);
    return check_launch(fn);
}

}  // extern "C"
