// The RANSAC pass of the ragged calls (sfm_view_graph.hip, sfm_register_views.hip, sfm_align_models.hip): what
// sfm_minimal_fit.h and sfm_minimal_score.h hold for the dense layout, over concatenated items of which range q owns
// offset[q] .. offset[q+1]-1.  The offset table comes from the caller's device memory unread by the host, so the first launch
// checks it and marks every range of a refused table; every later launch reads the mark before the table (range_of) and then
// treats every range as empty: nothing is indexed through a refused table.
//
// Besides the concepts of those two headers, a scorer is a struct with
//   kSample, kModel, Stored, kStride   as in the solver and the model;
//   Tile                               what one LDS tile slot holds;
//   score(tile, items, n, model, sample_row, thr, params...)   device function: the HypothesisScore of one lane, called by
//                                      every lane of the block with the same items and n.
// The kernels are static: each of the three translation units launches its own copies, and a kernel that nothing outside
// can name loses the LDS slot of the selection's winner, which no ragged launch reads back, as the kernels it replaces did.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_select.h"

namespace sfmrag {

using sfmmin::kScoreBlock;
constexpr int kFitBlock = sfmmin::kMinimalFitBlock;
constexpr int kSelectBlock = 1024;
constexpr int kCheckBlock = 1024;
constexpr int kMaskBlock = 256, kMaskBlocks = 1024;

static_assert(SFM_PAIR_BAD_OFFSETS == SFM_REGISTER_BAD_OFFSETS && SFM_REGISTER_BAD_OFFSETS == SFM_ALIGN_BAD_OFFSETS,
              "one code marks a refused offset table in the three ragged calls");
constexpr int32_t kBadOffsets = SFM_PAIR_BAD_OFFSETS;

// Where the mark of range q lives: the int32 at word[q * stride] — status[q] (stride 1), or the kind of a verdict record
// (its first field, stride 6).
struct Mark {
    int32_t* word;
    int64_t stride;
    SFM_DEVICE bool bad(int64_t q) const { return word[q * stride] == kBadOffsets; }
};

// The items of range q: none when the offset table was refused (the table itself always holds ranges + 1 entries).  The only
// reader of a range's own offset entries.
struct Range {
    int64_t first, n;
};
SFM_DEVICE Range range_of(const int64_t* __restrict__ offset, const Mark& mark, int64_t q) {
    const bool bad = mark.bad(q);
    const int64_t lo = bad ? 0 : offset[q], hi = bad ? 0 : offset[q + 1];
    return Range{lo, hi - lo};
}

// The threshold of range q: one for the call, or the range's own.
struct CallThreshold {
    double thr;
    SFM_DEVICE double of(int64_t) const { return thr; }
};
struct RangeThreshold {
    const double* thr;
    SFM_DEVICE double of(int64_t q) const { return thr[q]; }
};

// The winner of range q, or -1: what the launches behind the selection read.  A range too small for a sample has none (its
// record says so as well: the filler's best_h is -1).
template <int SAMPLE>
SFM_DEVICE int64_t winner_of(const sfm_select_result* __restrict__ result, int64_t q, int64_t n, int64_t h_count) {
    const int64_t best = result[q].best_h;
    return (n >= SAMPLE && best >= 0 && best < h_count) ? best : -1;
}

// One block: 0 <= offset[0] <= offset[1] <= ... <= offset[ranges] <= n_total and no range longer than max_items, or every
// mark kBadOffsets; `accepted` is what a range of an accepted table is stamped with.  A call without a cap passes
// max_items = n_total: entries within [0, n_total] cannot differ by more, so the test never fails there.
static __global__ __launch_bounds__(kCheckBlock) void ragged_offsets_kernel(const int64_t* __restrict__ offset, int64_t ranges,
                                                                            int64_t n_total, int64_t max_items, Mark mark,
                                                                            int32_t accepted) {
    bool ok = true;
    for (int64_t k = threadIdx.x; k <= ranges; k += kCheckBlock) {
        const int64_t v = offset[k];
        ok = ok && v >= 0 && v <= n_total && (k == 0 || (offset[k - 1] <= v && v - offset[k - 1] <= max_items));
    }
    const int32_t stamp = __syncthreads_and(ok ? 1 : 0) ? accepted : kBadOffsets;
    for (int64_t q = threadIdx.x; q < ranges; q += kCheckBlock) mark.word[q * mark.stride] = stamp;
}

// sfmmin::minimal_fit_kernel<Solver, true> with range blockIdx.y in place of a batch entry: one hypothesis per lane, its sample
// philox_sample8(seed + q * seed_stride, h_begin + h) over the range's n items.  OWNS_S: the row of S receives all eight, with
// -1 at the positions past the sample that are >= n; otherwise the same sample is drawn again for a second model and S is left
// alone.  A range smaller than the sample gets the filler: a model of NaNs, SFM_FIT_DEGENERATE and (OWNS_S) a row of -1.
// Each solver is a kernel of its own, so a solver that needs every register does not set the allocation of the others.
template <class Solver, bool OWNS_S>
static __global__ __launch_bounds__(kFitBlock) void ragged_fit_kernel(typename Solver::Data data, const int64_t* __restrict__ offset,
                                                                      Mark mark, uint64_t seed, uint64_t seed_stride, int64_t h_begin,
                                                                      int64_t h_count, int32_t* __restrict__ S, double* __restrict__ model,
                                                                      int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * kFitBlock + threadIdx.x;
    if (h >= h_count) return;
    const int64_t q = blockIdx.y;
    const int64_t qh = q * h_count + h;
    const Range r = range_of(offset, mark, q);
    if (r.n < Solver::kSample) {
#pragma unroll
        for (int i = 0; i < Solver::kModel; ++i) model[qh * Solver::kModel + i] = NAN;
        flags[qh] = SFM_FIT_DEGENERATE;
        if constexpr (OWNS_S) {
#pragma unroll
            for (int i = 0; i < 8; ++i) S[qh * 8 + i] = -1;
        }
        return;
    }
    int32_t idx[8];
    sfm::philox_sample8(seed + (uint64_t)q * seed_stride, (uint64_t)(h_begin + h), (uint32_t)r.n, idx);
    if constexpr (OWNS_S) {
#pragma unroll
        for (int i = Solver::kSample; i < 8; ++i) idx[i] = i < r.n ? idx[i] : -1;
#pragma unroll
        for (int i = 0; i < 8; ++i) S[qh * 8 + i] = idx[i];
    }
    double out[Solver::kModel];
    const int flag = Solver::fit(Solver::from(data, r.first), 0, r.n, idx, out);
#pragma unroll
    for (int i = 0; i < Solver::kModel; ++i) model[qh * Solver::kModel + i] = out[i];
    flags[qh] = flag;
}

// The scorer of a `Model` of sfm_minimal_score.h: sfmmin::score_hypothesis.
template <int SAMPLE, class Model>
struct model_scorer {
    static constexpr int kSample = SAMPLE, kModel = Model::kModel, kStride = Model::kStride;
    using Stored = typename Model::Stored;
    using Tile = typename Model::Item;
    template <class... Params>
    SFM_DEVICE static sfmmin::HypothesisScore score(Tile* tile, const Stored* items, int64_t n, const double* model,
                                                    const int32_t* sample_row, double thr, Params... params) {
        return sfmmin::score_hypothesis<SAMPLE>(tile, Model(model, params...), items, n, sample_row, thr);
    }
};

// One block of a score launch, grid x over the hypotheses: one hypothesis per lane over the items of range q.  A range smaller
// than the sample gets the filler (cnt 0, s1 = s2 = NaN).  `r` and q are uniform over the block, like everything tested before
// a barrier.
template <class Scorer, class... Params>
SFM_DEVICE void score_block(typename Scorer::Tile* tile, const typename Scorer::Stored* __restrict__ items, const Range& r, int64_t q,
                            const double* __restrict__ model, const int32_t* __restrict__ S, int64_t h_count, double thr,
                            int32_t* __restrict__ cnt, double* __restrict__ s1, double* __restrict__ s2, Params... params) {
    const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    if (r.n < Scorer::kSample) {
        if (h < h_count) {
            cnt[q * h_count + h] = 0;
            s1[q * h_count + h] = NAN;
            s2[q * h_count + h] = NAN;
        }
        return;
    }
    const int64_t hc = h < h_count ? h : h_count - 1;   // lanes past the end score a valid hypothesis and store nothing
    const int64_t qh = q * h_count + hc;
    const sfmmin::HypothesisScore s = Scorer::score(tile, items + r.first * Scorer::kStride, r.n, model + qh * Scorer::kModel, S + qh * 8,
                                                    thr, params...);
    if (h < h_count) {
        cnt[q * h_count + h] = s.c;
        s1[q * h_count + h] = s.a1;
        s2[q * h_count + h] = s.a2;
    }
}

// The score of one model: grid (h / 256, ranges).
template <class Scorer, class Threshold, class... Params>
static __global__ __launch_bounds__(kScoreBlock) void ragged_score_kernel(const typename Scorer::Stored* __restrict__ items,
                                                                          const int64_t* __restrict__ offset, Mark mark,
                                                                          const double* __restrict__ model, const int32_t* __restrict__ S,
                                                                          int64_t h_count, Threshold thr, int32_t* __restrict__ cnt,
                                                                          double* __restrict__ s1, double* __restrict__ s2,
                                                                          Params... params) {
    __shared__ typename Scorer::Tile tile[sfmmin::kScoreTile];
    const int64_t q = blockIdx.y;
    score_block<Scorer>(tile, items, range_of(offset, mark, q), q, model, S, h_count, thr.of(q), cnt, s1, s2, params...);
}

// The selection of range blockIdx.x: the one definition of sfm_select.h over the range's h_count rows with min_extra[q].
SFM_DEVICE void select_block(int sample, const int32_t* __restrict__ cnt, const double* __restrict__ s1, const double* __restrict__ s2,
                             const int32_t* __restrict__ flags, int64_t h_count, const double* __restrict__ min_extra, int aggregation,
                             sfm_select_result* __restrict__ result, sfmsel::SelectScratch<kSelectBlock>& scratch, int64_t* winner) {
    const int64_t q = blockIdx.x, first = q * h_count;
    sfmsel::block_select<kSelectBlock>(cnt + first, s1 + first, s2 + first, flags + first, h_count, 0, min_extra[q], aggregation,
                                       result + q, scratch, winner, sample);
}

template <int SAMPLE>
static __global__ __launch_bounds__(kSelectBlock) void ragged_select_kernel(const int32_t* __restrict__ cnt, const double* __restrict__ s1,
                                                                            const double* __restrict__ s2,
                                                                            const int32_t* __restrict__ flags, int64_t h_count,
                                                                            const double* __restrict__ min_extra, int aggregation,
                                                                            sfm_select_result* __restrict__ result) {
    __shared__ sfmsel::SelectScratch<kSelectBlock> scratch;
    __shared__ int64_t winner;
    select_block(SAMPLE, cnt, s1, s2, flags, h_count, min_extra, aggregation, result, scratch, &winner);
}

// The mask value of item i (of all items) under the winner of range q, which owns it: 2 for a sample item, 1 for another item
// within the threshold, 0 otherwise and without a winner.
template <int SAMPLE, class Model, class... Params>
SFM_DEVICE uint8_t winner_mask_value(const typename Model::Stored* __restrict__ items, int64_t i, const int64_t* __restrict__ offset,
                                     const Mark& mark, int64_t q, const int32_t* __restrict__ S, const double* __restrict__ model,
                                     int64_t h_count, const sfm_select_result* __restrict__ result, double thr, Params... params) {
    const Range r = range_of(offset, mark, q);
    const int64_t best = winner_of<SAMPLE>(result, q, r.n, h_count);
    if (best < 0) return 0;
    const int64_t qh = q * h_count + best;
    typename Model::Item item;
    Model::load(items, i, item);
    return sfmmin::mask_value<SAMPLE>(Model(model + qh * Model::kModel, params...), S + qh * 8, item, i - r.first, thr);
}

// The winner's mask of every item, a grid-stride walk over all n_total items (an item finds its range by bisection): 0 for an
// item no range owns, and mask_out — the mask a refinement writes range by range — of such an item is 0 as well.
template <int SAMPLE, class Model, class Threshold, class... Params>
static __global__ void ragged_mask_kernel(const typename Model::Stored* __restrict__ items, int64_t n_total,
                                          const int64_t* __restrict__ offset, int64_t ranges, Mark mark, const int32_t* __restrict__ S,
                                          const double* __restrict__ model, int64_t h_count,
                                          const sfm_select_result* __restrict__ result, Threshold thr, uint8_t* __restrict__ mask,
                                          uint8_t* __restrict__ mask_out, Params... params) {
    const bool bad = mark.bad(0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        const int64_t q = bad ? -1 : pair_of_item(offset, ranges, i);
        uint8_t m = 0;
        if (q >= 0) m = winner_mask_value<SAMPLE, Model>(items, i, offset, mark, q, S, model, h_count, result, thr.of(q), params...);
        else mask_out[i] = 0;
        mask[i] = m;
    }
}

// What the three entry points check about their sizes, all of it before the first launch: none negative (`others`: the
// caller's further sizes), fewer than 2^31 items, at most 65535 ranges, min_h <= h_count (0 where a call without hypotheses
// is a selection over zero rows, else 1), the grids of the fit and of the score of `score_models` models, the aggregation
// and h_begin.
inline int check_sizes(const char* fn, int64_t n_total, int64_t ranges, int64_t h_count, int64_t min_h, int score_models, int aggregation,
                       int64_t h_begin, std::initializer_list<int64_t> others = {}) {
    using sfmhost::fail_in;
    bool negative = n_total < 0 || ranges < 0 || (min_h == 0 && h_count < 0);
    for (const int64_t v : others) negative = negative || v < 0;
    if (negative) return fail_in(fn, "negative size");
    if (n_total > 0x7FFFFFFF) return fail_in(fn, "need fewer than 2^31 items");
    if (ranges > 65535) return fail_in(fn, "more than 65535 ranges");
    if (h_count < min_h) return fail_in(fn, "need at least one hypothesis per range");
    if (h_count > 0x3FFFFFFF || !sfmhost::grid_fits(h_count, kFitBlock, kFitBlock, ranges) ||
        !sfmhost::grid_fits(h_count, kScoreBlock, kScoreBlock, ranges, score_models))
        return fail_in(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail_in(fn, "unknown aggregation");
    if (h_begin < 0) return fail_in(fn, "negative h_begin");
    return SFM_OK;
}

}  // namespace sfmrag
