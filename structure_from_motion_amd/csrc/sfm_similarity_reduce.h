// The reduction passes of the masked similarity fit and of the refinement of a winner as device routines, one
// block's share of one entry each: what the dense kernels of sfm_similarity.hip (entry b of a [batch, n] layout) and the ragged
// ones of sfm_align_models.hip (pair q of an offset table) both wrap, moved here unchanged from
// sfm_similarity.hip so that both run the same operations in the same order.
//
// Every routine takes the entry's own item pointer and n, the entry's block count `blocks` and this block's index `block` in
// [0, blocks), and the entry's own slots of the workspace (its `blocks` partial records, its trial model, its state).  The walk
// over the items is the grid-stride one of a launch of `blocks` blocks, whatever the grid of the launch is: each block leaves
// one partial record, and every consumer adds the records in block order, so the sums have one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_math.h"
#include "sfm_similarity.h"

namespace sfmsim {

constexpr int kReduceBlock = 256;
constexpr int kReduceWaves = kReduceBlock / kWave;
constexpr int kItemsPerBlock = 2048;   // below this an entry's reduction is one block
constexpr int kMaxBlocks = 128;        // partial records per entry at most
constexpr int kSums = 7;               // sum a (3) | sum b (3) | count
constexpr int kMoments = 11;           // M (9) | sa2 | sb2
constexpr int kScores = 3;             // count | sum e | sum e^2

// The blocks (and partial records) of an entry of n items: it depends on n alone.
__host__ __device__ inline int blocks_for(int64_t n) {
    const int64_t g = (n + kItemsPerBlock - 1) / kItemsPerBlock;
    return (int)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

// What a refinement carries from round to round, per entry; double-buffered, so that the blocks of a launch read one copy
// while block 0 writes the other.
struct RefineState {
    double err;       // aggregated error of the model kept so far
    double cnt;       // its inlier count; < 0: not counted yet (no round has run)
    int32_t active;   // 0 once a round stopped early or was rejected
    int32_t accepted, rounds_run, pad;
};
static_assert(sizeof(RefineState) == 32, "two doubles and four words");

// The sum over an entry's `blocks` partial records of K doubles, in block order, into total (LDS, K doubles): valid for every
// thread after the call.
template <int K>
SFM_DEVICE void fold_partials(const double* __restrict__ partial, int blocks, double* total) {
    if (threadIdx.x < K) {
        double acc = partial[threadIdx.x];
        for (int j = 1; j < blocks; ++j) acc += partial[(int64_t)j * K + threadIdx.x];
        total[threadIdx.x] = acc;
    }
    __syncthreads();
}

// The means of the set from the folded sums: mu = sum / count.
SFM_DEVICE void centroids(const double* sums, double (&mua)[3], double (&mub)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mua[k] = sums[k] / sums[6];
        mub[k] = sums[3 + k] / sums[6];
    }
}

// The model of the set whose folded sums and moments are given (LDS): sfmsim::solve, the solve of the minimal fit.
SFM_DEVICE int model_of(const double* sums, const double* moments, double (&out)[kSimilarityModel]) {
    Moments mo;
    centroids(sums, mo.mua, mo.mub);
#pragma unroll
    for (int k = 0; k < 9; ++k) mo.M[k] = moments[k];
    mo.sa2 = moments[9];
    mo.sb2 = moments[10];
    return solve(mo, out);
}

// ---- pass 1: sum a, sum b and the count of the set `m` (null: every item), this block's partial record into part1 [blocks, 7];
// nothing for an entry whose `gate` (null: none) is not active ------------------------------------------------------------
SFM_DEVICE void sums_block(const SimPair* __restrict__ P, int64_t n, int blocks, int block, const uint8_t* __restrict__ m,
                           const RefineState* __restrict__ gate, double* __restrict__ part1) {
    __shared__ double part[kReduceWaves * kSums];
    __shared__ double total[kSums];
    if (gate != nullptr && !gate->active) return;   // block-uniform
    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    const int64_t stride = (int64_t)blocks * kReduceBlock;
    for (int64_t i = (int64_t)block * kReduceBlock + threadIdx.x; i < n; i += stride) {
        if (m != nullptr && m[i] == 0) continue;
        const SimPair q = P[i];
        v[0] += q.ax; v[1] += q.ay; v[2] += q.az;
        v[3] += q.bx; v[4] += q.by; v[5] += q.bz;
        v[6] += 1.0;
    }
    sfm::block_sum<kSums, kReduceBlock>(v, part, total);
    if (threadIdx.x < kSums) part1[(int64_t)block * kSums + threadIdx.x] = total[threadIdx.x];
}

// ---- pass 2: the centred moments about the centroid of pass 1, this block's partial record into part2 [blocks, 11] ---------
SFM_DEVICE void moments_block(const SimPair* __restrict__ P, int64_t n, int blocks, int block, const uint8_t* __restrict__ m,
                              const RefineState* __restrict__ gate, const double* __restrict__ part1, double* __restrict__ part2) {
    __shared__ double part[kReduceWaves * kMoments];
    __shared__ double total[kMoments];
    __shared__ double sums[kSums];
    if (gate != nullptr && !gate->active) return;   // block-uniform
    fold_partials<kSums>(part1, blocks, sums);
    double mua[3], mub[3];
    centroids(sums, mua, mub);
    double v[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) v[k] = 0.0;
    const int64_t stride = (int64_t)blocks * kReduceBlock;
    for (int64_t i = (int64_t)block * kReduceBlock + threadIdx.x; i < n; i += stride) {
        if (m != nullptr && m[i] == 0) continue;
        const SimPair q = P[i];
        const double da[3] = {q.ax - mua[0], q.ay - mua[1], q.az - mua[2]};
        const double db[3] = {q.bx - mub[0], q.by - mub[1], q.bz - mub[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 * r + k] += db[r] * da[k];
        v[9] += (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
        v[10] += (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
    }
    sfm::block_sum<kMoments, kReduceBlock>(v, part, total);
    if (threadIdx.x < kMoments) part2[(int64_t)block * kMoments + threadIdx.x] = total[threadIdx.x];
}

// ---- refinement: the start.  mask_out = (mask_in != 0), its count per block into part0 [blocks]; block 0 copies the model and
// opens the state with the error at err_in ----------------------------------------------------------------------------------
SFM_DEVICE void refine_begin_block(int64_t n, int blocks, int block, const double* __restrict__ model_in,
                                   const uint8_t* __restrict__ mask_in, const double* __restrict__ err_in,
                                   double* __restrict__ model_out, uint8_t* __restrict__ mask_out, double* __restrict__ part0,
                                   RefineState* __restrict__ state) {
    __shared__ double part[kReduceWaves];
    __shared__ double total[1];
    double v[1] = {0.0};
    const int64_t stride = (int64_t)blocks * kReduceBlock;
    for (int64_t i = (int64_t)block * kReduceBlock + threadIdx.x; i < n; i += stride) {
        const uint8_t m = mask_in[i] != 0 ? 1 : 0;
        mask_out[i] = m;
        v[0] += (double)m;
    }
    sfm::block_sum<1, kReduceBlock>(v, part, total);
    if (threadIdx.x == 0) part0[block] = total[0];
    if (block == 0) {
        if (threadIdx.x < kSimilarityModel) model_out[threadIdx.x] = model_in[threadIdx.x];
        if (threadIdx.x == 0) *state = RefineState{*err_in, -1.0, 1, 0, 0, 0};
    }
}

// ---- refinement: the model of the current inliers (every block solves it; block 0 leaves it in `trial`) and the re-score of
// every item under it, this block's partial record into part3 [blocks, 3] ---------------------------------------------------
SFM_DEVICE void refine_score_block(const SimPair* __restrict__ P, int64_t n, int blocks, int block,
                                   const RefineState* __restrict__ gate, const double* __restrict__ part1,
                                   const double* __restrict__ part2, double thr, double* __restrict__ trial,
                                   int32_t* __restrict__ trial_flag, double* __restrict__ part3) {
    __shared__ double part[kReduceWaves * kScores];
    __shared__ double total[kScores];
    __shared__ double sums[kSums];
    __shared__ double moments[kMoments];
    if (!gate->active) return;   // block-uniform
    fold_partials<kSums>(part1, blocks, sums);
    fold_partials<kMoments>(part2, blocks, moments);
    double m[kSimilarityModel];
    const int flag = model_of(sums, moments, m);
    if (block == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSimilarityModel; ++k) trial[k] = m[k];
        *trial_flag = flag;
    }
    if (!(sums[6] >= (double)kSimilaritySample) || flag != 0) return;   // block-uniform: the round stops in the accept routine
    double c[kScores] = {0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)blocks * kReduceBlock;
    for (int64_t i = (int64_t)block * kReduceBlock + threadIdx.x; i < n; i += stride) {
        const double e = pair_error(m, P[i]);
        if (e <= thr) {
            c[0] += 1.0;
            c[1] += e;
            c[2] += e * e;
        }
    }
    sfm::block_sum<kScores, kReduceBlock>(c, part, total);
    if (threadIdx.x < kScores) part3[(int64_t)block * kScores + threadIdx.x] = total[threadIdx.x];
}

// ---- refinement: the accept rule (sfmfit::refit_wins), decided alike by every block from the same records;
// a kept round rewrites the mask, and block 0 moves the model and the state on -----------------------------------------------
SFM_DEVICE void refine_accept_block(const SimPair* __restrict__ P, int64_t n, int blocks, int block,
                                    const RefineState* __restrict__ state_in, RefineState* __restrict__ state_out,
                                    const double* __restrict__ part1, const double* __restrict__ part3,
                                    const double* __restrict__ trial, const int32_t* __restrict__ trial_flag, double thr,
                                    int aggregation, double* __restrict__ model_out, uint8_t* __restrict__ mask_out) {
    __shared__ double sums[kSums];
    __shared__ double scores[kScores];
    const bool writer = block == 0 && threadIdx.x == 0;
    const RefineState st = *state_in;
    if (!st.active) {   // block-uniform
        if (writer) *state_out = st;
        return;
    }
    fold_partials<kSums>(part1, blocks, sums);
    const double current = sums[6];
    const bool enough = current >= (double)kSimilaritySample;
    if (!enough || *trial_flag != 0) {   // block-uniform: fewer than three inliers, or a degenerate set
        if (writer) *state_out = RefineState{st.err, current, 0, st.accepted, st.rounds_run + (enough ? 1 : 0), 0};
        return;
    }
    fold_partials<kScores>(part3, blocks, scores);
    const double cnt = scores[0];
    const double err = sfmfit::aggregate_error(aggregation, (int)cnt, scores[1], scores[2], 0);
    if (!sfmfit::refit_wins(cnt, err, current, st.err)) {   // block-uniform
        if (writer) *state_out = RefineState{st.err, current, 0, st.accepted, st.rounds_run + 1, 0};
        return;
    }
    double m[kSimilarityModel];
#pragma unroll
    for (int k = 0; k < kSimilarityModel; ++k) m[k] = trial[k];
    const int64_t stride = (int64_t)blocks * kReduceBlock;
    for (int64_t i = (int64_t)block * kReduceBlock + threadIdx.x; i < n; i += stride)
        mask_out[i] = pair_error(m, P[i]) <= thr ? 1 : 0;
    if (block == 0 && threadIdx.x < kSimilarityModel) model_out[threadIdx.x] = m[threadIdx.x];
    if (writer) *state_out = RefineState{err, cnt, 1, st.accepted + 1, st.rounds_run + 1, 0};
}

// ---- refinement: the record of an entry from its last state and the counts of the start; one wave ---------------------------
SFM_DEVICE void refine_end_entry(const RefineState* __restrict__ state, const double* __restrict__ part0, int blocks,
                                 sfm_similarity_refine_info* __restrict__ info) {
    __shared__ double counted[1];
    fold_partials<1>(part0, blocks, counted);
    if (threadIdx.x == 0) {
        const RefineState st = *state;
        sfm_similarity_refine_info r;
        r.error = st.err;
        r.count = (int32_t)(st.cnt < 0.0 ? counted[0] : st.cnt);
        r.accepted = st.accepted;
        r.rounds_run = st.rounds_run;
        r.reserved = 0;
        *info = r;
    }
}

}  // namespace sfmsim
