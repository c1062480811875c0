// Relative pose and triangulation angle of every pair of a match graph, chained behind sfm_verify_pairs
// (sfm_view_graph.hip) on that call's buffers: per pair the four poses of its winning essential matrix, the cheirality vote of
// its inliers (the items with e_mask != 0, all of them), the winning pose and the lower median of the angle between the two
// viewing rays of the items that pass under it.  The decomposition is sfmdec::decompose_essential (sfm_decompose.h, the body of
// sfm_decompose_essential); the solve and test, the chunk compaction and the vote are those of sfm_cheirality.h.
//
// Three launches whatever the number of pairs, nothing read back:
//   1. pose_decompose_kernel    one lane per pair: status, the four candidates (workspace), the filler of a pair without a pose
//   2. pose_cheirality_kernel   one walk over the N items, a wave per chunk of 512: an item finds its pair by bisection, the wave
//                               compacts its chunk to the inliers of pairs with candidates (ballot + mbcnt into an LDS list) and
//                               runs two DLT solves per inlier, each serving an antipodal pair of poses: 4 pass bits per item;
//                               every item's angle is set to NaN
//   3. pose_vote_median_kernel  one block per pair: the four votes, the first maximum, the angle of every passing item under the
//                               winning rotation (workspace), and the item of rank (k - 1) / 2 among those k angles by a most-
//                               significant-digit radix select on their bit patterns (angles are >= 0: bit order is value order):
//                               eight passes of 8-bit digits, a 256-bin LDS histogram with integer LDS atomics and a scan
// The DLT solve owns a launch because it dominates registers.  No global atomics, no floating-point atomics: the histogram
// counts are integers, so a call is reproducible bit for bit.  Nothing is indexed through an offset table that was refused.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_cheirality.h"
#include "sfm_common.h"
#include "sfm_decompose.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"

static_assert(sizeof(sfm_pair_pose) == 128, "sfm_pair_pose is 128 bytes");

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_for;

using sfmchi::kChunk;                 // items per wave in the cheirality walk
constexpr int kCheiralityBlock = 256;
constexpr int kMedianBlock = 256;     // one thread per bin of the digit histogram
constexpr int kCandidateDoubles = 48; // four poses of R (9) | t (3)

// The regions of the workspace: the angle of every item first (the documented part), then the candidates and the pass bits.
struct Regions {
    double* angle;      // [n_total]
    double* candidates; // [pairs, 4, 12]
    uint8_t* pass;      // [n_total] bit p: the item passes under candidate p
};
inline int64_t pass_bytes(int64_t n_total) { return (n_total + 7) / 8 * 8; }
inline int64_t workspace_bytes(int64_t n_total, int64_t pairs) {
    return 8 * n_total + 8 * kCandidateDoubles * pairs + pass_bytes(n_total);
}
inline Regions regions(void* workspace, int64_t n_total, int64_t pairs) {
    double* base = (double*)workspace;
    return Regions{base, base + n_total, (uint8_t*)(base + n_total + kCandidateDoubles * pairs)};
}

SFM_DEVICE void write_filler(sfm_pair_pose* __restrict__ out, int status) {
    sfm_pair_pose p;
#pragma unroll
    for (int k = 0; k < 9; ++k) p.R[k] = NAN;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.t[k] = NAN;
    p.median_angle = NAN;
#pragma unroll
    for (int k = 0; k < 4; ++k) p.votes[k] = 0;
    p.best = -1;
    p.status = status;
    *out = p;
}

// One lane per pair.  A pair without an essential winner decomposes a fixed essential matrix (every lane of the wave must run
// the sweeps) and stores nothing of it.  A pair with candidates gets status SFM_POSE_OK here and the rest of its record from
// pose_vote_median_kernel; every other pair gets its whole record here.
__global__ __launch_bounds__(kWave) void pose_decompose_kernel(const double* __restrict__ E, int64_t h_count,
                                                               const sfm_select_result* __restrict__ e_result,
                                                               const sfm_pair_verdict* __restrict__ verdict, int64_t pairs,
                                                               double* __restrict__ candidates, sfm_pair_pose* __restrict__ pose) {
    const int64_t q_raw = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool active = q_raw < pairs;
    const int64_t q = active ? q_raw : pairs - 1;
    const bool bad = verdict[q].kind == SFM_PAIR_BAD_OFFSETS;
    const int64_t eb = e_result[q].best_h;
    const bool have = !bad && eb >= 0 && eb < h_count;
    double e[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};   // [t]x of t = (1, 0, 0)
    if (have) {
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = E[(q * h_count + eb) * 9 + k];
    }
    int32_t st = 0;
    sfmdec::decompose_essential(e, active && have, candidates + q * kCandidateDoubles, &st);
    if (!active) return;
    const int status = bad ? SFM_POSE_BAD_OFFSETS : (!have ? SFM_POSE_NO_MODEL : (st != 0 ? SFM_POSE_NOT_ESSENTIAL : SFM_POSE_OK));
    if (status != SFM_POSE_OK) write_filler(pose + q, status);
    else pose[q].status = SFM_POSE_OK;
}

// The cheirality test (sfm_cheirality.h) over the concatenated items: an item is solved when its pair has candidates and its
// e_mask is not 0.  The decomposition writes candidates 2k and 2k + 1 as an antipodal pair, so two solves decide all four.
__global__ __launch_bounds__(kCheiralityBlock) void pose_cheirality_kernel(const Corr* __restrict__ corr, int64_t n_total,
                                                                           const int64_t* __restrict__ offset, int64_t pairs,
                                                                           const sfm_pair_verdict* __restrict__ verdict,
                                                                           const uint8_t* __restrict__ e_mask,
                                                                           const sfm_pair_pose* __restrict__ pose,
                                                                           const double* __restrict__ candidates,
                                                                           double distance_threshold, uint8_t* __restrict__ pass,
                                                                           double* __restrict__ angle) {
    __shared__ int32_t list[kCheiralityBlock / kWave][kChunk];   // (pair << 9) | position in the chunk; pair <= 65534
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int64_t base = ((int64_t)blockIdx.x * (kCheiralityBlock / kWave) + wave) * kChunk;
    if (base >= n_total) return;   // whole wave; no block-level barrier below
    const bool bad = verdict[0].kind == SFM_PAIR_BAD_OFFSETS;
    const int total = sfmchi::compact_chunk<kChunk>(list[wave], lane, [&](int position, int32_t& entry) {
        const int64_t i = base + position;
        const bool inside = i < n_total;
        const int64_t q = (inside && !bad) ? pair_of_item(offset, pairs, i) : -1;
        const bool act = q >= 0 && pose[q].status == SFM_POSE_OK && e_mask[i] != 0;
        if (inside) {
            angle[i] = NAN;
            if (!act) pass[i] = 0;
        }
        entry = (int32_t)(q << 9) | position;
        return act;
    });
    for (int j = 0; j < total; j += kWave) {
        bool active;
        const int32_t entry = sfmchi::group_entry(list[wave], j, lane, total, active);
        const int64_t i = base + (entry & (kChunk - 1));
        const double* __restrict__ cand = candidates + (int64_t)(entry >> 9) * kCandidateDoubles;
        const Corr p = corr[i];
        unsigned bits = 0;
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {   // candidates 0 and 2: (R1, t), (R2, t)
            const sfmchi::Cheirality c = sfmchi::cheirality_test(cand + k * 24, p, distance_threshold);
            bits |= (c.ok ? 1u : 0u) << (2 * k) | (c.mirrored ? 1u : 0u) << (2 * k + 1);
        }
        if (active) pass[i] = (uint8_t)bits;
    }
}

// The angle between the viewing rays a = (xa, ya, 1) and R^T (xb, yb, 1), every operation rounded on its own.
SFM_DEVICE double ray_angle(const double* R, const Corr& p) {
    double c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = (R[0 + j] * p.xb + R[3 + j] * p.yb) + R[6 + j] * 1.0;
    const double w0 = p.ya * c[2] - 1.0 * c[1];
    const double w1 = 1.0 * c[0] - p.xa * c[2];
    const double w2 = p.xa * c[1] - p.ya * c[0];
    const double n = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double d = (p.xa * c[0] + p.ya * c[1]) + 1.0 * c[2];
    return atan2(n, d);
}

// One block per pair with candidates.  Thread t visits items first + t, first + t + 256, ... in every loop below, so it reads
// back only angles it stored itself.
__global__ __launch_bounds__(kMedianBlock) void pose_vote_median_kernel(const Corr* __restrict__ corr, int64_t n_total,
                                                                        const int64_t* __restrict__ offset,
                                                                        const double* __restrict__ candidates,
                                                                        const uint8_t* __restrict__ pass, double* __restrict__ angle,
                                                                        sfm_pair_pose* __restrict__ pose) {
    __shared__ int partial[kMedianBlock / kWave][4];
    __shared__ int hist[256];
    __shared__ int chosen[2];   // the bin holding the rank, and the rank within that bin
    const int64_t q = blockIdx.x;
    if (pose[q].status != SFM_POSE_OK) return;   // block-uniform: its record is complete
    // within [0, n_total] whatever the table holds (a table sfm_verify_pairs accepted is)
    int64_t first = offset[q], last = offset[q + 1];
    first = first < 0 ? 0 : (first > n_total ? n_total : first);
    last = last < first ? first : (last > n_total ? n_total : last);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    int cnt[4] = {0, 0, 0, 0};
    for (int64_t i = first + threadIdx.x; i < last; i += kMedianBlock) {
        const int b = pass[i];
#pragma unroll
        for (int p = 0; p < 4; ++p) cnt[p] += (b >> p) & 1;
    }
    int votes[4], best, top;
    sfmchi::block_votes(cnt, partial, votes);
    sfmchi::first_maximum(votes, best, top);
    if (best < 0) {   // block-uniform
        if (threadIdx.x == 0) write_filler(pose + q, SFM_POSE_NO_VOTE);
        return;
    }
    double rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) rt[k] = candidates[q * kCandidateDoubles + best * 12 + k];
    for (int64_t i = first + threadIdx.x; i < last; i += kMedianBlock)
        if ((pass[i] >> best) & 1) angle[i] = ray_angle(rt, corr[i]);
    // radix select of the key of rank (top - 1) / 2 among the top passing items, most significant digit first
    int rank = (top - 1) / 2;
    uint64_t prefix = 0;
#pragma unroll 1
    for (int digit = 0; digit < 8; ++digit) {
        const int shift = 56 - 8 * digit;
        hist[threadIdx.x] = 0;
        if (threadIdx.x < 2) chosen[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t i = first + threadIdx.x; i < last; i += kMedianBlock) {
            if (((pass[i] >> best) & 1) == 0) continue;
            const uint64_t key = (uint64_t)__double_as_longlong(angle[i]);
            const uint64_t above = digit == 0 ? 0 : key >> (shift + 8);
            if (above == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (wave == 0) {   // lane l owns bins 4 l .. 4 l + 3; an inclusive scan of the lanes' sums finds the lane holding the rank
            int c[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[k] = hist[4 * lane + k];
                sum += c[k];
            }
            int inclusive = sum;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const int up = __shfl_up(inclusive, d);
                if (lane >= d) inclusive += up;
            }
            int r = rank - (inclusive - sum);
            if (r >= 0 && rank < inclusive) {
                int bin = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (bin == k && r >= c[k]) {
                        r -= c[k];
                        bin = k + 1;
                    }
                }
                chosen[0] = 4 * lane + bin;
                chosen[1] = r;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint64_t)chosen[0];
        rank = chosen[1];
        __syncthreads();   // chosen is reset by the next pass
    }
    if (threadIdx.x == 0) {
        sfm_pair_pose p;
#pragma unroll
        for (int k = 0; k < 9; ++k) p.R[k] = rt[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) p.t[k] = rt[9 + k];
        p.median_angle = __longlong_as_double((long long)prefix);
#pragma unroll
        for (int k = 0; k < 4; ++k) p.votes[k] = votes[k];
        p.best = best;
        p.status = SFM_POSE_OK;
        pose[q] = p;
    }
}

}  // namespace

extern "C" {

int64_t sfm_pair_poses_workspace_bytes(int64_t n_total, int64_t pairs) {
    if (n_total < 0 || pairs < 0 || n_total > 0x7FFFFFFF || pairs > 65535) return -1;
    return workspace_bytes(n_total, pairs);
}

int sfm_pair_poses(const double* corr, int64_t n_total, const int64_t* offset, int64_t pairs, const double* E, int64_t h_count,
                   const sfm_select_result* e_result, const uint8_t* e_mask, const sfm_pair_verdict* verdict,
                   double distance_threshold, sfm_pair_pose* pose, void* workspace, int64_t workspace_bytes_given, void* stream) {
    const char* fn = "sfm_pair_poses";
    if (n_total < 0 || pairs < 0) return fail_in(fn, "negative size");
    if (n_total > 0x7FFFFFFF) return fail_in(fn, "need fewer than 2^31 items");
    if (pairs > 65535) return fail_in(fn, "pairs > 65535");
    if (h_count < 1 || h_count > 0x3FFFFFFF) return fail_in(fn, "h_count must be in [1, 2^30)");
    if (pairs == 0) return SFM_OK;
    if (!offset || !E || !e_result || !verdict || !pose || !workspace || (n_total > 0 && (!corr || !e_mask)))
        return fail_in(fn, "null pointer");
    if (workspace_bytes_given < workspace_bytes(n_total, pairs)) return fail_in(fn, "workspace too small (sfm_pair_poses_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const Corr* items = (const Corr*)corr;
    const Regions ws = regions(workspace, n_total, pairs);
    hipLaunchKernelGGL(pose_decompose_kernel, dim3(grid_for(pairs, kWave)), dim3(kWave), 0, st, E, h_count, e_result, verdict, pairs,
                       ws.candidates, pose);
    if (n_total > 0)
        hipLaunchKernelGGL(pose_cheirality_kernel, dim3(grid_for(n_total, kChunk * (kCheiralityBlock / kWave))),
                           dim3(kCheiralityBlock), 0, st, items, n_total, offset, pairs, verdict, e_mask, pose, ws.candidates,
                           distance_threshold, ws.pass, ws.angle);
    hipLaunchKernelGGL(pose_vote_median_kernel, dim3((unsigned)pairs), dim3(kMedianBlock), 0, st, items, n_total, offset, ws.candidates,
                       ws.pass, ws.angle, pose);
    return check_launch(fn);
}

}  // extern "C"
