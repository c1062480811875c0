// Batched, device-resident pose selection and triangulation for many image pairs (BASELINE.json
// config "256 image pairs x 10k correspondences: E-estimation + cheirality + triangulation end-to-end
// on GPU").  These entry points chain after sfm_select_best / sfm_inlier_mask without a host round
// trip; together they are the device form of reference eight_point.py:181-242 (_recover_r_t) and
// triangulation.py:42-62 (triangulate_points) applied to the RANSAC inliers, as apps/sfm.py:110-186 does.
// The test, the chunk compaction and the vote are those of sfm_cheirality.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_cheirality.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_for;

// Cheirality test (sfm_cheirality.h) of every correspondence of every pair under its 4 candidate poses.  Points whose inlier
// mask is 0 are reported as not passing — and cost nothing: each wave first compacts the inliers of its 512-point chunk, then
// runs the DLT solves only on full 64-lane groups of inliers.  With the usual 30-40 % inliers that is ~3 passes per chunk
// instead of 8 per pose.
using sfmchi::kChunk;

__global__ __launch_bounds__(256) void cheirality_batched_kernel(
    const Corr* __restrict__ corr, int64_t n, const double* __restrict__ pose_rt,
    const uint8_t* __restrict__ mask, double distance_threshold, uint8_t* __restrict__ pass) {
    __shared__ int32_t list[256 / kWave][kChunk];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int64_t b = blockIdx.y;
    const int64_t base = ((int64_t)blockIdx.x * (256 / kWave) + wave) * kChunk;
    if (base >= n) return;  // whole wave; no block-level barrier below
    const uint8_t* m = mask != nullptr ? mask + b * n : nullptr;
    // The four candidates come in two antipodal pairs, (R, t) and (R, -t) (eight_point.py:210-212; sfm_decompose_essential writes
    // them so), and one solve decides both (sfm_cheirality.h).  Taken only when the second pose of a pair IS the first with t
    // negated, bit for bit (block-uniform); any other pose table is solved pose by pose.  One pair of poses per block in z (more
    // waves in flight; the compaction is cheap enough to repeat).
    const int pose_begin = 2 * (int)blockIdx.z;
    const double* rt0 = pose_rt + (b * 4 + pose_begin) * 12;
    const double* rt1 = rt0 + 12;
    bool antipodal = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) antipodal = antipodal && (k < 9 ? rt1[k] == rt0[k] : rt1[k] == -rt0[k]);
    uint8_t* out0 = pass + (b * 4 + pose_begin) * n;   // the rows of this block's two poses
    uint8_t* out1 = out0 + n;
    const int total = sfmchi::compact_chunk<kChunk>(list[wave], lane, [&](int position, int32_t& entry) {
        const int64_t i = base + position;
        const bool inside = i < n;
        const bool act = inside && (m == nullptr || m[i] != 0);
        if (inside && !act) {
            out0[i] = 0;
            out1[i] = 0;
        }
        entry = position;
        return act;
    });
    for (int j = 0; j < total; j += kWave) {
        bool active;
        const int64_t i = base + sfmchi::group_entry(list[wave], j, lane, total, active);
        const Corr p = corr[b * n + i];
        for (int k = 0; k < (antipodal ? 1 : 2); ++k) {
            const sfmchi::Cheirality c = sfmchi::cheirality_test(k == 0 ? rt0 : rt1, p, distance_threshold);
            if (active) (k == 0 ? out0 : out1)[i] = c.ok ? 1 : 0;
            if (antipodal && active) out1[i] = c.mirrored ? 1 : 0;
        }
    }
}

// Pose vote (eight_point.py:213-237): votes[p] = number of passing correspondences, not counting the one
// at position 0 of the list handed to the reference (np.count_nonzero of the *index* array) — here the
// correspondence `skip_index[b]`; best = first maximum, -1 if every vote is zero.
__global__ __launch_bounds__(256) void pose_vote_kernel(const uint8_t* __restrict__ pass, int64_t n,
                                                        const int32_t* __restrict__ skip_index,
                                                        int32_t* __restrict__ votes,
                                                        int32_t* __restrict__ best) {
    const int64_t b = blockIdx.x;
    const int64_t skip = skip_index != nullptr ? (int64_t)skip_index[b] : -1;
    int cnt[4] = {0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int use = (i != skip) ? 1 : 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) cnt[p] += use & (int)pass[(b * 4 + p) * n + i];
    }
    __shared__ int partial[256 / kWave][4];
    int v[4];
    sfmchi::block_votes(cnt, partial, v);
    if (threadIdx.x == 0) {
        int arg, top;
        sfmchi::first_maximum(v, arg, top);
#pragma unroll
        for (int p = 0; p < 4; ++p) votes[b * 4 + p] = v[p];
        best[b] = arg;
    }
}

// Triangulation (triangulation.py:42-62) of the correspondences that pass the cheirality test of the
// chosen pose: P1 = [K|0], P2 = [K|0] [R t; 0 1], pixel coordinates.
struct Intrinsics {
    double k[9];
};

__global__ __launch_bounds__(256) void triangulate_selected_kernel(
    const double2* __restrict__ pix_a, const double2* __restrict__ pix_b, int64_t n, Intrinsics K,
    const double* __restrict__ pose_rt, const int32_t* __restrict__ best, const uint8_t* __restrict__ pass,
    double* __restrict__ X, uint8_t* __restrict__ valid) {
    // DLT solves only for the points that passed
    __shared__ int32_t list[256 / kWave][kChunk];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int64_t b = blockIdx.y;
    const int64_t base = ((int64_t)blockIdx.x * (256 / kWave) + wave) * kChunk;
    if (base >= n) return;
    const int pose = best[b];
    const bool have_pose = pose >= 0;
    const uint8_t* chosen = pass + (b * 4 + (have_pose ? pose : 0)) * n;
    const int total = sfmchi::compact_chunk<kChunk>(list[wave], lane, [&](int position, int32_t& entry) {
        const int64_t i = base + position;
        const bool inside = i < n;
        const bool keep = inside && have_pose && chosen[i] != 0;
        if (inside && !keep) {
            double* out = X + (b * n + i) * 3;
            out[0] = 0.0;
            out[1] = 0.0;
            out[2] = 0.0;
            valid[b * n + i] = 0;
        }
        entry = position;
        return keep;
    });
    if (total == 0) return;
    const double* rt = pose_rt + (b * 4 + pose) * 12;
    double P1[12], P2[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P1[r * 4 + c] = K.k[r * 3 + c];
            P2[r * 4 + c] = (K.k[r * 3 + 0] * rt[0 * 3 + c] + K.k[r * 3 + 1] * rt[1 * 3 + c]) + K.k[r * 3 + 2] * rt[2 * 3 + c];
        }
        P1[r * 4 + 3] = 0.0;
        P2[r * 4 + 3] = (K.k[r * 3 + 0] * rt[9 + 0] + K.k[r * 3 + 1] * rt[9 + 1]) + K.k[r * 3 + 2] * rt[9 + 2];
    }
    for (int j = 0; j < total; j += kWave) {
        bool active;
        const int64_t i = base + sfmchi::group_entry(list[wave], j, lane, total, active);
        const double2 a = pix_a[b * n + i];
        const double2 q = pix_b[b * n + i];
        double Xp[3];
        sfm::triangulate_dlt(P1, P2, a.x, a.y, q.x, q.y, Xp);
        if (active) {
            double* out = X + (b * n + i) * 3;
            out[0] = Xp[0];
            out[1] = Xp[1];
            out[2] = Xp[2];
            valid[b * n + i] = 1;
        }
    }
}

}  // namespace

extern "C" {

int sfm_cheirality_batched(const double* corr, int64_t n, int64_t batch, const double* pose_rt,
                           const uint8_t* mask, double distance_threshold, uint8_t* pass, void* stream) {
    if (n < 0 || batch < 0) return fail(SFM_EINVAL, "sfm_cheirality_batched: negative size");
    if (n == 0 || batch == 0) return SFM_OK;
    if (batch > 65535) return fail(SFM_EINVAL, "sfm_cheirality_batched: batch > 65535");
    if (!corr || !pose_rt || !pass) return fail(SFM_EINVAL, "sfm_cheirality_batched: null pointer");
    // one antipodal pair of poses per block in z (one pose per block until round 5: 5.08 ms per C5 batch vs 5.29 with all four
    // poses in one wave, profiles/r01/README.md; the pair shares its solve now)
    SFM_REQUIRE_GRID("sfm_cheirality_batched", n, kChunk * (256 / kWave), 256, batch);
    hipLaunchKernelGGL(cheirality_batched_kernel, dim3(grid_for(n, kChunk * (256 / kWave)), (unsigned)batch, 2),
                       dim3(256), 0, (hipStream_t)stream, (const Corr*)corr, n, pose_rt, mask, distance_threshold, pass);
    return check_launch("cheirality_batched_kernel");
}

int sfm_pose_vote(const uint8_t* pass, int64_t n, int64_t batch, const int32_t* skip_index, int32_t* votes,
                  int32_t* best, void* stream) {
    if (n < 0 || batch < 0) return fail(SFM_EINVAL, "sfm_pose_vote: negative size");
    if (batch == 0) return SFM_OK;
    if (!votes || !best || (n > 0 && !pass)) return fail(SFM_EINVAL, "sfm_pose_vote: null pointer");
    hipLaunchKernelGGL(pose_vote_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, pass, n,
                       skip_index, votes, best);
    return check_launch("pose_vote_kernel");
}

int sfm_triangulate_selected(const double* pix_a, const double* pix_b, int64_t n, int64_t batch,
                             const double* K, const double* pose_rt, const int32_t* best,
                             const uint8_t* pass, double* X, uint8_t* valid, void* stream) {
    if (n < 0 || batch < 0) return fail(SFM_EINVAL, "sfm_triangulate_selected: negative size");
    if (n == 0 || batch == 0) return SFM_OK;
    if (batch > 65535) return fail(SFM_EINVAL, "sfm_triangulate_selected: batch > 65535");
    if (!pix_a || !pix_b || !K || !pose_rt || !best || !pass || !X || !valid)
        return fail(SFM_EINVAL, "sfm_triangulate_selected: null pointer");
    Intrinsics intr;
    for (int j = 0; j < 9; ++j) intr.k[j] = K[j];  // host pointer, passed by value
    SFM_REQUIRE_GRID("sfm_triangulate_selected", n, kChunk * (256 / kWave), 256, batch);
    hipLaunchKernelGGL(triangulate_selected_kernel, dim3(grid_for(n, kChunk * (256 / kWave)), (unsigned)batch),
                       dim3(256), 0, (hipStream_t)stream, (const double2*)pix_a, (const double2*)pix_b, n, intr, pose_rt, best,
                       pass, X, valid);
    return check_launch("triangulate_selected_kernel");
}

}  // extern "C"
