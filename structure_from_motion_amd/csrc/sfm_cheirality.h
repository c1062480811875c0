// The two-view pose stage's shared device code: the cheirality test of one correspondence under one pose (reference
// eight_point.py:449-488), the wave-level compaction of a chunk of items to those worth a DLT solve, and the four-way pose vote
// (eight_point.py:213-237).  Used by cheirality_kernel (sfm_kernels.hip), cheirality_batched_kernel, triangulate_selected_kernel
// and pose_vote_kernel (sfm_pose.hip), pose_cheirality_kernel and pose_vote_median_kernel (sfm_view_graph_pose.hip).
//
// Two properties every caller relies on:
//   * sfm::triangulate_dlt ends in null_vector4, whose inverse-iteration loop and Jacobi fallback break on __all / __any.  Every
//     lane of a wave must reach the call together (converged control flow; a lane without an item of its own redoes a valid
//     one), and the number of iterations a lane runs depends on its wave-mates: the last bits of X are a function of WHICH items
//     share a wave.  compact_chunk therefore pushes survivors in item order, and group_entry hands lane l of group j entry
//     j + l: a wave holds the same items whichever kernel calls them, and results are reproducible bit for bit.
//   * Where the decisions go is the caller's: 4 bits per item (view graph), 4 x n bytes (batched call), poses x m bytes (single
//     call).  Nothing here stores to global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmchi {

constexpr int kChunk = 512;   // items per wave of the compacting kernels

// The 12 doubles R (9) | t (3) of a pose as the 3 x 4 row-major [R | t].
SFM_DEVICE void pose_matrix(const double* rt, double P2[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P2[r * 4 + 0] = rt[r * 3 + 0];
        P2[r * 4 + 1] = rt[r * 3 + 1];
        P2[r * 4 + 2] = rt[r * 3 + 2];
        P2[r * 4 + 3] = rt[9 + r];
    }
}

// The decision for the pose (R, t), the decision for its antipode (R, -t), and the point triangulated under (R, t).
struct Cheirality {
    bool ok, mirrored;
    double X[3];
};

// One DLT solve of correspondence p between P1 = [I | 0] and P2 = [R | t], and the reference's three comparisons: depth in
// camera 1, depth in camera 2 (third row of P2 @ [X, 1], eight_point.py:476, summed left to right) and the distance.
// The antipodal shortcut: the DLT null vector of (R, -t) is that of (R, t) with its last component negated, so X' = -X, and
// R X' - t = -(R X + t): both depths change sign and the norm stays.  ONE solve decides both poses; `mirrored` is valid only
// when the other pose IS this one with t negated, bit for bit (sfm_decompose_essential writes candidates 2k and 2k + 1 so).
// NaN fails both, as it does when each is solved.  A caller that reads only `ok` pays nothing for the rest.
SFM_DEVICE Cheirality cheirality_test(const double* rt, const Corr& p, double distance_threshold) {
    const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double P2[12];
    pose_matrix(rt, P2);
    Cheirality c;
    sfm::triangulate_dlt(P1, P2, p.xa, p.ya, p.xb, p.yb, c.X);
    const double z2 = ((P2[8] * c.X[0] + P2[9] * c.X[1]) + P2[10] * c.X[2]) + P2[11];
    const double norm = sqrt((c.X[0] * c.X[0] + c.X[1] * c.X[1]) + c.X[2] * c.X[2]);
    c.ok = (c.X[2] >= -1e-8) && (z2 >= -1e-8) && (norm <= distance_threshold);
    c.mirrored = (-c.X[2] >= -1e-8) && (-z2 >= -1e-8) && (norm <= distance_threshold);
    return c;
}

// Compacts the CHUNK items of a wave into `list` (the wave's own CHUNK words of LDS): item(position, entry) says whether the
// item at `position` = s + lane of the chunk survives and, if so, which word to push; what it stores for an item that does not
// survive is its own business.  Survivors land in item order (ballot + prefix count).  Returns their number, wave-uniform.
template <int CHUNK, typename Item>
SFM_DEVICE int compact_chunk(int32_t* list, int lane, Item item) {
    int total = 0;
    for (int s = 0; s < CHUNK; s += kWave) {
        int32_t entry = 0;
        const bool keep = item(s + lane, entry);
        const unsigned long long votes = __ballot(keep);
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(votes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)votes, 0));
        if (keep) list[total + before] = entry;
        total += (int)__popcll(votes);
    }
    return total;
}

// The entry of this lane in the group of 64 survivors that starts at j.  Lanes past the end (`active` false) redo the group's
// first entry so that the wave-uniform loops of null_vector4 see valid data; they must store nothing.
SFM_DEVICE int32_t group_entry(const int32_t* list, int j, int lane, int total, bool& active) {
    active = j + lane < total;
    return list[active ? j + lane : j];
}

// Block totals of four per-thread counts: wave sums, one partial per wave in LDS, a barrier.  Every thread gets the totals.
template <int WAVES>
SFM_DEVICE void block_votes(const int cnt[4], int (&partial)[WAVES][4], int votes[4]) {
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int total = sfm::wave_sum(cnt[p]);
        if (lane == 0) partial[wave][p] = total;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        votes[p] = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) votes[p] += partial[w][p];
    }
}

// The first maximum of the votes (np.argmax) and its count; -1 and 0 when every vote is zero.
SFM_DEVICE void first_maximum(const int votes[4], int& best, int& top) {
    best = -1;
    top = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (votes[p] > top) {   // strict: the first maximum wins
            top = votes[p];
            best = p;
        }
    }
}

}  // namespace sfmchi
