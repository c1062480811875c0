// Heap-summary pieces shared by the matchers (sfm_match.hip: NCC / SSD windows; sfm_brief.hip: Hamming distances).
//
// A row of scores pushed in B order onto the reference's per-feature heapq leaves heap[0] = the first minimum and
// heap[1] (the LEFT child, which the ratio test divides by) = min over pushes i landing in the left subtree of
// max(score_i, running minimum before i).  That scan splits over column tiles: with c = minimum of everything before
// the tile and p_i = minimum of the tile's own columns before i,
//     max(v_i, min(c, p_i)) = min(max(v_i, p_i), max(v_i, c)),   and   min_i max(v_i, c) = max(c, min_i v_i),
// so per (row, tile) four numbers suffice (TileSummary) and summary_combine_kernel walks them in B order.  All of it is
// selection (min / max / compare), no arithmetic: the result is bit-identical to a scan of the full row.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_math.h"

// heap position (1-based push count) -> does the push land in the root's left subtree
SFM_DEVICE bool in_left_subtree(int64_t position_1based) {
    if (position_1based < 2) return false;
    const int k = 63 - __builtin_clzll((unsigned long long)position_1based);
    return position_1based < ((int64_t)1 << k) + ((int64_t)1 << (k - 1));
}

// (value, index) lexicographic minimum == first occurrence of the smallest value
struct MinAt {
    double v;
    int64_t i;
};
SFM_DEVICE MinAt min_at(MinAt a, MinAt b) {
    const bool take_b = (b.v < a.v) || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}

// One (row, column tile): M = tile minimum and its first column, left_prefixed = min over left-subtree columns of
// max(v_i, p_i), left_min = min over left-subtree columns of v_i.  Stored tile-major: tiles[tile * nA + row].
struct TileSummary {
    double tile_min, left_prefixed, left_min;
    int64_t tile_arg;
};
static_assert(sizeof(TileSummary) == 32, "workspace sizing of the *_summary_workspace_bytes entry points");

// one thread per A-feature walks its tile summaries in B order
static __global__ void summary_combine_kernel(const TileSummary* __restrict__ tiles, int64_t nA, int64_t nB,
                                              int64_t n_tiles, double* __restrict__ best, int32_t* __restrict__ arg,
                                              double* __restrict__ second) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nA) return;
    double before = INFINITY, sec = INFINITY;  // `before`: minimum of all columns ahead of the tile
    MinAt top = {INFINITY, INT64_MAX};
    for (int64_t t = 0; t < n_tiles; ++t) {
        const TileSummary r = tiles[t * nA + row];
        const double via_before = (r.left_min < before) ? before : r.left_min;
        sec = fmin(sec, fmin(r.left_prefixed, via_before));
        top = min_at(top, MinAt{r.tile_min, r.tile_arg});
        before = fmin(before, r.tile_min);
    }
    best[row] = top.v;
    arg[row] = (int32_t)top.i;
    second[row] = nB > 1 ? sec : NAN;
}
