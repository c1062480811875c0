// The tile of the brute-force Hamming matchers of 32-byte descriptors (hamming_summary_kernel of sfm_brief.hip,
// match_pairs_nearest_kernel and, with coordinates, match_pairs_guided_kernel of sfm_match_pairs.hip).  A 256-thread
// block owns 256 rows, one per lane: the lane keeps its descriptor in eight registers and walks 512 descriptors of the
// other side, which sit in LDS with their validity flags and are read as broadcasts.  The walk stays in the kernels and the distance is a macro: a callback per column, or a
// distance function, changed the order of selects, sums and LDS reads: 2 to 8 % slower on small calls.
#pragma once
#include <hip/hip_runtime.h>

#include "sfm_math.h"

namespace sfmham {

constexpr int kRows = 256;   // rows per block, one per lane
constexpr int kCols = 512;   // descriptors of the other side per LDS tile: 16 KiB plus the flags

struct Tile {
    uint4 desc[kCols][2];
    int ok[kCols];
};
struct Row {
    uint4 lo, hi;
    bool valid;
};
SFM_DEVICE Row load_row(const uint4* __restrict__ desc, const uint8_t* __restrict__ ok, int64_t index) {
    return Row{desc[2 * index], desc[2 * index + 1], ok[index] != 0};
}

// Descriptors first .. first + cols - 1 into the tile, by all kRows lanes.  The barriers around it are the caller's.
SFM_DEVICE void stage(Tile& tile, const uint4* __restrict__ desc, const uint8_t* __restrict__ ok, int64_t first, int cols) {
    for (int j = threadIdx.x; j < cols; j += kRows) {
        tile.desc[j][0] = desc[2 * (first + j)];
        tile.desc[j][1] = desc[2 * (first + j) + 1];
        tile.ok[j] = ok[first + j] != 0;
    }
}

// The same tile with the columns' K-normalised coordinates beside them (match_pairs_guided_kernel: 8 KiB more), staged in
// the same pass by the same lanes.  xy is only 8-byte aligned in global memory: two loads, one 16-byte LDS store.
struct TileXY {
    uint4 desc[kCols][2];
    int ok[kCols];
    double2 xy[kCols];
};
SFM_DEVICE void stage(TileXY& tile, const uint4* __restrict__ desc, const uint8_t* __restrict__ ok, const double* __restrict__ xy,
                      int64_t first, int cols) {
    for (int j = threadIdx.x; j < cols; j += kRows) {
        tile.desc[j][0] = desc[2 * (first + j)];
        tile.desc[j][1] = desc[2 * (first + j) + 1];
        tile.ok[j] = ok[first + j] != 0;
        tile.xy[j] = make_double2(xy[2 * (first + j)], xy[2 * (first + j) + 1]);
    }
}

}  // namespace sfmham

// Hamming distance of a Row to column j of a Tile or a TileXY
#define SFM_HAMMING_DISTANCE(row, tile, j)                                                     \
    (__popc((row).lo.x ^ (tile).desc[j][0].x) + __popc((row).lo.y ^ (tile).desc[j][0].y) +     \
     __popc((row).lo.z ^ (tile).desc[j][0].z) + __popc((row).lo.w ^ (tile).desc[j][0].w) +     \
     __popc((row).hi.x ^ (tile).desc[j][1].x) + __popc((row).hi.y ^ (tile).desc[j][1].y) +     \
     __popc((row).hi.z ^ (tile).desc[j][1].z) + __popc((row).hi.w ^ (tile).desc[j][1].w))
