// Oriented integer BRIEF descriptors and their brute-force Hamming matcher (definition:
// tests/brief_oracle.py).  Everything is integer arithmetic on a uint8 image — no libm, no floating-point rounding —, so
// both kernels are bit-identical to the NumPy definition.
//
//   brief_describe_kernel    (its body is sfmbrief::describe_feature of sfm_brief_device.h, which the keypoint detector of
//                            sfm_keypoints.hip calls too) one wave per feature: the 31 x 31 patch goes to LDS while the
//                            lanes accumulate the intensity moments m10 / m01 over the radius-15 disc (integer sums: any order); lanes 0..bins-1 each test
//                            one angle bin with two int64 cross products against the table's boundary vectors and a ballot
//                            picks the bin; the 27 x 27 sums of 5 x 5 boxes are built separably in LDS (at most 25 * 255 =
//                            6375: 16 bits); lane l evaluates tests l, l + 64, l + 128, l + 192 of the bin's pattern and four
//                            64-bit ballots ARE the four little-endian descriptor words.
//   hamming_summary_kernel   a 256-thread block owns 256 A rows x 512 B columns (the tile of sfm_hamming_tile.h): the
//                            lane scans its 512 columns in B order and leaves the four numbers of sfm_match_summary.h.  The
//                            shared summary_combine_kernel then walks the tiles: same best / arg / second as sfm_match_summary,
//                            and the |A| x |B| matrix is never written.  Splitting the columns over blocks gives
//                            20 000 x 20 000 descriptors 79 x 40 blocks instead of 313 waves.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_brief_device.h"
#include "sfm_common.h"
#include "sfm_hamming_tile.h"
#include "sfm_match_summary.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_for;

using sfmbrief::kWords;

__global__ __launch_bounds__(kWave) void brief_describe_kernel(
    const uint8_t* __restrict__ image, int64_t height, int64_t width, const double* __restrict__ feats,
    const int32_t* __restrict__ offsets, const long long* __restrict__ boundaries, int bins,
    unsigned long long* __restrict__ desc, uint8_t* __restrict__ ok, uint8_t* __restrict__ angle_bin) {
    const int64_t f = blockIdx.x;
    sfmbrief::describe_feature(image, height, width, feats[2 * f], feats[2 * f + 1], offsets, boundaries, bins,
                               desc + f * kWords, ok + f, angle_bin + f);
}

using sfmham::kCols;
using sfmham::kRows;
// distances are at most 256; an invalid pair scores +inf.  "Nothing yet" ranks above it so that the first column of a tile
// of invalid pairs still becomes the tile's first minimum, as +inf does in the heap.
constexpr int kHamInvalid = 0x7FFFFFFE, kHamNothing = 0x7FFFFFFF;

SFM_DEVICE double hamming_score(int v) { return v >= kHamInvalid ? INFINITY : (double)v; }

__global__ __launch_bounds__(kRows) void hamming_summary_kernel(
    const uint4* __restrict__ desc_a, const uint8_t* __restrict__ ok_a, int64_t nA, const uint4* __restrict__ desc_b,
    const uint8_t* __restrict__ ok_b, int64_t nB, int64_t row_blocks, TileSummary* __restrict__ tiles) {
    __shared__ sfmham::Tile s_b;
    // consecutive blocks share a B tile
    const int64_t row_block = blockIdx.x % row_blocks, tile = blockIdx.x / row_blocks;
    const int64_t c0 = tile * kCols;
    const int cols = (int)min((int64_t)kCols, nB - c0);   // >= 1
    sfmham::stage(s_b, desc_b, ok_b, c0, cols);
    const int64_t row = row_block * kRows + threadIdx.x;
    const sfmham::Row a = sfmham::load_row(desc_a, ok_a, min(row, nA - 1));
    __syncthreads();
    int tile_min = kHamNothing, tile_arg = 0, left_prefixed = kHamNothing, left_min = kHamNothing;
#pragma unroll 4
    for (int j = 0; j < cols; ++j) {
        const int d = SFM_HAMMING_DISTANCE(a, s_b, j);
        const int v = (a.valid && s_b.ok[j]) ? d : kHamInvalid;
        if (in_left_subtree(c0 + j + 1)) {           // wave-uniform; tile_min is still the minimum BEFORE column j
            left_prefixed = min(left_prefixed, max(v, tile_min));
            left_min = min(left_min, v);
        }
        if (v < tile_min) {                          // strict: the first minimum keeps its column
            tile_min = v;
            tile_arg = j;
        }
    }
    if (row < nA) {
        TileSummary r;
        r.tile_min = hamming_score(tile_min);
        r.left_prefixed = hamming_score(left_prefixed);
        r.left_min = hamming_score(left_min);
        r.tile_arg = c0 + tile_arg;
        tiles[tile * nA + row] = r;
    }
}

}  // namespace

extern "C" {

int sfm_brief_describe(const uint8_t* image, int64_t height, int64_t width, const double* feats, int64_t n,
                       const int8_t* offsets, const int64_t* boundaries, int bins, uint8_t* desc, uint8_t* ok,
                       uint8_t* angle_bin, void* stream) {
    if (n < 0 || height <= 0 || width <= 0) return fail(SFM_EINVAL, "sfm_brief_describe: bad size");
    if (bins < 1 || bins > kWave) return fail(SFM_EINVAL, "sfm_brief_describe: bins must be in 1..64");
    if (n == 0) return SFM_OK;
    if (!image || !feats || !offsets || !boundaries || !desc || !ok || !angle_bin)
        return fail(SFM_EINVAL, "sfm_brief_describe: null pointer");
    if ((reinterpret_cast<uintptr_t>(desc) & 7u) != 0 || (reinterpret_cast<uintptr_t>(offsets) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(boundaries) & 7u) != 0 || (reinterpret_cast<uintptr_t>(feats) & 7u) != 0)
        return fail(SFM_EINVAL, "sfm_brief_describe: desc, boundaries, feats must be 8-byte and offsets 4-byte aligned");
    SFM_REQUIRE_GRID("sfm_brief_describe", n, 1, kWave);
    hipLaunchKernelGGL(brief_describe_kernel, dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream, image, height, width,
                       feats, reinterpret_cast<const int32_t*>(offsets), reinterpret_cast<const long long*>(boundaries), bins,
                       reinterpret_cast<unsigned long long*>(desc), ok, angle_bin);
    return check_launch("brief_describe_kernel");
}

int64_t sfm_hamming_summary_workspace_bytes(int64_t n_a, int64_t n_b) {
    if (n_a < 0 || n_b < 0) return -1;
    return (int64_t)sizeof(TileSummary) * n_a * ((n_b + kCols - 1) / kCols);
}

int sfm_hamming_summary(const uint8_t* desc_a, const uint8_t* ok_a, int64_t n_a, const uint8_t* desc_b, const uint8_t* ok_b,
                        int64_t n_b, void* workspace, int64_t workspace_bytes, double* best, int32_t* arg, double* second,
                        void* stream) {
    if (n_a < 0 || n_b < 0) return fail(SFM_EINVAL, "sfm_hamming_summary: negative size");
    if (n_a == 0) return SFM_OK;
    if (n_b == 0) return fail(SFM_EINVAL, "sfm_hamming_summary: empty rows");
    if (n_b > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_hamming_summary: rows too long");
    if (!desc_a || !ok_a || !desc_b || !ok_b || !workspace || !best || !arg || !second)
        return fail(SFM_EINVAL, "sfm_hamming_summary: null pointer");
    if (workspace_bytes < sfm_hamming_summary_workspace_bytes(n_a, n_b))
        return fail(SFM_EINVAL, "sfm_hamming_summary: workspace smaller than sfm_hamming_summary_workspace_bytes(n_a, n_b)");
    if (((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(desc_a) | reinterpret_cast<uintptr_t>(desc_b)) & 15u) != 0)
        return fail(SFM_EINVAL, "sfm_hamming_summary: workspace and descriptors must be 16-byte aligned");
    const int64_t row_blocks = (n_a + kRows - 1) / kRows, n_tiles = (n_b + kCols - 1) / kCols;
    if (row_blocks * n_tiles > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_hamming_summary: too many tiles");
    SFM_REQUIRE_GRID("sfm_hamming_summary", n_a, 256, 256);
    TileSummary* tiles = static_cast<TileSummary*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hamming_summary_kernel, dim3((unsigned)(row_blocks * n_tiles)), dim3(kRows), 0, st,
                       reinterpret_cast<const uint4*>(desc_a), ok_a, n_a, reinterpret_cast<const uint4*>(desc_b), ok_b, n_b,
                       row_blocks, tiles);
    hipLaunchKernelGGL(summary_combine_kernel, dim3(grid_for(n_a, 256)), dim3(256), 0, st, tiles, n_a, n_b, n_tiles, best,
                       arg, second);
    return check_launch("hamming_summary_kernel");
}

}  // extern "C"
