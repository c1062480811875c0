// Oriented integer BRIEF descriptors and their brute-force Hamming matcher (definition:
// tests/brief_oracle.py).  Everything is integer arithmetic on a uint8 image — no libm, no floating-point rounding —, so
// both kernels are bit-identical to the NumPy definition.
//
//   brief_describe_kernel    one wave per feature: the 31 x 31 patch goes to LDS while the lanes accumulate the intensity
//                            moments m10 / m01 over the radius-15 disc (integer sums: any order); lanes 0..bins-1 each test
//                            one angle bin with two int64 cross products against the table's boundary vectors and a ballot
//                            picks the bin; the 27 x 27 sums of 5 x 5 boxes are built separably in LDS (at most 25 * 255 =
//                            6375: 16 bits); lane l evaluates tests l, l + 64, l + 128, l + 192 of the bin's pattern and four
//                            64-bit ballots ARE the four little-endian descriptor words.
//   hamming_summary_kernel   a 256-thread block owns 256 A rows x 512 B columns: every lane keeps the descriptor of one A row
//                            in eight registers, the B tile sits in LDS and is read as a broadcast; the lane scans its 512
//                            columns in B order and leaves the four numbers of sfm_match_summary.h.  The shared
//                            summary_combine_kernel then walks the tiles: same best / arg / second as sfm_match_summary,
//                            and the |A| x |B| matrix is never written.  Splitting the columns over blocks gives
//                            20 000 x 20 000 descriptors 79 x 40 blocks instead of 313 waves.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_match_summary.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_for;

constexpr int kPatchRadius = 15;                    // orientation disc and patch half-width
constexpr int kPatch = 2 * kPatchRadius + 1;        // 31
constexpr int kBoxSide = 5;                         // a sample is the sum of a 5 x 5 box
constexpr int kBox = kPatch - kBoxSide + 1;         // 27 box centres per axis: offsets -13 .. 13
constexpr int kReach = kBox / 2;                    // 13
constexpr int kTests = 256;
constexpr int kWords = kTests / 64;                 // descriptor: 4 x 64 bits = 32 bytes
static_assert(kTests == kWords * kWave, "one ballot per descriptor word");

__global__ __launch_bounds__(kWave) void brief_describe_kernel(
    const uint8_t* __restrict__ image, int64_t height, int64_t width, const double* __restrict__ feats,
    const int32_t* __restrict__ offsets, const long long* __restrict__ boundaries, int bins,
    unsigned long long* __restrict__ desc, uint8_t* __restrict__ ok, uint8_t* __restrict__ angle_bin) {
    __shared__ uint8_t s_patch[kPatch * kPatch];
    __shared__ uint16_t s_rows[kPatch * kBox];      // horizontal 5-sums
    __shared__ uint16_t s_box[kBox * kBox];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const double x = feats[2 * f], y = feats[2 * f + 1];
    const double xc = floor(x + 0.5), yc = floor(y + 0.5);
    // block-uniform.  NaN fails every comparison; the range test also bounds the int conversion below
    const bool valid = xc >= (double)kPatchRadius && xc <= (double)(width - kPatchRadius - 1) &&
                       yc >= (double)kPatchRadius && yc <= (double)(height - kPatchRadius - 1);
    if (!valid) {
        if (lane < kWords) desc[f * kWords + lane] = 0ull;
        if (lane == 0) {
            ok[f] = 0;
            angle_bin[f] = 0;
        }
        return;
    }
    const int64_t x0 = (int64_t)xc - kPatchRadius, y0 = (int64_t)yc - kPatchRadius;
    int m10 = 0, m01 = 0;                           // |m| <= 709 pixels * 15 * 255
    for (int idx = lane; idx < kPatch * kPatch; idx += kWave) {
        const int r = idx / kPatch, c = idx - r * kPatch;
        const int p = image[(y0 + r) * width + (x0 + c)];
        s_patch[idx] = (uint8_t)p;
        const int dx = c - kPatchRadius, dy = r - kPatchRadius;
        if (dx * dx + dy * dy <= kPatchRadius * kPatchRadius) {
            m10 += dx * p;
            m01 += dy * p;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off, kWave);
        m01 += __shfl_xor(m01, off, kWave);
    }
    // bin b: cross(B[b-1], m) >= 0 and cross(B[b], m) < 0 — a 12 degree wedge, exactly one for m != 0, none for m = 0
    bool hit = false;
    if (lane < bins) {
        const int prev = lane == 0 ? bins - 1 : lane - 1;
        const long long px = boundaries[2 * prev], py = boundaries[2 * prev + 1];
        const long long qx = boundaries[2 * lane], qy = boundaries[2 * lane + 1];
        hit = (px * m01 - py * m10 >= 0) && (qx * m01 - qy * m10 < 0);
    }
    const unsigned long long hits = __ballot(hit);
    const int bin = hits ? __ffsll((long long)hits) - 1 : 0;
    __syncthreads();
    for (int idx = lane; idx < kPatch * kBox; idx += kWave) {
        const int r = idx / kBox, c = idx - r * kBox;
        int s = 0;
#pragma unroll
        for (int k = 0; k < kBoxSide; ++k) s += s_patch[r * kPatch + c + k];
        s_rows[idx] = (uint16_t)s;
    }
    __syncthreads();
    for (int idx = lane; idx < kBox * kBox; idx += kWave) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < kBoxSide; ++k) s += s_rows[idx + k * kBox];
        s_box[idx] = (uint16_t)s;
    }
    __syncthreads();
    auto coordinate = [](int32_t packed, int byte) {   // int8 of the packed (ax, ay, bx, by), held inside the box array
        const int v = (int)(int8_t)(packed >> (8 * byte));
        return min(max(v, -kReach), kReach) + kReach;
    };
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
        const int32_t o = offsets[(int64_t)bin * kTests + k * kWave + lane];
        const int a = s_box[coordinate(o, 1) * kBox + coordinate(o, 0)];
        const int b = s_box[coordinate(o, 3) * kBox + coordinate(o, 2)];
        const unsigned long long word = __ballot(a < b);
        if (lane == 0) desc[f * kWords + k] = word;
    }
    if (lane == 0) {
        ok[f] = 1;
        angle_bin[f] = (uint8_t)bin;
    }
}

constexpr int kHamRows = 256;                       // A rows per block, one per lane
constexpr int kHamCols = 512;                       // B columns per block: 16 KiB of LDS
// distances are at most 256; an invalid pair scores +inf.  "Nothing yet" ranks above it so that the first column of a tile
// of invalid pairs still becomes the tile's first minimum, as +inf does in the heap.
constexpr int kHamInvalid = 0x7FFFFFFE, kHamNothing = 0x7FFFFFFF;

SFM_DEVICE double hamming_score(int v) { return v >= kHamInvalid ? INFINITY : (double)v; }

__global__ __launch_bounds__(kHamRows) void hamming_summary_kernel(
    const uint4* __restrict__ desc_a, const uint8_t* __restrict__ ok_a, int64_t nA, const uint4* __restrict__ desc_b,
    const uint8_t* __restrict__ ok_b, int64_t nB, int64_t row_blocks, TileSummary* __restrict__ tiles) {
    __shared__ uint4 s_b[kHamCols][2];
    __shared__ int s_ok[kHamCols];
    const int tid = threadIdx.x;
    // consecutive blocks share a B tile
    const int64_t row_block = blockIdx.x % row_blocks, tile = blockIdx.x / row_blocks;
    const int64_t c0 = tile * kHamCols;
    const int cols = (int)min((int64_t)kHamCols, nB - c0);   // >= 1
    for (int j = tid; j < cols; j += kHamRows) {
        s_b[j][0] = desc_b[2 * (c0 + j)];
        s_b[j][1] = desc_b[2 * (c0 + j) + 1];
        s_ok[j] = ok_b[c0 + j] != 0;
    }
    const int64_t row = row_block * kHamRows + tid;
    const int64_t src = min(row, nA - 1);
    const uint4 a0 = desc_a[2 * src], a1 = desc_a[2 * src + 1];
    const bool a_valid = ok_a[src] != 0;
    __syncthreads();
    int tile_min = kHamNothing, tile_arg = 0, left_prefixed = kHamNothing, left_min = kHamNothing;
#pragma unroll 4
    for (int j = 0; j < cols; ++j) {
        const uint4 b0 = s_b[j][0], b1 = s_b[j][1];
        const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                      __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
        const int v = (a_valid && s_ok[j]) ? d : kHamInvalid;
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
    return (int64_t)sizeof(TileSummary) * n_a * ((n_b + kHamCols - 1) / kHamCols);
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
    const int64_t row_blocks = (n_a + kHamRows - 1) / kHamRows, n_tiles = (n_b + kHamCols - 1) / kHamCols;
    if (row_blocks * n_tiles > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_hamming_summary: too many tiles");
    SFM_REQUIRE_GRID("sfm_hamming_summary", n_a, 256, 256);
    TileSummary* tiles = static_cast<TileSummary*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hamming_summary_kernel, dim3((unsigned)(row_blocks * n_tiles)), dim3(kHamRows), 0, st,
                       reinterpret_cast<const uint4*>(desc_a), ok_a, n_a, reinterpret_cast<const uint4*>(desc_b), ok_b, n_b,
                       row_blocks, tiles);
    hipLaunchKernelGGL(summary_combine_kernel, dim3(grid_for(n_a, 256)), dim3(256), 0, st, tiles, n_a, n_b, n_tiles, best,
                       arg, second);
    return check_launch("hamming_summary_kernel");
}

}  // extern "C"
