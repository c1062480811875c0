// Multi-scale FAST-9 keypoints with oriented BRIEF per pyramid level, for a whole image collection in one call (DESIGN.md
// section 6x; definition: tests/keypoint_oracle.py).  Everything is integer arithmetic on uint8 planes, so every kernel is
// byte-identical to the NumPy definition.
//
// All planes of all images lie in one pixel pool; the plane table says where.  Every plane is cut into tiles of 64 x 16 pixels
// and a block owns one tile: it finds its plane by a binary search over the running tile counts, so one launch covers planes of
// any mix of sizes without an idle block.
//
//   pyramid_level_kernel       level l from level l - 1 of the same image (bilinear at scale 5/4 in 1/8 pixel steps), one launch
//                              per level over the images that have it
//   fast_score_kernel          stages the tile with a 3 pixel halo in LDS, tests the 16 circle pixels of every centre that has a
//                              whole BRIEF patch around it and writes the uint16 score map (0: no corner)
//   suppress_kernel            3 x 3 non-maximum suppression of the score map into a second map (not in place: the result does not
//                              depend on the order of the blocks) and one histogram of the survivors' scores per plane
//   cutoff_kernel              one block per plane: the largest T with count(score >= T) >= quota, or 1
//   collect_kernel             appends every survivor at or above its plane's cutoff to the candidate list (slot order arbitrary;
//                              the counter keeps counting beyond the capacity and the host calls again with that capacity)
//   keypoint_describe_kernel   one wave per candidate slot below the device-side count: sfm_brief_describe's descriptor on the
//                              candidate's plane
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "sfm_brief_device.h"
#include "sfm_common.h"
#include "sfm_keypoint_planes.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;

using sfmplanes::CheckedTable;
using sfmplanes::DevPlane;                          // the plane table as the kernels read it (sfm_keypoint_planes.h)
using sfmplanes::kMaxPlanes;
using sfmplanes::kTileH;
using sfmplanes::kTileW;

constexpr int kThreads = 256;                       // lane x of the tile, rows y, y + 4, y + 8, y + 12
constexpr int kRowsPerThread = kTileW * kTileH / kThreads;
constexpr int kRowStep = kThreads / kTileW;
constexpr int kRing = 3;                            // radius of the FAST circle
constexpr int kBorder = 15;                         // a tested centre keeps a whole 31 x 31 BRIEF patch
constexpr int kBins = 4096;                         // scores are at most 16 * 254 = 4064
static_assert(kTileW == kWave && kThreads % kTileW == 0, "a wave owns one row of the tile");

// The plane whose tiles hold global tile `tile`: planes[n].tile_start is the total.
__device__ __forceinline__ int plane_of_tile(const DevPlane* __restrict__ planes, int n, int tile) {
    int lo = 0, hi = n - 1;                         // the last p with tile_start[p] <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (planes[mid].tile_start <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct Tile {
    DevPlane plane;
    int index, x0, y0;
};

__device__ __forceinline__ Tile tile_of_block(const DevPlane* __restrict__ planes, int n, int first_tile) {
    Tile t;
    const int tile = first_tile + (int)blockIdx.x;
    t.index = plane_of_tile(planes, n, tile);
    t.plane = planes[t.index];
    const int local = tile - t.plane.tile_start;
    t.y0 = (local / t.plane.tiles_x) * kTileH;
    t.x0 = (local % t.plane.tiles_x) * kTileW;
    return t;
}

__global__ __launch_bounds__(kThreads) void pyramid_level_kernel(const DevPlane* __restrict__ planes, int n, int first_tile,
                                                                 uint8_t* __restrict__ pool) {
    const Tile t = tile_of_block(planes, n, first_tile);
    const int W = t.plane.width, H = t.plane.height;
    const DevPlane below = planes[t.plane.source];
    const uint8_t* __restrict__ src = pool + below.offset;
    const int64_t SW = below.width;
    const int x = t.x0 + (int)(threadIdx.x % kTileW);
    if (x >= W) return;
    const int ux = 10 * x + 1, sx = ux >> 3, fx = ux & 7;   // sx + 1 <= SW - 1 because 10 (W - 1) + 1 <= 8 SW - 9
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int y = t.y0 + (int)(threadIdx.x / kTileW) + k * kRowStep;
        if (y >= H) break;
        const int uy = 10 * y + 1, sy = uy >> 3, fy = uy & 7;
        const uint8_t* row = src + sy * SW + sx;
        const int top = (8 - fx) * row[0] + fx * row[1], bottom = (8 - fx) * row[SW] + fx * row[SW + 1];
        pool[t.plane.offset + (int64_t)y * W + x] = (uint8_t)(((8 - fy) * top + fy * bottom + 32) >> 6);
    }
}

// the 16 circle pixels in the definition's order, as (dx, dy)
__device__ constexpr int8_t kCircle[16][2] = {{0, -3}, {1, -3}, {2, -2}, {3, -1}, {3, 0},  {3, 1},   {2, 2},   {1, 3},
                                              {0, 3},  {-1, 3}, {-2, 2}, {-3, 1}, {-3, 0}, {-3, -1}, {-2, -2}, {-1, -3}};

// nine cyclically contiguous bits of a 16-bit mask
__device__ __forceinline__ bool nine_in_a_row(unsigned mask) {
    const unsigned m = mask | (mask << 16);
    const unsigned two = m & (m >> 1), four = two & (two >> 2), eight = four & (four >> 4);
    return (eight & (m >> 8)) != 0u;
}

__global__ __launch_bounds__(kThreads) void fast_score_kernel(const DevPlane* __restrict__ planes, int n,
                                                              const uint8_t* __restrict__ pool, int threshold,
                                                              uint16_t* __restrict__ score) {
    constexpr int kStageW = kTileW + 2 * kRing, kStageH = kTileH + 2 * kRing, kPitch = kStageW + 2;
    __shared__ uint8_t s_tile[kStageH * kPitch];
    const Tile t = tile_of_block(planes, n, 0);
    const int W = t.plane.width, H = t.plane.height;
    const uint8_t* __restrict__ image = pool + t.plane.offset;
    // a tile none of whose pixels is tested needs no pixels
    const bool any = t.x0 + kTileW > kBorder && t.x0 <= W - kBorder - 1 && t.y0 + kTileH > kBorder && t.y0 <= H - kBorder - 1;
    if (any) {
        for (int idx = threadIdx.x; idx < kStageH * kStageW; idx += kThreads) {
            const int r = idx / kStageW, c = idx - r * kStageW;
            const int y = t.y0 + r - kRing, x = t.x0 + c - kRing;
            s_tile[r * kPitch + c] = (y >= 0 && y < H && x >= 0 && x < W) ? image[(int64_t)y * W + x] : (uint8_t)0;
        }
        __syncthreads();
    }
    const int lx = threadIdx.x % kTileW, x = t.x0 + lx;
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int ly = (int)(threadIdx.x / kTileW) + k * kRowStep, y = t.y0 + ly;
        if (y >= H) break;
        int value = 0;
        if (x >= kBorder && x <= W - kBorder - 1 && y >= kBorder && y <= H - kBorder - 1) {
            const uint8_t* centre = s_tile + (ly + kRing) * kPitch + (lx + kRing);
            const int high = (int)centre[0] + threshold, low = (int)centre[0] - threshold;
            unsigned brighter = 0u, darker = 0u;
            int sum_brighter = 0, sum_darker = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int v = centre[kCircle[i][1] * kPitch + kCircle[i][0]];
                if (v > high) {
                    brighter |= 1u << i;
                    sum_brighter += v - high;
                }
                if (v < low) {
                    darker |= 1u << i;
                    sum_darker += low - v;
                }
            }
            if (nine_in_a_row(brighter) || nine_in_a_row(darker)) value = max(sum_brighter, sum_darker);
        }
        score[t.plane.offset + (int64_t)y * W + x] = (uint16_t)value;
    }
}

__global__ __launch_bounds__(kThreads) void suppress_kernel(const DevPlane* __restrict__ planes, int n,
                                                            const uint16_t* __restrict__ score, uint16_t* __restrict__ kept,
                                                            int32_t* __restrict__ histogram) {
    const Tile t = tile_of_block(planes, n, 0);
    const int W = t.plane.width, H = t.plane.height;
    const uint16_t* __restrict__ map = score + t.plane.offset;
    const int x = t.x0 + (int)(threadIdx.x % kTileW);
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int y = t.y0 + (int)(threadIdx.x / kTileW) + k * kRowStep;
        if (y >= H) break;
        const int s = map[(int64_t)y * W + x];
        bool survives = s > 0;
        if (survives) {
            for (int dy = -1; dy <= 1; ++dy) {
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const int ny = y + dy, nx = x + dx;
                    const int v = (ny >= 0 && ny < H && nx >= 0 && nx < W) ? (int)map[(int64_t)ny * W + nx] : 0;
                    const bool earlier = dy < 0 || (dy == 0 && dx < 0);   // raster order: an equal earlier neighbour wins
                    survives = survives && (earlier ? s > v : s >= v);
                }
            }
        }
        kept[t.plane.offset + (int64_t)y * W + x] = (uint16_t)(survives ? s : 0);
        if (survives) atomicAdd(&histogram[(int64_t)t.index * kBins + min(s, kBins - 1)], 1);
    }
}

// cutoff[p] = the largest T in 1 .. kBins - 1 with count(score >= T) >= quota, 1 if there are fewer survivors than the quota,
// kBins (nothing passes) for a quota of 0
__global__ __launch_bounds__(kThreads) void cutoff_kernel(const DevPlane* __restrict__ planes, const int32_t* __restrict__ histogram,
                                                          int32_t* __restrict__ cutoff) {
    constexpr int kPer = kBins / kThreads;          // thread i owns bins kBins - kPer (i + 1) .. kBins - kPer i - 1: from the top
    __shared__ int s_sum[kThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int quota = planes[p].quota;
    const int32_t* __restrict__ h = histogram + (int64_t)p * kBins;
    const int top = kBins - kPer * tid;
    int own = 0;
#pragma unroll
    for (int k = 1; k <= kPer; ++k) own += h[top - k];
    s_sum[tid] = own;
    __syncthreads();
    for (int step = 1; step < kThreads; step <<= 1) {   // inclusive scan
        const int add = tid >= step ? s_sum[tid - step] : 0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    if (tid == 0) {
        if (quota <= 0) cutoff[p] = kBins;
        else if (s_sum[kThreads - 1] < quota) cutoff[p] = 1;
    }
    const int through = s_sum[tid], before = through - own;
    if (quota > 0 && before < quota && through >= quota) {   // exactly one thread
        int count = before, T = top;
        for (int k = 1; k <= kPer; ++k) {
            count += h[top - k];
            if (count >= quota) {
                T = top - k;
                break;
            }
        }
        cutoff[p] = max(T, 1);
    }
}

__global__ __launch_bounds__(kThreads) void collect_kernel(const DevPlane* __restrict__ planes, int n,
                                                           const uint16_t* __restrict__ kept, const int32_t* __restrict__ cutoff,
                                                           int32_t capacity, int32_t* __restrict__ counter,
                                                           sfm_keypoint_candidate* __restrict__ candidates) {
    const Tile t = tile_of_block(planes, n, 0);
    const int W = t.plane.width, H = t.plane.height;
    const int need = cutoff[t.index];
    const int x = t.x0 + (int)(threadIdx.x % kTileW);
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int y = t.y0 + (int)(threadIdx.x / kTileW) + k * kRowStep;
        if (y >= H) break;
        const int s = kept[t.plane.offset + (int64_t)y * W + x];
        if (s > 0 && s >= need) {
            const int slot = atomicAdd(counter, 1);
            if (slot >= 0 && slot < capacity) {
                sfm_keypoint_candidate c;
                c.plane = t.index;
                c.x = x;
                c.y = y;
                c.score = s;
                candidates[slot] = c;
            }
        }
    }
}

__global__ __launch_bounds__(kWave) void keypoint_describe_kernel(
    const DevPlane* __restrict__ planes, const uint8_t* __restrict__ pool, const int32_t* __restrict__ counter, int32_t capacity,
    const sfm_keypoint_candidate* __restrict__ candidates, const int32_t* __restrict__ offsets,
    const long long* __restrict__ boundaries, int bins, unsigned long long* __restrict__ desc, uint8_t* __restrict__ ok,
    uint8_t* __restrict__ angle_bin) {
    const int f = blockIdx.x;
    const int found = *counter;                     // block-uniform; a counter beyond the capacity describes the slots there are
    if (f >= found || f >= capacity) return;
    const sfm_keypoint_candidate c = candidates[f];
    const DevPlane plane = planes[c.plane];
    sfmbrief::describe_feature(pool + plane.offset, plane.height, plane.width, (double)c.x, (double)c.y, offsets, boundaries, bins,
                               desc + (int64_t)f * sfmbrief::kWords, ok + f, angle_bin + f);
}

struct Layout {
    DevPlane* planes;
    int32_t* histogram;
    int32_t* cutoff;
    int64_t bytes;
};

Layout carve(void* workspace, int64_t planes) {
    sfmhost::Carver c{reinterpret_cast<uintptr_t>(workspace), 0};
    Layout l;
    l.planes = c.take<DevPlane>(planes + 1);
    l.histogram = c.take<int32_t>(planes * kBins);
    l.cutoff = c.take<int32_t>(planes);
    l.bytes = c.at;
    return l;
}

// What sfm_detect_keypoints and sfm_build_pyramid share behind their own size and pointer checks: the caller's table against
// the rules of the header (sfmplanes::check_table, SFM_EINVAL under the caller's name `fn` before anything is enqueued), the
// table's upload (it is pageable host memory: the copy has left it when the call returns) and one pyramid_level_kernel launch
// per level above 0, over the images that have it.
int build_pyramid(const char* fn, const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, uint8_t* pool,
                  int64_t pool_bytes, DevPlane* planes_dev, hipStream_t st, CheckedTable& checked) {
    if (sfmplanes::check_table(fn, plane_table, planes, images, pool_bytes, checked) != SFM_OK) return SFM_EINVAL;
    const std::vector<DevPlane>& table = checked.table;
    if (hipMemcpyAsync(planes_dev, table.data(), sizeof(DevPlane) * table.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        return check_launch(fn);
    const int n = (int)planes;
    for (size_t l = 1; l + 1 < checked.level_first.size(); ++l) {
        const int first = table[(size_t)checked.level_first[l]].tile_start, last = table[(size_t)checked.level_first[l + 1]].tile_start;
        hipLaunchKernelGGL(pyramid_level_kernel, dim3((unsigned)(last - first)), dim3(kThreads), 0, st, planes_dev, n, first, pool);
    }
    return SFM_OK;
}

}  // namespace

extern "C" {

int64_t sfm_build_pyramid_workspace_bytes(int64_t planes) {
    if (planes < 0 || planes > kMaxPlanes) return -1;
    sfmhost::Carver c{0, 0};
    c.take<DevPlane>(planes + 1);
    return c.at;
}

int sfm_build_pyramid(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, uint8_t* pool, int64_t pool_bytes,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    if (planes < 0 || images < 0 || pool_bytes < 0 || workspace_bytes < 0) return fail(SFM_EINVAL, "sfm_build_pyramid: negative size");
    if (planes > kMaxPlanes) return fail(SFM_EINVAL, "sfm_build_pyramid: more than 65535 planes");
    if (pool_bytes > 0x7FFFFFFFLL || images > 0x7FFFFFFFLL)
        return fail(SFM_EINVAL, "sfm_build_pyramid: the pool and the images must stay below 2^31");
    if (planes == 0) return SFM_OK;
    if (!plane_table || !pool || !workspace) return fail(SFM_EINVAL, "sfm_build_pyramid: null pointer");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return fail(SFM_EINVAL, "sfm_build_pyramid: workspace must be 16-byte aligned");
    if (workspace_bytes < sfm_build_pyramid_workspace_bytes(planes))
        return fail(SFM_EINVAL, "sfm_build_pyramid: workspace smaller than sfm_build_pyramid_workspace_bytes(planes)");
    CheckedTable checked;
    const int rc = build_pyramid("sfm_build_pyramid", plane_table, planes, images, pool, pool_bytes, reinterpret_cast<DevPlane*>(workspace),
                                 (hipStream_t)stream, checked);
    if (rc != SFM_OK) return rc;
    return check_launch("sfm_build_pyramid");
}

int64_t sfm_detect_keypoints_workspace_bytes(int64_t planes) {
    if (planes < 0 || planes > kMaxPlanes) return -1;
    return carve(nullptr, planes).bytes;
}

int sfm_detect_keypoints(const sfm_keypoint_plane* plane_table, int64_t planes, int64_t images, uint8_t* pool, int64_t pool_bytes,
                         int threshold, const int8_t* offsets, const int64_t* boundaries, int bins, uint16_t* score,
                         uint16_t* kept, int64_t capacity, int32_t* counter, sfm_keypoint_candidate* candidates, uint8_t* desc,
                         uint8_t* ok, uint8_t* angle_bin, void* workspace, int64_t workspace_bytes, void* stream) {
    if (planes < 0 || images < 0 || pool_bytes < 0 || capacity < 0 || workspace_bytes < 0)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: negative size");
    if (planes > kMaxPlanes) return fail(SFM_EINVAL, "sfm_detect_keypoints: more than 65535 planes");
    if (pool_bytes > 0x7FFFFFFFLL || capacity > 0x7FFFFFFFLL || images > 0x7FFFFFFFLL)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: the pool, the capacity and the images must stay below 2^31");
    if (threshold < 1 || threshold > 254) return fail(SFM_EINVAL, "sfm_detect_keypoints: threshold must be in 1..254");
    if (bins < 1 || bins > kWave) return fail(SFM_EINVAL, "sfm_detect_keypoints: bins must be in 1..64");
    if (capacity < 1) return fail(SFM_EINVAL, "sfm_detect_keypoints: capacity must be at least 1");
    if (!counter) return fail(SFM_EINVAL, "sfm_detect_keypoints: null pointer");
    if ((reinterpret_cast<uintptr_t>(counter) & 3u) != 0)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: counter must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (planes == 0) {
        if (hipMemsetAsync(counter, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("sfm_detect_keypoints: memset");
        return SFM_OK;
    }
    if (!plane_table || !pool || !offsets || !boundaries || !score || !kept || !candidates || !desc || !ok || !angle_bin || !workspace)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: null pointer");
    if ((reinterpret_cast<uintptr_t>(desc) & 7u) != 0 || (reinterpret_cast<uintptr_t>(offsets) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(boundaries) & 7u) != 0 || (reinterpret_cast<uintptr_t>(score) & 1u) != 0 ||
        (reinterpret_cast<uintptr_t>(kept) & 1u) != 0 || (reinterpret_cast<uintptr_t>(candidates) & 15u) != 0 ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: candidates and workspace must be 16-byte, desc and boundaries 8-byte, "
                                "offsets 4-byte and the score maps 2-byte aligned");
    const Layout layout = carve(workspace, planes);
    if (workspace_bytes < layout.bytes)
        return fail(SFM_EINVAL, "sfm_detect_keypoints: workspace smaller than sfm_detect_keypoints_workspace_bytes(planes)");
    SFM_REQUIRE_GRID("sfm_detect_keypoints", capacity, 1, kWave);
    CheckedTable checked;
    const int rc = build_pyramid("sfm_detect_keypoints", plane_table, planes, images, pool, pool_bytes, layout.planes, st, checked);
    if (rc != SFM_OK) return rc;
    const int64_t tiles = checked.tiles;
    if (hipMemsetAsync(layout.histogram, 0, sizeof(int32_t) * (size_t)planes * kBins, st) != hipSuccess ||
        hipMemsetAsync(counter, 0, sizeof(int32_t), st) != hipSuccess)
        return check_launch("sfm_detect_keypoints: memset");
    const int n = (int)planes;
    hipLaunchKernelGGL(fast_score_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, layout.planes, n, pool, threshold, score);
    hipLaunchKernelGGL(suppress_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, layout.planes, n, score, kept, layout.histogram);
    hipLaunchKernelGGL(cutoff_kernel, dim3((unsigned)planes), dim3(kThreads), 0, st, layout.planes, layout.histogram, layout.cutoff);
    hipLaunchKernelGGL(collect_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, layout.planes, n, kept, layout.cutoff,
                       (int32_t)capacity, counter, candidates);
    hipLaunchKernelGGL(keypoint_describe_kernel, dim3((unsigned)capacity), dim3(kWave), 0, st, layout.planes, pool, counter,
                       (int32_t)capacity, candidates, reinterpret_cast<const int32_t*>(offsets),
                       reinterpret_cast<const long long*>(boundaries), bins, reinterpret_cast<unsigned long long*>(desc), ok,
                       angle_bin);
    return check_launch("sfm_detect_keypoints");
}

}  // extern "C"
