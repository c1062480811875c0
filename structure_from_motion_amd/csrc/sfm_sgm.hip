// Semi-global smoothing of the plane-sweep cost volume.
//
// Every step is fp64 + - * / min in a written order (the build has -ffp-contract=off), so a result is a matter of bytes:
// tests/sgm_oracle.py states the same sequence in NumPy.  Every term of a min is finite, so its order does not matter.
//
// sfm_sgm_aggregate, paths + 1 launches whatever the sizes, nothing read back, no atomics, no memset:
//   sgm_vertical_kernel<G>     the directions with dy != 0, one launch each.  Grid (ceil(W / 16), refs), 256 threads = 16 paths x 16
//                              depth groups; the 16 lanes of a DPP row share one path and lane g keeps the G = Dpad / 16 values
//                              L(d), d = g G .. g G + G - 1, of the path's previous pixel in registers.  Path p is at column
//                              (p + dx t) mod W of the t-th row: every pixel of a row belongs to one path, and a path that leaves
//                              the image restarts at the other side with L = C'.  The minimum over d is a DPP butterfly of the
//                              row, the neighbours d - 1 and d + 1 of a lane's first and last value one DPP row shift each: no
//                              LDS and no barrier.  The unary costs and the running sum of the next row are loaded before the
//                              current row is worked on.
//   sgm_horizontal_kernel<G>   the directions (1, 0) and (-1, 0), one launch each.  Grid (ceil(H / 4), refs), 64 threads = 4 image
//                              rows x 16 depth groups.  A tile of 4 rows x XT columns x D is read with x fastest across the lanes,
//                              transposed through LDS, walked column by column with the same step as above, the L values put back
//                              into LDS and added to the running sum with x fastest again.
//   sgm_winner_kernel          one thread per pixel: the eligible hypothesis of lowest sum and the parabola step of the sweep
//                              (sfmdense::DepthWinner, sfm_dense.h).
// The first direction writes the running sum, the later ones add to it in launch order: the left fold of the definition.
// G is 1, 2, 4, 8 or 16 (D up to 16, 32, 64, 128, 256); a value beyond D is +inf in the registers and never stored.  Nothing is
// indexed by a run-time value but LDS and global memory, so no kernel uses scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_dense.h"

namespace {

using sfmhost::aligned_to;
using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_for;

constexpr int kGroups = 16;            // depth groups of a path: one DPP row
constexpr int kMaxDepths = 16 * kGroups;
constexpr int kVerticalPaths = 16;     // paths of a block of the vertical kernel
constexpr int kVerticalBlock = kVerticalPaths * kGroups;
constexpr int kHorizontalRows = 4;     // image rows of a block of the horizontal kernel: one wave
constexpr int kHorizontalBlock = kHorizontalRows * kGroups;
constexpr int kWinnerBlock = 256;

struct SgmArgs {
    const double *volume, *depths;
    double* sum;   // [R, D, H, W]: `aggregated`, or the workspace
    int H, W, D;
    double p1, p2, invalid_cost;
};

// lane i of a DPP row of 16 reads the lane that CTRL names; a lane without a source gets `fill`
template <int CTRL>
SFM_DEVICE double row_move(double v, double fill) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(fill), __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E;             // quad_perm:[1,0,3,2] and [2,3,0,1]
constexpr int kDppHalfMirror = 0x141, kDppMirror = 0x140;   // row_half_mirror, row_mirror
constexpr int kDppShl1 = 0x101, kDppShr1 = 0x111;           // row_shl:1 (lane i reads i + 1), row_shr:1 (lane i reads i - 1)

// the minimum over the 16 lanes of a DPP row, in every lane
SFM_DEVICE double row_min(double v) {
    v = fmin(v, row_move<kDppXor1>(v, v));
    v = fmin(v, row_move<kDppXor2>(v, v));
    v = fmin(v, row_move<kDppHalfMirror>(v, v));
    return fmin(v, row_move<kDppMirror>(v, v));
}

// One pixel of a path.  L: the values of the previous pixel (in: +inf beyond D), replaced by those of this pixel; c: C' here.
template <int G>
SFM_DEVICE void sgm_step(double (&L)[G], const double (&c)[G], bool restart, int g, int D, double p1, double p2) {
    double m = L[0];
#pragma unroll
    for (int j = 1; j < G; ++j) m = fmin(m, L[j]);
    m = row_min(m);
    const double below = row_move<kDppShr1>(L[G - 1], INFINITY);   // L(d - 1) of this lane's first value
    const double above = row_move<kDppShl1>(L[0], INFINITY);       // L(d + 1) of its last one
    const double jump = m + p2;
    double out[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const double lower = j > 0 ? L[j - 1] : below, upper = j < G - 1 ? L[j + 1] : above;
        const double best = fmin(fmin(L[j], lower + p1), fmin(upper + p1, jump));
        out[j] = restart ? c[j] : (c[j] + best) - m;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) L[j] = g * G + j < D ? out[j] : INFINITY;
}

SFM_DEVICE double unary(double v, double invalid_cost) { return isfinite(v) ? v : invalid_cost; }

template <int G>
__global__ __launch_bounds__(kVerticalBlock) void sgm_vertical_kernel(const SgmArgs a, int dx, int dy, int first) {
    const int g = threadIdx.x & (kGroups - 1);
    const int64_t p = (int64_t)blockIdx.x * kVerticalPaths + threadIdx.x / kGroups;
    const int H = a.H, W = a.W, D = a.D;
    const bool active = p < W;   // uniform over a DPP row
    const int64_t plane = (int64_t)H * W;
    const int64_t base = ((int64_t)blockIdx.y * D + g * G) * plane;
    const double* __restrict__ vol = a.volume + base;
    double* __restrict__ sum = a.sum + base;
    int x = active ? (int)p : 0;
    double L[G], c[G], s[G], cn[G], sn[G];
#pragma unroll
    for (int j = 0; j < G; ++j) L[j] = INFINITY, cn[j] = 0.0, sn[j] = 0.0;
    {
        const int64_t at = (int64_t)(dy > 0 ? 0 : H - 1) * W + x;
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (active && g * G + j < D) {
                cn[j] = vol[j * plane + at];
                if (!first) sn[j] = sum[j * plane + at];
            }
    }
    for (int t = 0; t < H; ++t) {
        const int y = dy > 0 ? t : H - 1 - t;
        const bool restart = t == 0 || (dx > 0 && x == 0) || (dx < 0 && x == W - 1);
        const int64_t at = (int64_t)y * W + x;
#pragma unroll
        for (int j = 0; j < G; ++j) c[j] = unary(cn[j], a.invalid_cost), s[j] = sn[j];
        x += dx;
        if (x >= W) x = 0;
        if (x < 0) x = W - 1;
        if (t + 1 < H) {   // the next row, before this one is worked on
            const int64_t next = (int64_t)(dy > 0 ? t + 1 : H - 2 - t) * W + x;
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (active && g * G + j < D) {
                    cn[j] = vol[j * plane + next];
                    if (!first) sn[j] = sum[j * plane + next];
                }
        }
        sgm_step<G>(L, c, restart, g, D, a.p1, a.p2);
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (active && g * G + j < D) sum[j * plane + at] = first ? L[j] : s[j] + L[j];
    }
}

// the columns of a tile of the horizontal kernel: 9.5 KiB to 33.5 KiB of LDS a block
template <int G>
struct HorizontalTile {
    static constexpr int kColumns = G <= 4 ? 16 : G == 8 ? 8 : 4;
    static constexpr int kColumnStride = 16 * G + 2;   // doubles; 2 mod 32: the transposing stores of the columns spread over the banks
    // 16 mod 32: the two rows of 16 lanes that an 8-byte read serves together fall into disjoint halves of the 64 banks
    static constexpr int kRowStride = kColumns * kColumnStride + (48 - kColumns * kColumnStride % 32) % 32;
    static constexpr int kDoubles = kHorizontalRows * kRowStride;
};

template <int G>
__global__ __launch_bounds__(kHorizontalBlock) void sgm_horizontal_kernel(const SgmArgs a, int dx, int first) {
    using Tile = HorizontalTile<G>;
    constexpr int XT = Tile::kColumns, kPerPass = kHorizontalBlock / XT;   // depths a pass of the wave moves for one row
    __shared__ double tile[Tile::kDoubles];
    const int lane = threadIdx.x, g = lane & (kGroups - 1), row = lane / kGroups;
    const int H = a.H, W = a.W, D = a.D;
    const int y0 = blockIdx.x * kHorizontalRows;
    const int64_t plane = (int64_t)H * W;
    const int64_t base = (int64_t)blockIdx.y * D * plane;
    const double* __restrict__ vol = a.volume + base;
    double* __restrict__ sum = a.sum + base;
    const int mc = lane % XT, md = lane / XT;   // the column and the depth within a pass that this lane moves
    double* mine = tile + row * Tile::kRowStride + g;
    const int tiles = (W + XT - 1) / XT;
    double L[G], c[G];
#pragma unroll
    for (int j = 0; j < G; ++j) L[j] = INFINITY;
    for (int k = 0; k < tiles; ++k) {
        const int xb = (dx > 0 ? k : tiles - 1 - k) * XT;
        const bool column = xb + mc < W;
        for (int rr = 0; rr < kHorizontalRows; ++rr) {
            if (y0 + rr >= H) break;   // uniform
            for (int d0 = 0; d0 < D; d0 += kPerPass) {
                const int d = d0 + md;
                if (d < D && column)
                    tile[rr * Tile::kRowStride + mc * Tile::kColumnStride + (d % G) * kGroups + d / G] =
                        unary(vol[d * plane + (int64_t)(y0 + rr) * W + xb + mc], a.invalid_cost);
            }
        }
        __syncthreads();
        for (int i = 0; i < XT; ++i) {
            const int col = dx > 0 ? i : XT - 1 - i;
            if (xb + col >= W) continue;   // uniform
            double* at = mine + col * Tile::kColumnStride;
#pragma unroll
            for (int j = 0; j < G; ++j) c[j] = g * G + j < D ? at[j * kGroups] : 0.0;
            sgm_step<G>(L, c, dx > 0 ? xb + col == 0 : xb + col == W - 1, g, D, a.p1, a.p2);
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (g * G + j < D) at[j * kGroups] = L[j];
        }
        __syncthreads();
        for (int rr = 0; rr < kHorizontalRows; ++rr) {
            if (y0 + rr >= H) break;
            for (int d0 = 0; d0 < D; d0 += kPerPass) {
                const int d = d0 + md;
                if (d < D && column) {
                    const double l = tile[rr * Tile::kRowStride + mc * Tile::kColumnStride + (d % G) * kGroups + d / G];
                    double* out = sum + d * plane + (int64_t)(y0 + rr) * W + xb + mc;
                    *out = first ? l : *out + l;
                }
            }
        }
        __syncthreads();   // the tile is overwritten by the next one
    }
}

// The winner of a pixel: the sweep's rule (sfmdense::DepthWinner) on the sums, a hypothesis that is not eligible counting as NaN.
__global__ __launch_bounds__(kWinnerBlock) void sgm_winner_kernel(const SgmArgs a, double* __restrict__ depth, int32_t* __restrict__ index,
                                                                  double* __restrict__ cost) {
    const int64_t plane = (int64_t)a.H * a.W, i = (int64_t)blockIdx.x * kWinnerBlock + threadIdx.x;
    if (i >= plane) return;
    const int64_t r = blockIdx.y;
    const int D = a.D;
    const double* vol = a.volume + r * D * plane + i;
    const double* sum = a.sum + r * D * plane + i;
    const double* z = a.depths + r * D;
    sfmdense::DepthWinner winner;
    for (int d = 0; d < D; ++d) {
        const double zd = z[d];
        winner.offer(d, isfinite(vol[d * plane]) && isfinite(zd) && zd > 0.0 ? sum[d * plane] : NAN);
    }
    depth[r * plane + i] = winner.depth(z, D);
    cost[r * plane + i] = winner.best_cost;
    index[r * plane + i] = winner.best;
}

bool sgm_sizes_ok(int64_t refs, int64_t depths, int64_t height, int64_t width) {
    // the volume of a reference is a stack of `depths` planes
    return refs >= 0 && refs <= 65535 && depths <= kMaxDepths && sfmhost::image_stack_ok(depths, height, width);
}

int64_t sgm_bytes(int64_t refs, int64_t depths, int64_t height, int64_t width, bool keep_aggregated) {
    if (keep_aggregated) return 0;
    sfmhost::Carver c{0, 0};
    c.take<double>(refs * depths * height * width);
    return c.at;
}

template <int G>
void launch_direction(const SgmArgs& a, int64_t refs, int dx, int dy, int first, hipStream_t st) {
    if (dy != 0)
        hipLaunchKernelGGL(sgm_vertical_kernel<G>, dim3(grid_for(a.W, kVerticalPaths), (unsigned)refs), dim3(kVerticalBlock), 0, st, a, dx, dy,
                           first);
    else
        hipLaunchKernelGGL(sgm_horizontal_kernel<G>, dim3(grid_for(a.H, kHorizontalRows), (unsigned)refs), dim3(kHorizontalBlock), 0, st, a,
                           dx, first);
}

}  // namespace

extern "C" {

int64_t sfm_sgm_workspace_bytes(int64_t refs, int64_t depths, int64_t height, int64_t width, int keep_aggregated) {
    return sgm_sizes_ok(refs, depths, height, width) ? sgm_bytes(refs, depths, height, width, keep_aggregated != 0) : -1;
}

int sfm_sgm_aggregate(const double* volume, int64_t ref_count, int64_t depth_count, int64_t height, int64_t width, const double* depths,
                      double p1, double p2, double invalid_cost, int paths, double* depth, int32_t* index, double* cost,
                      double* aggregated, void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (!sgm_sizes_ok(ref_count, depth_count, height, width))
        return fail(SFM_EINVAL, "sfm_sgm_aggregate: need 0 <= refs <= 65535, 1 <= depths <= 256, height, width >= 1 and "
                                "height * width < 2^31");
    if (paths != 4 && paths != 8) return fail(SFM_EINVAL, "sfm_sgm_aggregate: paths must be 4 or 8");
    if (!isfinite(p1) || !isfinite(p2) || !isfinite(invalid_cost) || !(p1 >= 0.0) || !(p1 <= p2))
        return fail(SFM_EINVAL, "sfm_sgm_aggregate: p1, p2 and invalid_cost must be finite with 0 <= p1 <= p2");
    if (ref_count == 0) return SFM_OK;
    if (!volume || !depths || !depth || !index || !cost || !workspace) return fail(SFM_EINVAL, "sfm_sgm_aggregate: null pointer");
    if (!aligned_to(volume, 8) || !aligned_to(depths, 8) || !aligned_to(depth, 8) || !aligned_to(cost, 8) || !aligned_to(aggregated, 8) ||
        !aligned_to(index, 4) || !aligned_to(workspace, 16))
        return fail(SFM_EINVAL, "sfm_sgm_aggregate: misaligned pointer (doubles 8, int32 4, the workspace 16 bytes)");
    if (aggregated == volume) return fail(SFM_EINVAL, "sfm_sgm_aggregate: aggregated must not be the volume");
    if (workspace_bytes < sgm_bytes(ref_count, depth_count, height, width, aggregated != nullptr))
        return fail(SFM_EINVAL, "sfm_sgm_aggregate: workspace too small (sfm_sgm_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    SgmArgs a{};
    a.volume = volume, a.depths = depths, a.sum = aggregated ? aggregated : (double*)workspace;
    a.H = (int)height, a.W = (int)width, a.D = (int)depth_count;
    a.p1 = p1, a.p2 = p2, a.invalid_cost = invalid_cost;
    static const int kEight[8][2] = {{0, 1}, {1, 1}, {-1, 1}, {0, -1}, {-1, -1}, {1, -1}, {1, 0}, {-1, 0}};
    static const int kFour[4][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}};
    const int(*dir)[2] = paths == 8 ? kEight : kFour;
    for (int k = 0; k < paths; ++k) {
        const int dx = dir[k][0], dy = dir[k][1], first = k == 0;
        if (a.D <= 16) launch_direction<1>(a, ref_count, dx, dy, first, st);
        else if (a.D <= 32) launch_direction<2>(a, ref_count, dx, dy, first, st);
        else if (a.D <= 64) launch_direction<4>(a, ref_count, dx, dy, first, st);
        else if (a.D <= 128) launch_direction<8>(a, ref_count, dx, dy, first, st);
        else launch_direction<16>(a, ref_count, dx, dy, first, st);
    }
    hipLaunchKernelGGL(sgm_winner_kernel, dim3(grid_for(height * width, kWinnerBlock), (unsigned)ref_count), dim3(kWinnerBlock), 0, st, a,
                       depth, index, cost);
    return check_launch("sfm_sgm_aggregate");
}

}  // extern "C"
