// Plane-sweep depth maps of posed grey images and the forward-backward consistency filter across them.
//
// Every step of both is fp64 + - * / sqrt in a written order (the build has -ffp-contract=off), so a result is a matter of bytes:
// tests/plane_sweep_oracle.py states the same sequence in NumPy.  The camera, the bilinear cell formula and the winner over the
// depth hypotheses are those of sfm_dense.h, which the other dense translation units share.
//
// sfm_plane_sweep, 2 launches whatever the sizes, nothing read back:
//   1. sweep_homography_kernel   one thread per (reference r, source slot s, depth d): G = K (Rrel + trel e3^T / z) K^-1 into the
//                                workspace, or nine NaNs for a bad reference, an absent slot or an invalid depth
//   2. plane_sweep_kernel<R>     grid (tiles, refs), 256 threads own a 16 x 16 tile of one reference view.  The tile with its halo
//                                of `radius` pixels is staged in LDS once (NaN outside the image), and each thread keeps its
//                                window's sums of a and a^2.  Per (depth, source), uniform over the block: the block warps the
//                                source once per halo pixel into a second LDS plane, (16 + 2 radius)^2 bilinear samples instead of
//                                256 (2 radius + 1)^2, and each thread forms the sums of b, b^2 and ab of its window from LDS: rows
//                                left to right, then the row sums top to bottom.  The valid scores of a depth are kept sorted in
//                                eight registers by insertion (equal scores add to the same bits in either order), the running
//                                winner, the cost before it and the cost after it (sfmdense::DepthWinner) in registers as well.
// The LDS rows are 48 doubles apart: two rows of 16 threads then fall into disjoint halves of the 64 banks of an 8-byte read.
// An invalid sample, sum, score or cost is a NaN on the way and in `volume`; nothing is indexed by a run-time value but LDS and
// global memory, so no kernel uses scratch.
//
// sfm_filter_depth_maps, 1 launch: one thread per pixel of a reference view.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_dense.h"

namespace {

using namespace sfmdense;   // dot3, Mat3, mul3, the camera, bilinear_cell, DepthWinner
using sfmhost::aligned_to;
using sfmhost::check_launch;
using sfmhost::fail;
using sfmhost::grid_fits;
using sfmhost::grid_for;

constexpr int kTile = 16;
constexpr int kSweepBlock = kTile * kTile;
constexpr int kHaloStride = 48;   // doubles between LDS rows: 16 mod 32
constexpr int kMaxSources = 8;
constexpr int kMaxDepths = 4096;
constexpr int kSetupBlock = 256;
constexpr int kFilterBlock = 256;

SFM_DEVICE bool slot_present(int32_t src, int32_t ref, int64_t views) { return src >= 0 && (int64_t)src < views && src != ref; }

__global__ __launch_bounds__(kSetupBlock) void sweep_homography_kernel(const double* __restrict__ K, const double* __restrict__ poses,
                                                                       int64_t views, const int32_t* __restrict__ refs,
                                                                       const int32_t* __restrict__ sources,
                                                                       const double* __restrict__ depths, int64_t R, int S, int D,
                                                                       double* __restrict__ G) {
    const int64_t i = (int64_t)blockIdx.x * kSetupBlock + threadIdx.x;
    if (i >= R * S * D) return;
    const int64_t r = i / ((int64_t)S * D), s = (i / D) % S, d = i % D;
    const int32_t ref = refs[r], src = sources[r * S + s];
    const double z = depths[r * D + d];
    double* out = G + i * 9;
    if (ref < 0 || (int64_t)ref >= views || !slot_present(src, ref, views) || !isfinite(z) || !(z > 0.0)) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = NAN;
        return;
    }
    const double* Pr = poses + (int64_t)ref * 12;
    const double* Ps = poses + (int64_t)src * 12;
    Mat3 M;
    double trel[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)   // Rs Rr^T
            M.m[a][b] = dot3(Ps[3 * a], Pr[3 * b], Ps[3 * a + 1], Pr[3 * b + 1], Ps[3 * a + 2], Pr[3 * b + 2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) trel[a] = Ps[9 + a] - dot3(M.m[a][0], Pr[9], M.m[a][1], Pr[10], M.m[a][2], Pr[11]);
#pragma unroll
    for (int a = 0; a < 3; ++a) M.m[a][2] = M.m[a][2] + trel[a] / z;
    Mat3 Km, Ki;
    camera_matrices(K, Km, Ki);
    const Mat3 g = mul3(mul3(Km, M), Ki);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[3 * a + b] = g.m[a][b];
}

struct SweepArgs {
    const uint8_t* images;
    const int32_t *refs, *sources;
    const double *depths, *G;
    int64_t views;
    int H, W, S, D, tiles_x, top_k, min_sources;
    double gate;   // min_variance * n * n
    double *depth, *cost, *volume;
    int32_t *index, *status;
};

template <int RADIUS>
__global__ __launch_bounds__(kSweepBlock) void plane_sweep_kernel(const SweepArgs a) {
    constexpr int kHalo = kTile + 2 * RADIUS;
    constexpr int kWin = 2 * RADIUS + 1;
    constexpr double n = (double)(kWin * kWin);
    __shared__ double ref_tile[kHalo * kHaloStride];
    __shared__ double src_tile[kHalo * kHaloStride];
    const int tid = threadIdx.x, tx = tid & (kTile - 1), ty = tid / kTile;
    const int64_t r = blockIdx.y;
    const int tile_x = blockIdx.x % a.tiles_x, tile_y = blockIdx.x / a.tiles_x;
    const int px = tile_x * kTile + tx, py = tile_y * kTile + ty;
    const int H = a.H, W = a.W, S = a.S, D = a.D;
    const bool inside = px < W && py < H;
    const int64_t plane = (int64_t)H * W;
    const int64_t pixel = r * plane + (int64_t)py * W + px;
    const int32_t ref = a.refs[r];
    if (ref < 0 || (int64_t)ref >= a.views) {   // block-uniform: the filler of a bad reference
        if (inside) {
            a.depth[pixel] = NAN;
            a.cost[pixel] = NAN;
            a.index[pixel] = -1;
            if (a.volume)
                for (int d = 0; d < D; ++d) a.volume[(r * D + d) * plane + (int64_t)py * W + px] = NAN;
        }
        if (blockIdx.x == 0 && tid == 0) a.status[r] = SFM_SWEEP_BAD_REFERENCE;
        return;
    }
    if (blockIdx.x == 0 && tid == 0) a.status[r] = SFM_SWEEP_OK;
    const uint8_t* ref_image = a.images + (int64_t)ref * plane;
    for (int i = tid; i < kHalo * kHalo; i += kSweepBlock) {
        const int hy = i / kHalo, hx = i % kHalo;
        const int gx = tile_x * kTile + hx - RADIUS, gy = tile_y * kTile + hy - RADIUS;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        ref_tile[hy * kHaloStride + hx] = in ? (double)ref_image[(int64_t)gy * W + gx] : NAN;
    }
    __syncthreads();
    double sa = 0.0, saa = 0.0;
#pragma unroll 1
    for (int dy = 0; dy < kWin; ++dy) {
        const double* row = ref_tile + (ty + dy) * kHaloStride + tx;
        double ra = row[0], raa = row[0] * row[0];
#pragma unroll
        for (int dx = 1; dx < kWin; ++dx) {
            ra = ra + row[dx];
            raa = raa + row[dx] * row[dx];
        }
        sa = dy == 0 ? ra : sa + ra;
        saa = dy == 0 ? raa : saa + raa;
    }
    const double va = n * saa - sa * sa;
    const bool va_ok = isfinite(va) && va >= a.gate;

    DepthWinner winner;
    for (int d = 0; d < D; ++d) {
        const double z = a.depths[r * D + d];
        double cost = NAN;
        if (isfinite(z) && z > 0.0) {   // block-uniform
            double v0 = INFINITY, v1 = INFINITY, v2 = INFINITY, v3 = INFINITY, v4 = INFINITY, v5 = INFINITY, v6 = INFINITY, v7 = INFINITY;
            int valid = 0;
            for (int s = 0; s < S; ++s) {
                const int32_t src = a.sources[r * S + s];
                if (!slot_present(src, ref, a.views)) continue;   // block-uniform
                const double* g = a.G + ((r * S + s) * D + d) * 9;
                const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5], g6 = g[6], g7 = g[7], g8 = g[8];
                const uint8_t* image = a.images + (int64_t)src * plane;
                for (int i = tid; i < kHalo * kHalo; i += kSweepBlock) {
                    const int hy = i / kHalo, hx = i % kHalo;
                    const int gx = tile_x * kTile + hx - RADIUS, gy = tile_y * kTile + hy - RADIUS;
                    double b = NAN;
                    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                        const double x = (double)gx, y = (double)gy;
                        const double X = (g0 * x + g1 * y) + g2, Y = (g3 * x + g4 * y) + g5, Wd = (g6 * x + g7 * y) + g8;
                        if (Wd > 0.0) {
                            const double inv = 1.0 / Wd;
                            const double u = X * inv, v = Y * inv;
                            if (u >= 0.0 && u < (double)(W - 1) && v >= 0.0 && v < (double)(H - 1)) {
                                const double xf = floor(u), yf = floor(v);
                                b = bilinear_cell(image + (int64_t)(int)yf * W + (int)xf, W, u - xf, v - yf);
                            }
                        }
                    }
                    src_tile[hy * kHaloStride + hx] = b;
                }
                __syncthreads();
                double sb = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll 1
                for (int dy = 0; dy < kWin; ++dy) {
                    const double* ra = ref_tile + (ty + dy) * kHaloStride + tx;
                    const double* rb = src_tile + (ty + dy) * kHaloStride + tx;
                    double qb = rb[0], qbb = rb[0] * rb[0], qab = ra[0] * rb[0];
#pragma unroll
                    for (int dx = 1; dx < kWin; ++dx) {
                        qb = qb + rb[dx];
                        qbb = qbb + rb[dx] * rb[dx];
                        qab = qab + ra[dx] * rb[dx];
                    }
                    sb = dy == 0 ? qb : sb + qb;
                    sbb = dy == 0 ? qbb : sbb + qbb;
                    sab = dy == 0 ? qab : sab + qab;
                }
                __syncthreads();   // the plane is overwritten by the next source
                const double vb = n * sbb - sb * sb, num = n * sab - sa * sb;
                if (va_ok && isfinite(vb) && isfinite(num) && vb >= a.gate) {
                    double c = 1.0 - num / sqrt(va * vb);
                    if (isfinite(c)) {
                        ++valid;
                        double t;   // insertion into the ascending list v0 .. v7
#define SFM_SWEEP_INSERT(v) \
    if (c < v) {            \
        t = v;              \
        v = c;              \
        c = t;              \
    }
                        SFM_SWEEP_INSERT(v0) SFM_SWEEP_INSERT(v1) SFM_SWEEP_INSERT(v2) SFM_SWEEP_INSERT(v3)
                        SFM_SWEEP_INSERT(v4) SFM_SWEEP_INSERT(v5) SFM_SWEEP_INSERT(v6) SFM_SWEEP_INSERT(v7)
#undef SFM_SWEEP_INSERT
                    }
                }
            }
            if (valid >= a.min_sources) {
                const int take = a.top_k > 0 && a.top_k < valid ? a.top_k : valid;
                double sum = v0;
                if (take > 1) sum = sum + v1;
                if (take > 2) sum = sum + v2;
                if (take > 3) sum = sum + v3;
                if (take > 4) sum = sum + v4;
                if (take > 5) sum = sum + v5;
                if (take > 6) sum = sum + v6;
                if (take > 7) sum = sum + v7;
                cost = sum / (double)take;
            }
        }
        if (a.volume && inside) a.volume[(r * D + d) * plane + (int64_t)py * W + px] = cost;
        winner.offer(d, cost);
    }
    if (!inside) return;
    a.depth[pixel] = winner.depth(a.depths + r * D, D);
    a.cost[pixel] = winner.best_cost;
    a.index[pixel] = winner.best;
}

__global__ __launch_bounds__(kFilterBlock) void filter_depth_maps_kernel(const double* __restrict__ depth, int64_t views, int H, int W,
                                                                         const double* __restrict__ K, const double* __restrict__ poses,
                                                                         const int32_t* __restrict__ refs,
                                                                         const int32_t* __restrict__ sources, int S, double max_pixel_error,
                                                                         double max_relative_depth_error, int min_consistent,
                                                                         int32_t* __restrict__ count, double* __restrict__ filtered,
                                                                         double* __restrict__ points, int32_t* __restrict__ status) {
    const int64_t r = blockIdx.y, plane = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * kFilterBlock + threadIdx.x;
    const int32_t ref = refs[r];
    const bool bad = ref < 0 || (int64_t)ref >= views;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[r] = bad ? SFM_SWEEP_BAD_REFERENCE : SFM_SWEEP_OK;
    if (i >= plane) return;
    const int64_t at = r * plane + i;
    int agreeing = 0;
    double Xw[3] = {NAN, NAN, NAN};
    double kept = NAN;
    const double d = bad ? NAN : depth[(int64_t)ref * plane + i];
    if (isfinite(d)) {
        Mat3 Km, Ki;
        camera_matrices(K, Km, Ki);
        const double* Pr = poses + (int64_t)ref * 12;
        const double x = (double)(i % W), y = (double)(i / W);
        back_project(Ki, Pr, x, y, d, Xw);
        const double limit = max_pixel_error * max_pixel_error, near = max_relative_depth_error * d;
        for (int s = 0; s < S; ++s) {
            const int32_t src = sources[r * S + s];
            if (!slot_present(src, ref, views)) continue;
            const double* Ps = poses + (int64_t)src * 12;
            double u, v, z;
            project(Km, Ps, Xw, u, v, z);
            if (!(z > 0.0)) continue;
            const double xs = floor(u + 0.5), ys = floor(v + 0.5);
            if (!(xs >= 0.0 && xs < (double)W && ys >= 0.0 && ys < (double)H)) continue;
            const double ds = depth[(int64_t)src * plane + (int64_t)(int)ys * W + (int)xs];
            if (!isfinite(ds)) continue;
            double Xb[3], xr, yr, zr;
            back_project(Ki, Ps, xs, ys, ds, Xb);
            project(Km, Pr, Xb, xr, yr, zr);
            const double ex = xr - x, ey = yr - y;
            if (ex * ex + ey * ey <= limit && fabs(zr - d) <= near) ++agreeing;
        }
        if (agreeing >= min_consistent) kept = d;
    }
    const bool keep = kept == kept;
    count[at] = agreeing;
    filtered[at] = kept;
    points[at * 3 + 0] = keep ? Xw[0] : NAN;
    points[at * 3 + 1] = keep ? Xw[1] : NAN;
    points[at * 3 + 2] = keep ? Xw[2] : NAN;
}

bool image_sizes_ok(int64_t views, int64_t height, int64_t width, int64_t refs, int64_t sources) {
    return sfmhost::image_stack_ok(views, height, width) && refs >= 0 && refs <= 65535 && sources >= 1 && sources <= kMaxSources;
}

// the sizes of a sweep whatever its radius: the smallest window (radius 1) must fit
bool sweep_sizes_ok(int64_t views, int64_t height, int64_t width, int64_t refs, int64_t sources, int64_t depths) {
    return image_sizes_ok(views, height, width, refs, sources) && height >= 4 && width >= 4 && depths >= 1 && depths <= kMaxDepths;
}

int64_t sweep_bytes(int64_t refs, int64_t sources, int64_t depths) {
    sfmhost::Carver c{0, 0};
    c.take<double>(refs * sources * depths * 9);
    return c.at;
}

template <int RADIUS>
void launch_sweep(dim3 grid, hipStream_t st, const SweepArgs& a) {
    hipLaunchKernelGGL(plane_sweep_kernel<RADIUS>, grid, dim3(kSweepBlock), 0, st, a);
}

}  // namespace

extern "C" {

int64_t sfm_plane_sweep_workspace_bytes(int64_t views, int64_t height, int64_t width, int64_t refs, int64_t sources, int64_t depths) {
    return sweep_sizes_ok(views, height, width, refs, sources, depths) ? sweep_bytes(refs, sources, depths) : -1;
}

int sfm_plane_sweep(const uint8_t* images, int64_t views, int64_t height, int64_t width, const double* K, const double* poses,
                    const int32_t* refs, int64_t ref_count, const int32_t* sources, int64_t source_count, const double* depths,
                    int64_t depth_count, int radius, int top_k, int min_sources, double min_variance, double* depth, int32_t* index,
                    double* cost, int32_t* status, double* volume, void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (!sweep_sizes_ok(views, height, width, ref_count, source_count, depth_count))
        return fail(SFM_EINVAL, "sfm_plane_sweep: need views >= 1, height * width < 2^31, 0 <= refs <= 65535, 1 <= sources <= 8 and "
                                "1 <= depths <= 4096");
    if (radius < 1 || radius > 5) return fail(SFM_EINVAL, "sfm_plane_sweep: radius must be in [1, 5]");
    if (height < 2 * radius + 2 || width < 2 * radius + 2)
        return fail(SFM_EINVAL, "sfm_plane_sweep: height and width must be at least 2 * radius + 2");
    if (top_k < 0 || min_sources < 1) return fail(SFM_EINVAL, "sfm_plane_sweep: need top_k >= 0 and min_sources >= 1");
    if (!(min_variance >= 0.0) || !isfinite(min_variance)) return fail(SFM_EINVAL, "sfm_plane_sweep: min_variance must be finite and >= 0");
    const int64_t tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    if (!grid_fits(tiles_x * tiles_y, 1, kSweepBlock, ref_count) ||
        !grid_fits(ref_count * source_count * depth_count, kSetupBlock, kSetupBlock))
        return fail(SFM_EINVAL, "sfm_plane_sweep: size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (ref_count == 0) return SFM_OK;
    if (!images || !K || !poses || !refs || !sources || !depths || !depth || !index || !cost || !status || !workspace)
        return fail(SFM_EINVAL, "sfm_plane_sweep: null pointer");
    if (!aligned_to(K, 8) || !aligned_to(poses, 8) || !aligned_to(depths, 8) || !aligned_to(depth, 8) || !aligned_to(cost, 8) ||
        !aligned_to(volume, 8) || !aligned_to(refs, 4) || !aligned_to(sources, 4) || !aligned_to(index, 4) || !aligned_to(status, 4) ||
        !aligned_to(workspace, 16))
        return fail(SFM_EINVAL, "sfm_plane_sweep: misaligned pointer (doubles 8, int32 4, the workspace 16 bytes)");
    if (workspace_bytes < sweep_bytes(ref_count, source_count, depth_count))
        return fail(SFM_EINVAL, "sfm_plane_sweep: workspace too small (sfm_plane_sweep_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    double* G = (double*)workspace;
    const int S = (int)source_count, D = (int)depth_count;
    hipLaunchKernelGGL(sweep_homography_kernel, dim3(grid_for(ref_count * S * D, kSetupBlock)), dim3(kSetupBlock), 0, st, K, poses, views,
                       refs, sources, depths, ref_count, S, D, G);
    const double n = (double)((2 * radius + 1) * (2 * radius + 1));
    SweepArgs a{};
    a.images = images, a.refs = refs, a.sources = sources, a.depths = depths, a.G = G, a.views = views;
    a.H = (int)height, a.W = (int)width, a.S = S, a.D = D, a.tiles_x = (int)tiles_x, a.top_k = top_k, a.min_sources = min_sources;
    a.gate = min_variance * n * n;
    a.depth = depth, a.cost = cost, a.volume = volume, a.index = index, a.status = status;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)ref_count);
    switch (radius) {
        case 1: launch_sweep<1>(grid, st, a); break;
        case 2: launch_sweep<2>(grid, st, a); break;
        case 3: launch_sweep<3>(grid, st, a); break;
        case 4: launch_sweep<4>(grid, st, a); break;
        default: launch_sweep<5>(grid, st, a); break;
    }
    return check_launch("sfm_plane_sweep");
}

int sfm_filter_depth_maps(const double* depth, int64_t views, int64_t height, int64_t width, const double* K, const double* poses,
                          const int32_t* refs, int64_t ref_count, const int32_t* sources, int64_t source_count, double max_pixel_error,
                          double max_relative_depth_error, int min_consistent, int32_t* count, double* filtered, double* points,
                          int32_t* status, void* stream) {
    if (!image_sizes_ok(views, height, width, ref_count, source_count))
        return fail(SFM_EINVAL, "sfm_filter_depth_maps: need views >= 1, 1 <= height * width < 2^31, 0 <= refs <= 65535 and "
                                "1 <= sources <= 8");
    if (!(max_pixel_error >= 0.0) || !(max_relative_depth_error >= 0.0) || !isfinite(max_pixel_error) ||
        !isfinite(max_relative_depth_error) || min_consistent < 0)
        return fail(SFM_EINVAL, "sfm_filter_depth_maps: the error bounds must be finite and >= 0, min_consistent >= 0");
    if (!grid_fits(height * width, kFilterBlock, kFilterBlock, ref_count))
        return fail(SFM_EINVAL, "sfm_filter_depth_maps: size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (ref_count == 0) return SFM_OK;
    if (!depth || !K || !poses || !refs || !sources || !count || !filtered || !points || !status)
        return fail(SFM_EINVAL, "sfm_filter_depth_maps: null pointer");
    if (!aligned_to(depth, 8) || !aligned_to(K, 8) || !aligned_to(poses, 8) || !aligned_to(filtered, 8) || !aligned_to(points, 8) ||
        !aligned_to(refs, 4) || !aligned_to(sources, 4) || !aligned_to(count, 4) || !aligned_to(status, 4))
        return fail(SFM_EINVAL, "sfm_filter_depth_maps: misaligned pointer (doubles 8, int32 4 bytes)");
    hipLaunchKernelGGL(filter_depth_maps_kernel, dim3(grid_for(height * width, kFilterBlock), (unsigned)ref_count), dim3(kFilterBlock), 0,
                       (hipStream_t)stream, depth, views, (int)height, (int)width, K, poses, refs, sources, (int)source_count,
                       max_pixel_error, max_relative_depth_error, min_consistent, count, filtered, points, status);
    return check_launch("sfm_filter_depth_maps");
}

}  // extern "C"
