// Orders of bundle-style observations (camera_index[M], point_index[M]), built once per call on the device.
//
// Point-major: a counting sort by point (integer atomics), a multi-workgroup exclusive scan of the counts, a scatter, then
// each point's run sorted by observation index.  The result does not depend on the order the atomics ran in:
// ord[off[p] .. off[p+1]) lists point p's observations in increasing observation index.  An index out of range sets *flag
// and every later step returns at once (the order is then undefined).  Used by sfm_tracks.hip,
// sfm_tracks_robust.hip (§6ae) and both bundle adjusters.
//
// Camera-major, after the point-major order: a stable LSD radix sort of the point-major positions on the camera index,
// 8 bits per pass (per-tile digit counts: 256 words per 1 024 observations, whatever the camera count), so that inside a
// camera the observations are sorted by point.  Used by both bundle adjusters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"

namespace sfmorder {

constexpr int kThreads = 256;
constexpr int kScanPerThread = 16;
constexpr int kScanTile = kThreads * kScanPerThread;   // counts per workgroup of the first scan level
constexpr int kTotalsThreads = 1024;
constexpr int kRadixTile = 1024;   // observations per workgroup of a radix pass
constexpr int kRadixBits = 8;
constexpr int kDigits = 1 << kRadixBits;

// Device buffers of the order.  off: [P + 1] (counts, then exclusive offsets, off[P] = M); fill: [P]; ord: [M];
// tile_sum: [tiles(P)]; flag: one int32, 0 or 1 (index out of range).
struct PointOrder {
    int32_t *off, *fill, *ord, *tile_sum, *flag;
};

inline int64_t tiles(int64_t P) { return (P + kScanTile - 1) / kScanTile; }

// Device buffers of the camera-major order.  camp: [M], the camera of every point-major position; seq0, seq1: [M], the
// radix passes' sequences; table: [table_size(M)]; table_sum: [tiles(table_size(M))]; off: [C + 1], the first position of
// every camera and off[C] = M; obs, pt: [M], the observation and the point of every camera-major position.
struct CameraOrder {
    int32_t *camp, *seq0, *seq1, *table, *table_sum, *off, *obs, *pt;
};

inline int64_t radix_tiles(int64_t M) { return (M + kRadixTile - 1) / kRadixTile; }
inline int64_t table_size(int64_t M) { return kDigits * radix_tiles(M) + 1; }

namespace {

// counts per point (off must be zero and *flag 0 before); an out-of-range index sets *flag
__global__ __launch_bounds__(kThreads) void order_count_kernel(const int32_t* __restrict__ cam, const int32_t* __restrict__ pt,
                                                               int M, int C, int P, PointOrder o) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    const int c = cam[m], p = pt[m];
    if (c < 0 || c >= C || p < 0 || p >= P)
        *o.flag = 1;   // every offender stores the same value
    else
        atomicAdd(o.off + p, 1);
}

// inclusive sum over the workgroup: shuffles inside each wave, then the wave totals through LDS
SFM_DEVICE int32_t block_inclusive(int32_t v, int32_t* wave_total, int32_t* total) {
    constexpr int kWaves = kThreads / kWave;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t up = __shfl_up(v, d, kWave);
        if (lane >= d) v += up;
    }
    if (lane == kWave - 1) wave_total[wave] = v;
    __syncthreads();
    int32_t below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        below += w < wave ? wave_total[w] : 0;
        all += wave_total[w];
    }
    __syncthreads();
    *total = all;
    return v + below;
}

// level 1: exclusive offsets inside each tile of kScanTile counts (in place), the tile's total to tile_sum
__global__ __launch_bounds__(kThreads) void order_scan_tiles_kernel(int P, PointOrder o) {
    __shared__ int32_t wave_total[kThreads / kWave];
    if (*o.flag) return;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    int32_t carry = 0;
    for (int pass = 0; pass < kScanPerThread; ++pass) {
        const int64_t i = base + pass * kThreads + threadIdx.x;
        const int32_t v = i < P ? o.off[i] : 0;
        int32_t all;
        const int32_t inc = block_inclusive(v, wave_total, &all);
        if (i < P) o.off[i] = carry + inc - v;
        carry += all;
    }
    if (threadIdx.x == 0) o.tile_sum[blockIdx.x] = carry;
}

// level 2: exclusive scan of the tile totals (chunked over one workgroup); off[P] = the grand total (= M)
__global__ __launch_bounds__(kTotalsThreads) void order_scan_totals_kernel(int P, int T, PointOrder o) {
    __shared__ int32_t sums[kTotalsThreads];
    if (*o.flag) return;
    const int tid = threadIdx.x;
    const int chunk = (T + kTotalsThreads - 1) / kTotalsThreads;
    const int lo = min(T, tid * chunk), hi = min(T, lo + chunk);
    int32_t s = 0;
    for (int t = lo; t < hi; ++t) s += o.tile_sum[t];
    sums[tid] = s;
    __syncthreads();
    for (int d = 1; d < kTotalsThreads; d <<= 1) {
        const int32_t below = tid >= d ? sums[tid - d] : 0;
        __syncthreads();
        sums[tid] += below;
        __syncthreads();
    }
    int32_t run = sums[tid] - s;
    for (int t = lo; t < hi; ++t) {
        const int32_t n = o.tile_sum[t];
        o.tile_sum[t] = run;
        run += n;
    }
    if (tid == kTotalsThreads - 1) o.off[P] = sums[tid];
}

// level 3: add each tile's base; fill = off
__global__ __launch_bounds__(kThreads) void order_scan_add_kernel(int P, PointOrder o) {
    if (*o.flag) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int32_t v = o.off[p] + o.tile_sum[p / kScanTile];
    o.off[p] = v;
    o.fill[p] = v;
}

__global__ __launch_bounds__(kThreads) void order_scatter_kernel(const int32_t* __restrict__ pt, int M, PointOrder o) {
    if (*o.flag) return;
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    o.ord[atomicAdd(o.fill + pt[m], 1)] = m;
}

// each point's run sorted by observation index (insertion sort: runs hold a few observations)
__global__ __launch_bounds__(kThreads) void order_sort_runs_kernel(int P, PointOrder o) {
    if (*o.flag) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    int32_t* run = o.ord + o.off[p];
    const int n = o.off[p + 1] - o.off[p];
    for (int i = 1; i < n; ++i) {
        const int32_t v = run[i];
        int j = i - 1;
        while (j >= 0 && run[j] > v) {
            run[j + 1] = run[j];
            --j;
        }
        run[j + 1] = v;
    }
}

// After the point order: the camera of every point-major position and the identity sequence the radix passes sort
__global__ __launch_bounds__(kThreads) void order_positions_kernel(const int32_t* __restrict__ cam, int M, PointOrder o,
                                                                   CameraOrder co) {
    if (*o.flag) return;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= M) return;
    co.camp[q] = cam[o.ord[q]];
    co.seq0[q] = q;
}

// One stable LSD radix pass over the sequence src of point-major positions, keyed by the digit of their camera at
// `shift`.  kScatter = false: the tile's count of every digit to table[digit * tiles + tile].  kScatter = true (after the
// exclusive scan of the table): every position to its place in dst.  Rank inside a tile: the lanes of a wave with the same
// digit by 8 ballots, then the waves in order.
template <bool kScatter>
__global__ __launch_bounds__(kRadixTile) void order_radix_kernel(int M, int shift, int tiles, const int32_t* __restrict__ src,
                                                                 int32_t* __restrict__ dst, PointOrder o, CameraOrder co) {
    constexpr int kWaves = kRadixTile / kWave;
    __shared__ int32_t wcount[kWaves][kDigits];
    if (*o.flag) return;
    for (int k = threadIdx.x; k < kWaves * kDigits; k += kRadixTile) (&wcount[0][0])[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = blockIdx.x * kRadixTile + threadIdx.x;
    const bool valid = i < M;
    const int32_t q = valid ? src[i] : 0;
    const int d = valid ? (co.camp[q] >> shift) & (kDigits - 1) : 0;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < kRadixBits; ++bit) {
        const bool set = (d >> bit) & 1;
        const uint64_t b = __ballot(set);
        peers &= set ? b : ~b;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcount[wave][d] = __popcll(peers);
    __syncthreads();
    if (!kScatter) {
        for (int k = threadIdx.x; k < kDigits; k += kRadixTile) {
            int32_t n = 0;
            for (int v = 0; v < kWaves; ++v) n += wcount[v][k];
            co.table[(int64_t)k * tiles + blockIdx.x] = n;
        }
    } else if (valid) {
        int32_t before = 0;
        for (int v = 0; v < wave; ++v) before += wcount[v][d];
        dst[co.table[(int64_t)d * tiles + blockIdx.x] + before + rank] = q;
    }
}

// After the last pass: camera-major position i -> observation and point; off[c] = first position of camera c
__global__ __launch_bounds__(kThreads) void order_camera_kernel(const int32_t* __restrict__ pt, int M, int C,
                                                                const int32_t* __restrict__ seq, PointOrder o, CameraOrder co) {
    if (*o.flag) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i > M) return;
    const int key = i < M ? co.camp[seq[i]] : C;
    const int prev = i > 0 ? co.camp[seq[i - 1]] : -1;
    for (int c = prev + 1; c <= key; ++c) co.off[c] = i;
    if (i < M) {
        const int32_t m = o.ord[seq[i]];
        co.obs[i] = m;
        co.pt[i] = pt[m];
    }
}

}  // namespace

// Enqueue the order on `st`.  Before it: off[0 .. P] and *flag zeroed on the same stream.  0 <= C, P, M < 2^31 (the caller
// has checked them); nothing is launched for an empty dimension.
inline void launch_point_order(const int32_t* cam, const int32_t* pt, int64_t M, int64_t C, int64_t P, const PointOrder& o,
                               hipStream_t st) {
    const unsigned mgrid = sfmhost::grid_for(M, kThreads), pgrid = sfmhost::grid_for(P, kThreads);
    if (M > 0) hipLaunchKernelGGL(order_count_kernel, dim3(mgrid), dim3(kThreads), 0, st, cam, pt, (int)M, (int)C, (int)P, o);
    if (P > 0) {
        const int T = (int)tiles(P);
        hipLaunchKernelGGL(order_scan_tiles_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, (int)P, o);
        hipLaunchKernelGGL(order_scan_totals_kernel, dim3(1), dim3(kTotalsThreads), 0, st, (int)P, T, o);
        hipLaunchKernelGGL(order_scan_add_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, o);
    }
    if (M > 0) hipLaunchKernelGGL(order_scatter_kernel, dim3(mgrid), dim3(kThreads), 0, st, pt, (int)M, o);
    if (P > 0) hipLaunchKernelGGL(order_sort_runs_kernel, dim3(pgrid), dim3(kThreads), 0, st, (int)P, o);
}

// Exclusive scan of n counts in place (counts[0 .. n), counts[n] = their total) by the point order's three scan levels.
// Its level 3 also writes `fill`, here the same array: both stores of a thread carry the same value.
inline void launch_scan(int32_t* counts, int64_t n, int32_t* tile_sum, int32_t* flag, hipStream_t st) {
    const PointOrder o{counts, counts, nullptr, tile_sum, flag};
    const int T = (int)tiles(n);
    hipLaunchKernelGGL(order_scan_tiles_kernel, dim3((unsigned)T), dim3(kThreads), 0, st, (int)n, o);
    hipLaunchKernelGGL(order_scan_totals_kernel, dim3(1), dim3(kTotalsThreads), 0, st, (int)n, T, o);
    hipLaunchKernelGGL(order_scan_add_kernel, dim3(sfmhost::grid_for(n, kThreads)), dim3(kThreads), 0, st, (int)n, o);
}

// Enqueue the camera-major order on `st`, after launch_point_order on the same stream.  Returns the sequence (co.seq0 or
// co.seq1) that holds the point-major position of every camera-major position once the order has run.
inline const int32_t* launch_camera_order(const int32_t* cam, const int32_t* pt, int64_t M, int64_t C, const PointOrder& o,
                                          const CameraOrder& co, hipStream_t st) {
    const int rtiles = (int)radix_tiles(M);
    hipLaunchKernelGGL(order_positions_kernel, dim3(sfmhost::grid_for(M, kThreads)), dim3(kThreads), 0, st, cam, (int)M, o, co);
    int32_t *src = co.seq0, *dst = co.seq1;
    for (int shift = 0; M > 0 && ((C - 1) >> shift) > 0; shift += kRadixBits) {
        hipLaunchKernelGGL(order_radix_kernel<false>, dim3(rtiles), dim3(kRadixTile), 0, st, (int)M, shift, rtiles, src, dst, o,
                           co);
        launch_scan(co.table, table_size(M) - 1, co.table_sum, o.flag, st);
        hipLaunchKernelGGL(order_radix_kernel<true>, dim3(rtiles), dim3(kRadixTile), 0, st, (int)M, shift, rtiles, src, dst, o,
                           co);
        int32_t* t = src;
        src = dst;
        dst = t;
    }
    hipLaunchKernelGGL(order_camera_kernel, dim3(sfmhost::grid_for(M + 1, kThreads)), dim3(kThreads), 0, st, pt, (int)M,
                       (int)C, src, o, co);
    return src;
}

}  // namespace sfmorder
