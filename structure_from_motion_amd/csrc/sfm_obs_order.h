// Point-major order of bundle-style observations (camera_index[M], point_index[M]), built once per call on the device:
// a counting sort by point (integer atomics), a multi-workgroup exclusive scan of the counts, a scatter, then each point's
// run sorted by observation index.  The result does not depend on the order the atomics ran in: ord[off[p] .. off[p+1])
// lists point p's observations in increasing observation index.  An index out of range sets *flag and every later step
// returns at once (the order is then undefined).  Used by sfm_tracks.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"

namespace sfmorder {

constexpr int kThreads = 256;
constexpr int kScanPerThread = 16;
constexpr int kScanTile = kThreads * kScanPerThread;   // counts per workgroup of the first scan level
constexpr int kTotalsThreads = 1024;

// Device buffers of the order.  off: [P + 1] (counts, then exclusive offsets, off[P] = M); fill: [P]; ord: [M];
// tile_sum: [tiles(P)]; flag: one int32, 0 or 1 (index out of range).
struct PointOrder {
    int32_t *off, *fill, *ord, *tile_sum, *flag;
};

inline int64_t tiles(int64_t P) { return (P + kScanTile - 1) / kScanTile; }

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

}  // namespace sfmorder
