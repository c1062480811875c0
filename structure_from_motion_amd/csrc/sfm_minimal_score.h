// What the minimal solvers of RANSAC share behind their fit (sfm_minimal_fit.h): the all-fp64 scoring of one hypothesis per lane
// over every item, and the winner's inlier mask — the homography (sfm_homography.hip), both models of the view graph
// (sfm_view_graph.hip) and the mask of the PnP pose (sfm_pnp.hip, whose scorer keeps a copy of the loop for the reason given
// there).  The five-point pass scores with score_sed_exact_kernel (hypotheses per wave).
//
// A model is a struct with
//   Stored, kStride   items are kStride consecutive Stored in memory (so entry b of a dense batch begins at b * n * kStride);
//   Item              what one tile slot holds;
//   kModel            doubles per model;
//   Model(m, params...)   device constructor from the lane's model pointer and whatever its error needs by value;
//   load(items, i, slot)   static device function: item i of `items` (const Stored*) into `slot`, an Item in LDS or registers
//                     (filled in place: an Item returned by value reaches a tile as scalar stores, not as 16-byte ones);
//   error(item)       device function: the error of one Item under this model, every operation in fp64 and rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"

namespace sfmmin {

constexpr int kScoreBlock = 256;
constexpr int kScoreTile = 512;   // items per tile: 16 KiB of LDS for a Corr, 24 KiB for a PnP point

struct HypothesisScore {
    int c;
    double a1, a2;
};

// One hypothesis per lane (its model in registers), the n items staged through LDS in tiles that every lane of the block reads
// at the same address (broadcast).  c = non-sample items with e <= thr; a1 / a2 = sums of e / e^2 over the SAMPLE sample items
// and those survivors (the layout sfm_select_best reads).  The tile loop counts every item; the sample items (the leading
// entries of sample_row) are then corrected: one that passed the gate is taken out of the count (its value is already in the
// sums), one that did not is added to the sums.  Every sum runs in item order in this lane; a NaN error or threshold passes no
// gate, so a NaN model gives NaN sums.  Every lane of the block must call this with the same `items` and n (two barriers per tile).
template <int SAMPLE, class Model>
SFM_DEVICE HypothesisScore score_hypothesis(typename Model::Item* tile, const Model& model,
                                            const typename Model::Stored* items, int64_t n, const int32_t* sample_row,
                                            double thr) {
    int c = 0;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t base = 0; base < n; base += kScoreTile) {
        const int count = (int)(n - base < kScoreTile ? n - base : kScoreTile);
        __syncthreads();   // the previous tile has been read by every lane
        for (int i = threadIdx.x; i < count; i += kScoreBlock) Model::load(items, base + i, tile[i]);
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < count; ++j) {
            const double e = model.error(tile[j]);
            const bool in = e <= thr;
            c += in ? 1 : 0;
            a1 += in ? e : 0.0;
            a2 += in ? e * e : 0.0;
        }
    }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) {
        typename Model::Item q;
        Model::load(items, checked_index(sample_row[k], n, bad), q);
        const double e = model.error(q);
        if (e <= thr) {
            --c;
        } else {
            a1 += e;
            a2 += e * e;
        }
    }
    return HypothesisScore{c, a1, a2};
}

// The dense layout: items [batch, n], models [batch, h_count, kModel], S [batch, h_count, 8]; grid (h_count / 256, batch).
template <int SAMPLE, class Model, class... Params>
__global__ __launch_bounds__(kScoreBlock) void score_kernel(const typename Model::Stored* __restrict__ items, int64_t n,
                                                            const double* __restrict__ model, const int32_t* __restrict__ S,
                                                            int64_t h_count, double thr, int32_t* __restrict__ cnt,
                                                            double* __restrict__ s1, double* __restrict__ s2, Params... params) {
    __shared__ typename Model::Item tile[kScoreTile];
    const int64_t b = blockIdx.y;
    const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    const int64_t hc = h < h_count ? h : h_count - 1;   // lanes past the end score a valid hypothesis and store nothing
    const int64_t bh = b * h_count + hc;
    const HypothesisScore r =
        score_hypothesis<SAMPLE>(tile, Model(model + bh * Model::kModel, params...), items + b * n * Model::kStride, n, S + bh * 8, thr);
    if (h < h_count) {
        cnt[b * h_count + h] = r.c;
        s1[b * h_count + h] = r.a1;
        s2[b * h_count + h] = r.a2;
    }
}

// Mask value of item i under `model`, whose sample is the SAMPLE items at smp: 2 for a sample item, 1 for another item with
// e <= thr, 0 otherwise.
template <int SAMPLE, class Model>
SFM_DEVICE uint8_t mask_value(const Model& model, const int32_t* smp, const typename Model::Item& item, int64_t i, double thr) {
    bool in_sample = false;
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) in_sample |= (smp[k] == (int32_t)i);
    const double e = model.error(item);
    return in_sample ? 2 : ((e <= thr) ? 1 : 0);
}

// mask[b, i] = mask_value under the winner of record b, all 0 when the record holds no model.  Grid-stride over the items; every
// byte of the mask is written.
template <int SAMPLE, class Model, class... Params>
__global__ void mask_kernel(const typename Model::Stored* __restrict__ items, int64_t n, const double* __restrict__ model,
                            const int32_t* __restrict__ S, int64_t h_count, const sfm_select_result* __restrict__ result, double thr,
                            uint8_t* __restrict__ mask, Params... params) {
    const int64_t b = blockIdx.y;
    const int64_t best = result[b].best_h;
    const bool none = best < 0 || best >= h_count;
    const int64_t bh = b * h_count + (none ? 0 : best);
    const typename Model::Stored* P = items + b * n * Model::kStride;
    uint8_t* out = mask + b * n;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (none) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = 0;
        return;
    }
    const Model winner(model + bh * Model::kModel, params...);
    int32_t smp[SAMPLE];
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) smp[k] = S[bh * 8 + k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        typename Model::Item q;
        Model::load(P, i, q);
        out[i] = mask_value<SAMPLE>(winner, smp, q, i, thr);
    }
}

// The launches of the two kernels over `batch` entries; the caller has checked the sizes (check_sizes with kScoreBlock).
template <int SAMPLE, class Model, class... Params>
int launch_score(const typename Model::Stored* items, int64_t n, const double* model, const int32_t* S, int64_t h_count, int64_t batch,
                 double thr, int32_t* cnt, double* s1, double* s2, hipStream_t st, Params... params) {
    const dim3 grid(sfmhost::grid_for(h_count, kScoreBlock), (unsigned)batch);
    hipLaunchKernelGGL((score_kernel<SAMPLE, Model, Params...>), grid, dim3(kScoreBlock), 0, st, items, n, model, S, h_count, thr, cnt, s1,
                       s2, params...);
    return sfmhost::check_launch("sfmmin::score_kernel");
}

template <int SAMPLE, class Model, class... Params>
int launch_mask(const typename Model::Stored* items, int64_t n, const double* model, const int32_t* S, int64_t h_count, int64_t batch,
                const sfm_select_result* result, double thr, uint8_t* mask, hipStream_t st, Params... params) {
    const dim3 grid(sfmhost::grid_stride(n, 256, 1024), (unsigned)batch);
    hipLaunchKernelGGL((mask_kernel<SAMPLE, Model, Params...>), grid, dim3(256), 0, st, items, n, model, S, h_count, result, thr, mask,
                       params...);
    return sfmhost::check_launch("sfmmin::mask_kernel");
}

}  // namespace sfmmin
