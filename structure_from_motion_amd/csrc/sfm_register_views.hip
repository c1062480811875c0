// Absolute pose of every candidate view against the model in one call: the P3P RANSAC pass and the
// refinement of its winner for each view, over the views' concatenated 2D-3D items ("ragged": view v owns items
// offset[v] .. offset[v+1]-1, any count per view).  View v's outputs are what sfm_pnp_ransac_pass(SFM_PNP_SOLVER_P3P,
// seed + v * seed_stride, use_philox = 1) with a mask, followed by sfm_pnp_refine on its winner with the winner's sample item 3
// taken out of the seed mask, give on that view alone: the solver (sfm_p3p.h), the scoring loop and the mask
// model (sfm_pnp_pass.h), the selection (sfmsel::block_select) and the refinement (sfm_pnp_lm.h) are the same device routines.
//
// Six launches whatever the number of views, nothing read back:
//   1. register_offsets_kernel   the offset table is non-decreasing within [0, N], or every status is SFM_REGISTER_BAD_OFFSETS;
//                                the later launches read that mark and then treat every view as empty, so nothing is indexed by it
//   2. register_fit_kernel       grid (h / 64, views): one hypothesis per lane, draws the Philox sample, fills S, the P3P fit
//   3. register_score_kernel     grid (h / 256, views): one hypothesis per lane, the view's items staged through LDS in tiles of
//                                512 (24 KiB), the sample items corrected after the tile loop
//   4. register_select_kernel    grid (views): sfmsel::block_select with the view's own min_extra, sample size 4
//   5. register_mask_kernel      the winners' masks, a grid-stride walk over all N items (an item finds its view by bisection);
//                                both masks of an item no view owns are 0
//   6. register_refine_kernel    one 512-thread block per view: gathers the winner's row, refines it, writes the status
// A view with fewer than 4 items gets the filler: rows of S all -1, models of 12 NaNs, flags SFM_FIT_DEGENERATE, cnt 0,
// s1 = s2 = NaN, and so a record without a winner whose n_flagged is h_count.  Every sum runs in a fixed order: no atomics, and
// a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_minimal_fit.h"
#include "sfm_minimal_score.h"
#include "sfm_pnp.h"
#include "sfm_pnp_lm.h"
#include "sfm_pnp_pass.h"
#include "sfm_select.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_fits;
using sfmhost::grid_for;
using sfmhost::grid_stride;
using sfmmin::kScoreBlock;
using sfmpnp::kP3PSample;
using sfmpnp::kPnPFields;
using sfmpnp::PnPCamera;

constexpr int kFitBlock = sfmmin::kMinimalFitBlock;
constexpr int kSelectBlock = 1024;
constexpr int kCheckBlock = 1024;
constexpr int kRefineBlock = sfmpnp::kRefineThreads;

// The items of view v: none when the offset table was refused (the table itself always holds views + 1 entries).
struct ViewItems {
    const double* pts;
    int64_t first, n;
};
SFM_DEVICE ViewItems view_items(const double* __restrict__ pts, const int64_t* __restrict__ offset,
                                const int32_t* __restrict__ status, int64_t v) {
    const bool bad = status[v] == SFM_REGISTER_BAD_OFFSETS;
    const int64_t lo = bad ? 0 : offset[v], hi = bad ? 0 : offset[v + 1];
    return ViewItems{pts + lo * kPnPFields, lo, hi - lo};
}

// One block: 0 <= offset[0] <= offset[1] <= ... <= offset[views] <= n_total, or every status SFM_REGISTER_BAD_OFFSETS.  The
// status of a view of an accepted table is written by register_refine_kernel.
__global__ __launch_bounds__(kCheckBlock) void register_offsets_kernel(const int64_t* __restrict__ offset, int64_t views,
                                                                       int64_t n_total, int32_t* __restrict__ status) {
    bool ok = true;
    for (int64_t k = threadIdx.x; k <= views; k += kCheckBlock) {
        const int64_t v = offset[k];
        ok = ok && v >= 0 && v <= n_total && (k == 0 || offset[k - 1] <= v);
    }
    const int mark = __syncthreads_and(ok ? 1 : 0) ? SFM_REGISTER_OK : SFM_REGISTER_BAD_OFFSETS;
    for (int64_t v = threadIdx.x; v < views; v += kCheckBlock) status[v] = mark;
}

// sfmmin::minimal_fit_kernel<p3p_solver, true> over the view's own items: draws the sample and stores its row of S.
__global__ __launch_bounds__(kFitBlock) void register_fit_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offset,
                                                                 const int32_t* __restrict__ status, PnPCamera cam, uint64_t seed,
                                                                 uint64_t seed_stride, int64_t h_begin, int64_t h_count,
                                                                 int32_t* __restrict__ S, double* __restrict__ model,
                                                                 int32_t* __restrict__ flags) {
    const int64_t h = (int64_t)blockIdx.x * kFitBlock + threadIdx.x;
    if (h >= h_count) return;
    const int64_t v = blockIdx.y;
    const int64_t vh = v * h_count + h;
    const ViewItems p = view_items(pts, offset, status, v);
    if (p.n < kP3PSample) {   // the filler of a view too small for a sample
#pragma unroll
        for (int i = 0; i < 12; ++i) model[vh * 12 + i] = NAN;
        flags[vh] = SFM_FIT_DEGENERATE;
#pragma unroll
        for (int i = 0; i < 8; ++i) S[vh * 8 + i] = -1;
        return;
    }
    int32_t idx[8];
    sfm::philox_sample8(seed + (uint64_t)v * seed_stride, (uint64_t)(h_begin + h), (uint32_t)p.n, idx);
#pragma unroll
    for (int i = kP3PSample; i < 8; ++i) idx[i] = i < p.n ? idx[i] : -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) S[vh * 8 + i] = idx[i];
    double out[12];
    const int flag = sfmpnp::p3p_solver::fit(sfmpnp::PoseData{p.pts, cam}, 0, p.n, idx, out);
#pragma unroll
    for (int i = 0; i < 12; ++i) model[vh * 12 + i] = out[i];
    flags[vh] = flag;
}

// One hypothesis per lane over its view's items: sfmpnp::score_pose_hypothesis with the lane's model and row of S.
__global__ __launch_bounds__(kScoreBlock) void register_score_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offset,
                                                                     const int32_t* __restrict__ status, PnPCamera cam,
                                                                     const double* __restrict__ model, const int32_t* __restrict__ S,
                                                                     int64_t h_count, double thr, int32_t* __restrict__ cnt,
                                                                     double* __restrict__ s1, double* __restrict__ s2) {
    __shared__ sfmpnp::TilePoint tile[sfmmin::kScoreTile];
    const int64_t v = blockIdx.y;
    const int64_t h = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    const ViewItems p = view_items(pts, offset, status, v);   // uniform over the block, like everything tested before a barrier
    if (p.n < kP3PSample) {
        if (h < h_count) {
            cnt[v * h_count + h] = 0;
            s1[v * h_count + h] = NAN;
            s2[v * h_count + h] = NAN;
        }
        return;
    }
    const int64_t hc = h < h_count ? h : h_count - 1;   // lanes past the end score a valid hypothesis and store nothing
    const int64_t vh = v * h_count + hc;
    const sfmmin::HypothesisScore r = sfmpnp::score_pose_hypothesis<kP3PSample>(tile, p.pts, p.n, model + vh * 12, S + vh * 8, cam, thr);
    if (h < h_count) {
        cnt[v * h_count + h] = r.c;
        s1[v * h_count + h] = r.a1;
        s2[v * h_count + h] = r.a2;
    }
}

// The per-view form of the selection: block v runs the one definition of sfm_select.h over view v's h_count rows with
// min_extra[v].
__global__ __launch_bounds__(kSelectBlock) void register_select_kernel(const int32_t* __restrict__ cnt, const double* __restrict__ s1,
                                                                       const double* __restrict__ s2, const int32_t* __restrict__ flags,
                                                                       int64_t h_count, const double* __restrict__ min_extra,
                                                                       int aggregation, sfm_select_result* __restrict__ result) {
    __shared__ sfmsel::SelectScratch<kSelectBlock> scratch;
    __shared__ int64_t winner;
    const int64_t v = blockIdx.x, first = v * h_count;
    sfmsel::block_select<kSelectBlock>(cnt + first, s1 + first, s2 + first, flags + first, h_count, 0, min_extra[v], aggregation,
                                       result + v, scratch, &winner, kP3PSample);
}

// The winner's mask of every item: 2 for the sample items of the view's winner, 1 for its other items within the threshold, 0
// otherwise, and 0 for an item no view owns or whose view has no winner.  mask_out of an item no view owns is 0 as well (the
// others are written by their view's block of register_refine_kernel).
__global__ void register_mask_kernel(const double* __restrict__ pts, int64_t n_total, const int64_t* __restrict__ offset, int64_t views,
                                     const int32_t* __restrict__ status, PnPCamera cam, const int32_t* __restrict__ S,
                                     const double* __restrict__ model, int64_t h_count, const sfm_select_result* __restrict__ result,
                                     double thr, uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_out) {
    const bool bad = status[0] == SFM_REGISTER_BAD_OFFSETS;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += stride) {
        const int64_t v = bad ? -1 : pair_of_item(offset, views, i);
        uint8_t m = 0;
        if (v >= 0) {
            const int64_t best = result[v].best_h;
            if (best >= 0 && best < h_count) {
                const int64_t vh = v * h_count + best;
                sfmpnp::pnp_model::Item q;
                sfmpnp::pnp_model::load(pts, i, q);
                m = sfmmin::mask_value<kP3PSample>(sfmpnp::pnp_model(model + vh * 12, cam), S + vh * 8, q, i - offset[v], thr);
            }
        } else {
            mask_out[i] = 0;
        }
        mask[i] = m;
    }
}

// One block per view: the winner's row gathered from the tables, sfmpnp::refine_view from it with the winner's sample item 3
// out of the seed mask, and the status.  A view without a winner gets the filler: 12 NaNs, its mask_out bytes 0, info
// {+inf, 0, 0, 0}.
__global__ __launch_bounds__(kRefineBlock) void register_refine_kernel(
    const double* __restrict__ pts, const int64_t* __restrict__ offset, PnPCamera cam, const int32_t* __restrict__ S,
    const double* __restrict__ model, int64_t h_count, const sfm_select_result* __restrict__ result, const uint8_t* __restrict__ mask,
    double thr, int aggregation, int rounds, int max_steps, double* __restrict__ pose_out, uint8_t* __restrict__ mask_out,
    sfm_pnp_refine_info* __restrict__ info, int32_t* __restrict__ status) {
    const int64_t v = blockIdx.x;
    const bool bad = status[v] == SFM_REGISTER_BAD_OFFSETS;   // read by every thread before thread 0 replaces it below
    const ViewItems p = view_items(pts, offset, status, v);
    const int64_t best = result[v].best_h;
    const bool found = !bad && p.n >= kP3PSample && best >= 0 && best < h_count;   // block-uniform
    __syncthreads();
    if (!found) {
        for (int64_t i = threadIdx.x; i < p.n; i += kRefineBlock) mask_out[p.first + i] = 0;
        if (threadIdx.x < 12) pose_out[v * 12 + threadIdx.x] = NAN;
        if (threadIdx.x == 0) {
            info[v].error = INFINITY;
            info[v].count = 0;
            info[v].accepted = 0;
            info[v].lm_steps = 0;
            info[v].reserved = 0;
            status[v] = bad ? SFM_REGISTER_BAD_OFFSETS : (p.n < kP3PSample ? SFM_REGISTER_TOO_FEW : SFM_REGISTER_NO_MODEL);
        }
        return;
    }
    const int64_t vh = v * h_count + best;
    sfmpnp::refine_view(p.pts, (int)p.n, mask + p.first, S[vh * 8 + 3], cam, model + vh * 12, result[v].best_err, thr, aggregation,
                        rounds, max_steps, pose_out + v * 12, mask_out + p.first, info + v);
    if (threadIdx.x == 0) status[v] = SFM_REGISTER_OK;
}

}  // namespace

extern "C" {

int sfm_register_views(uint64_t seed, uint64_t seed_stride, int64_t h_begin, const double* pts, int64_t n_total, const int64_t* offset,
                       int64_t views, const double* min_extra, const double* K, int64_t h_count, double thr, int aggregation,
                       int refine_rounds, int refine_max_steps, int32_t* S, double* model, int32_t* flags, int32_t* cnt, double* s1,
                       double* s2, sfm_select_result* result, uint8_t* mask, double* pose_out, uint8_t* mask_out,
                       sfm_pnp_refine_info* info, int32_t* status, void* stream) {
    const char* fn = "sfm_register_views";
    if (n_total < 0 || views < 0 || refine_rounds < 0 || refine_max_steps < 0) return fail_in(fn, "negative size");
    if (n_total > 0x7FFFFFFF) return fail_in(fn, "need fewer than 2^31 items");
    if (views > 65535) return fail_in(fn, "views > 65535");
    if (h_count < 1) return fail_in(fn, "need at least one hypothesis per view");
    if (h_count > 0x3FFFFFFF || !grid_fits(h_count, kFitBlock, kFitBlock, views) || !grid_fits(h_count, kScoreBlock, kScoreBlock, views))
        return fail_in(fn, "size exceeds what one launch covers (2^31-1 blocks, 2^32-1 threads in x; 65535 in y)");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail_in(fn, "unknown aggregation");
    if (h_begin < 0) return fail_in(fn, "negative h_begin");
    PnPCamera cam;
    const int rc = sfmpnp::camera_from(K, cam, fn);
    if (rc != SFM_OK) return rc;
    if (views == 0) return SFM_OK;
    if (!offset || !min_extra || !S || !model || !flags || !cnt || !s1 || !s2 || !result || !pose_out || !info || !status ||
        (n_total > 0 && (!pts || !mask || !mask_out)))
        return fail_in(fn, "null pointer");
    if (mask != nullptr && mask == mask_out) return fail_in(fn, "mask_out must not alias mask");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(register_offsets_kernel, dim3(1), dim3(kCheckBlock), 0, st, offset, views, n_total, status);
    hipLaunchKernelGGL(register_fit_kernel, dim3(grid_for(h_count, kFitBlock), (unsigned)views), dim3(kFitBlock), 0, st, pts, offset, status,
                       cam, seed, seed_stride, h_begin, h_count, S, model, flags);
    hipLaunchKernelGGL(register_score_kernel, dim3(grid_for(h_count, kScoreBlock), (unsigned)views), dim3(kScoreBlock), 0, st, pts, offset,
                       status, cam, model, S, h_count, thr, cnt, s1, s2);
    hipLaunchKernelGGL(register_select_kernel, dim3((unsigned)views), dim3(kSelectBlock), 0, st, cnt, s1, s2, flags, h_count, min_extra,
                       aggregation, result);
    if (n_total > 0)
        hipLaunchKernelGGL(register_mask_kernel, dim3(grid_stride(n_total, 256, 1024)), dim3(256), 0, st, pts, n_total, offset, views,
                           status, cam, S, model, h_count, result, thr, mask, mask_out);
    hipLaunchKernelGGL(register_refine_kernel, dim3((unsigned)views), dim3(kRefineBlock), 0, st, pts, offset, cam, S, model, h_count, result,
                       mask, thr, aggregation, refine_rounds, refine_max_steps, pose_out, mask_out, info, status);
    return check_launch(fn);
}

}  // extern "C"
