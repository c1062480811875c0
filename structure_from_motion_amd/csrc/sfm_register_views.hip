// Absolute pose of every candidate view against the model in one call: the P3P RANSAC pass and the
// refinement of its winner for each view, over the views' concatenated 2D-3D items ("ragged": view v owns items
// offset[v] .. offset[v+1]-1, any count per view).  View v's outputs are what sfm_pnp_ransac_pass(SFM_PNP_SOLVER_P3P,
// seed + v * seed_stride, use_philox = 1) with a mask, followed by sfm_pnp_refine on its winner with the winner's sample item 3
// taken out of the seed mask, give on that view alone: the solver (sfm_p3p.h), the scoring loop and the mask
// model (sfm_pnp_pass.h), the selection (sfmsel::block_select) and the refinement (sfm_pnp_lm.h) are the same device routines.
//
// Six launches whatever the number of views, nothing read back; the first five are the ragged pass of sfm_ragged_pass.h:
//   1. sfmrag::ragged_offsets_kernel               the offset table is non-decreasing within [0, N], or every status is
//                                                  SFM_REGISTER_BAD_OFFSETS; the later launches read that mark and then treat
//                                                  every view as empty, so nothing is indexed by it
//   2. sfmrag::ragged_fit_kernel<p3p_solver, true> grid (h / 64, views): one hypothesis per lane, draws the Philox sample, fills
//                                                  S, the P3P fit
//   3. sfmrag::ragged_score_kernel<pose_scorer>    grid (h / 256, views): one hypothesis per lane, the view's items staged through
//                                                  LDS in tiles of 512 (24 KiB), the sample items corrected after the tile loop
//   4. sfmrag::ragged_select_kernel<4>             grid (views): sfmsel::block_select with the view's own min_extra
//   5. sfmrag::ragged_mask_kernel<4, pnp_model>    the winners' masks, a grid-stride walk over all N items (an item finds its
//                                                  view by bisection); both masks of an item no view owns are 0
//   6. register_refine_kernel                      one 512-thread block per view: gathers the winner's row, refines it, writes
//                                                  the status
// A view with fewer than 4 items gets the filler: rows of S all -1, models of 12 NaNs, flags SFM_FIT_DEGENERATE, cnt 0,
// s1 = s2 = NaN, and so a record without a winner whose n_flagged is h_count.  Every sum runs in a fixed order: no atomics, and
// a call is reproducible bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"
#include "sfm_pnp.h"
#include "sfm_pnp_lm.h"
#include "sfm_pnp_pass.h"
#include "sfm_ragged_pass.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail_in;
using sfmhost::grid_for;
using sfmhost::grid_stride;
using sfmpnp::kP3PSample;
using sfmpnp::kPnPFields;
using sfmpnp::PnPCamera;
using sfmrag::Mark;

constexpr int kRefineBlock = sfmpnp::kRefineThreads;

// The scorer of sfmrag::ragged_score_kernel: sfmpnp::score_pose_hypothesis with the lane's model, its row of S and the camera.
struct pose_scorer {
    static constexpr int kSample = kP3PSample, kModel = 12, kStride = kPnPFields;
    using Stored = double;
    using Tile = sfmpnp::TilePoint;
    SFM_DEVICE static sfmmin::HypothesisScore score(Tile* tile, const double* __restrict__ P, int64_t n, const double* __restrict__ model,
                                                    const int32_t* __restrict__ sample_row, double thr, const PnPCamera& cam) {
        return sfmpnp::score_pose_hypothesis<kP3PSample>(tile, P, n, model, sample_row, cam, thr);
    }
};

// One block per view: the winner's row gathered from the tables, sfmpnp::refine_view from it with the winner's sample item 3
// out of the seed mask, and the status.  A view without a winner gets the filler: 12 NaNs, its mask_out bytes 0, info
// {+inf, 0, 0, 0}.
__global__ __launch_bounds__(kRefineBlock) void register_refine_kernel(
    const double* __restrict__ pts, const int64_t* __restrict__ offset, PnPCamera cam, const int32_t* __restrict__ S,
    const double* __restrict__ model, int64_t h_count, const sfm_select_result* __restrict__ result, const uint8_t* __restrict__ mask,
    double thr, int aggregation, int rounds, int max_steps, double* __restrict__ pose_out, uint8_t* __restrict__ mask_out,
    sfm_pnp_refine_info* __restrict__ info, int32_t* __restrict__ status) {
    const int64_t v = blockIdx.x;
    const Mark mark{status, 1};
    const bool bad = mark.bad(v);   // read by every thread before thread 0 replaces it below
    const sfmrag::Range p = sfmrag::range_of(offset, mark, v);
    const int64_t best = sfmrag::winner_of<kP3PSample>(result, v, p.n, h_count);   // block-uniform
    __syncthreads();
    if (best < 0) {
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
    sfmpnp::refine_view(pts + p.first * kPnPFields, (int)p.n, mask + p.first, S[vh * 8 + 3], cam, model + vh * 12, result[v].best_err, thr,
                        aggregation, rounds, max_steps, pose_out + v * 12, mask_out + p.first, info + v);
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
    // every check before the first launch: a refused call has enqueued nothing
    int rc = sfmrag::check_sizes(fn, n_total, views, h_count, 1, 1, aggregation, h_begin, {refine_rounds, refine_max_steps});
    if (rc != SFM_OK) return rc;
    PnPCamera cam;
    rc = sfmpnp::camera_from(K, cam, fn);
    if (rc != SFM_OK) return rc;
    if (views == 0) return SFM_OK;
    if (!offset || !min_extra || !S || !model || !flags || !cnt || !s1 || !s2 || !result || !pose_out || !info || !status ||
        (n_total > 0 && (!pts || !mask || !mask_out)))
        return fail_in(fn, "null pointer");
    if (mask != nullptr && mask == mask_out) return fail_in(fn, "mask_out must not alias mask");
    hipStream_t st = (hipStream_t)stream;
    const Mark mark{status, 1};
    const sfmrag::CallThreshold gate{thr};
    hipLaunchKernelGGL(sfmrag::ragged_offsets_kernel, dim3(1), dim3(sfmrag::kCheckBlock), 0, st, offset, views, n_total, n_total, mark,
                       SFM_REGISTER_OK);
    hipLaunchKernelGGL((sfmrag::ragged_fit_kernel<sfmpnp::p3p_solver, true>), dim3(grid_for(h_count, sfmrag::kFitBlock), (unsigned)views),
                       dim3(sfmrag::kFitBlock), 0, st, sfmpnp::PoseData{pts, cam}, offset, mark, seed, seed_stride, h_begin, h_count, S, model,
                       flags);
    hipLaunchKernelGGL((sfmrag::ragged_score_kernel<pose_scorer, sfmrag::CallThreshold, PnPCamera>),
                       dim3(grid_for(h_count, sfmrag::kScoreBlock), (unsigned)views), dim3(sfmrag::kScoreBlock), 0, st, pts, offset, mark,
                       (const double*)model, (const int32_t*)S, h_count, gate, cnt, s1, s2, cam);
    hipLaunchKernelGGL(sfmrag::ragged_select_kernel<kP3PSample>, dim3((unsigned)views), dim3(sfmrag::kSelectBlock), 0, st,
                       (const int32_t*)cnt, (const double*)s1, (const double*)s2, (const int32_t*)flags, h_count, min_extra, aggregation,
                       result);
    if (n_total > 0)
        hipLaunchKernelGGL((sfmrag::ragged_mask_kernel<kP3PSample, sfmpnp::pnp_model, sfmrag::CallThreshold, PnPCamera>),
                           dim3(grid_stride(n_total, sfmrag::kMaskBlock, sfmrag::kMaskBlocks)), dim3(sfmrag::kMaskBlock), 0, st, pts, n_total,
                           offset, views, mark, (const int32_t*)S, (const double*)model, h_count, (const sfm_select_result*)result, gate,
                           mask, mask_out, cam);
    hipLaunchKernelGGL(register_refine_kernel, dim3((unsigned)views), dim3(kRefineBlock), 0, st, pts, offset, cam, S, model, h_count, result,
                       mask, thr, aggregation, refine_rounds, refine_max_steps, pose_out, mask_out, info, status);
    return check_launch(fn);
}

}  // extern "C"
