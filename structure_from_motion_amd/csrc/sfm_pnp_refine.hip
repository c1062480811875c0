// Nonlinear refinement of a PnP winner on its inliers: Levenberg-Marquardt on the sum of the PnP scorer's squared
// reprojection errors, then a re-score of every item and the accept rule of sfm_refine_inliers (more inliers, or as
// many and a lower aggregated error: sfmfit::refit_wins).  The PnP counterpart of sfm_refine.hip; off unless asked for.
// The LM constants, the step rules and the 6 x 6 Cholesky solve are those of sfm_lm.h.
//
// One 512-thread block per view runs the whole loop.  The pass over the inliers is latency-bound at one block per view
// (50 000 items x 40 B are L2-resident), so eight waves keep twice the loads of four in flight; the 28-value reduction
// costs the same per wave either way.  Each LM step is one fused pass at the trial pose: its cost C and, in the same
// pass, H = sum J^T J and g = sum J^T r there, so an accepted step already has its next system.  The LM state lives in
// LDS and only thread 0 changes it: the 6 x 6 damped Cholesky solve, the Rodrigues update, accept / reject.  Every
// branch that contains a barrier depends only on LDS values published behind a barrier, so it is block-uniform.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_lm.h"
#include "sfm_math.h"
#include "sfm_pnp.h"
#include "sfm_pnp_lm.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmpnp::camera_from;
using sfmpnp::kPnPFields;
using sfmpnp::PnPCamera;

using sfmpnp::kThreads;

static_assert(sizeof(sfm_pnp_refine_info) == 24, "sfm_pnp_refine_info layout is part of the ABI");

// One block per view: sfmpnp::refine_view (sfm_pnp_lm.h) on the view's rows of the dense tables, no item excluded.
__global__ __launch_bounds__(kThreads) void pnp_refine_kernel(
    const double* __restrict__ pts, int n, PnPCamera cam, const double* __restrict__ model_in,
    const uint8_t* __restrict__ mask_in, const double* __restrict__ err_in, double thr, int aggregation, int rounds,
    int max_steps, double* __restrict__ model_out, uint8_t* __restrict__ mask_out, sfm_pnp_refine_info* __restrict__ info) {
    const int64_t b = blockIdx.x;
    sfmpnp::refine_view(pts + b * n * kPnPFields, n, mask_in + b * n, -1, cam, model_in + b * 12, err_in[b], thr, aggregation, rounds,
                        max_steps, model_out + b * 12, mask_out + b * n, info + b);
}

}  // namespace

extern "C" {

int sfm_pnp_refine(const double* pts, int64_t n, int64_t batch, const double* K, const double* model_in, const uint8_t* mask_in,
                   const double* err_in, double thr, int aggregation, int rounds, int max_steps, double* model_out,
                   uint8_t* mask_out, sfm_pnp_refine_info* info, void* stream) {
    // every check before the launch: a refused call has enqueued nothing
    if (n < 0 || batch < 0 || rounds < 0 || max_steps < 0) return fail(SFM_EINVAL, "sfm_pnp_refine: negative size");
    if (n > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_pnp_refine: n too large");
    if (batch > 0x7FFFFFFF) return fail(SFM_EINVAL, "sfm_pnp_refine: batch exceeds one launch (2^31-1 blocks)");
    if (aggregation < SFM_AGG_SUM || aggregation > SFM_AGG_RMS) return fail(SFM_EINVAL, "sfm_pnp_refine: unknown aggregation");
    PnPCamera cam;
    const int rc = camera_from(K, cam, "sfm_pnp_refine");
    if (rc != SFM_OK) return rc;
    if (batch == 0) return SFM_OK;
    if (!model_in || !err_in || !model_out || !info || (n > 0 && (!pts || !mask_in || !mask_out)))
        return fail(SFM_EINVAL, "sfm_pnp_refine: null pointer");
    if (mask_in != nullptr && mask_in == mask_out) return fail(SFM_EINVAL, "sfm_pnp_refine: mask_out must not alias mask_in");
    hipLaunchKernelGGL(pnp_refine_kernel, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, pts, (int)n, cam,
                       model_in, mask_in, err_in, thr, aggregation, rounds, max_steps, model_out, mask_out, info);
    return check_launch("pnp_refine_kernel");
}

}  // extern "C"
