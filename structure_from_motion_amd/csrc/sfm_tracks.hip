// Triangulation of multi-view tracks: each point from every observation of it, in the observation layout of the bundle
// adjuster (camera_index, point_index, pixels), with an optional per-point Levenberg-Marquardt refinement and the quality
// checks an incremental reconstruction accepts or rejects a point by (the NumPy oracle is
// tests/tracks_oracle.py).  fp64 throughout.
//
// Set-up, once per call: the observations in point-major order (sfm_obs_order.h: a counting sort by point, a
// multi-workgroup scan, each run sorted by observation index).  Main pass, thread p for point p:
//   1. the DLT rows of the reference's triangulate_dlt (y P3 - P2, P1 - x P3 with P = K [R | t]) of each observation,
//      streamed by Givens rotations into a 4 x 4 upper-triangular R (same right singular vectors as the stacked A, the
//      condition number not squared), then R's null vector by sfm::null_vector4 and X = v[0:3] / v[3];
//   2. optionally LM on the point alone (the rules of sfm_lm.h, the Jacobian of sfm_pnp.h), on F(X) = sum of
//      sfm_pnp_score's e over its observations;
//   3. e per observation, cheirality, the triangulation angle and the status.
// A track whose observations all name one camera is DEGENERATE whatever its pixels say: its rays meet at that camera's
// centre, which the DLT would return with a depth of rounding size.
// The DLT rows, the Givens accumulation and the LM are those of sfm_tracks_device.h, shared with sfm_tracks_robust.hip; this
// kernel uses them over all observations of a point.
// null_vector4 decides per wave, so a point's lane is fixed by its index.  No floating-point atomics: a call is
// bit-identical from run to run, and to any call whose observations keep each point's own order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_lm.h"
#include "sfm_math.h"
#include "sfm_obs_order.h"
#include "sfm_pnp.h"
#include "sfm_tracks_device.h"

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmpnp::camera_from;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;
using sfmtracks::AllObservations;
using sfmtracks::Obs;
using sfmtracks::ray;

constexpr int kThreads = 256;

static_assert(sizeof(sfm_tracks_info) == 32, "sfm_tracks_info layout is part of the ABI");

struct Layout {
    size_t off, fill, ord, tile_sum, flag, total;
};

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

Layout layout(int64_t P, int64_t M) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o = align256(o + bytes);
        return (size_t)at;
    };
    L.off = take(4 * (P + 1));
    L.fill = take(4 * P);
    L.ord = take(4 * M);
    L.tile_sum = take(4 * sfmorder::tiles(P));
    L.flag = take(4);
    L.total = (size_t)o;
    return L;
}

struct Out {
    double* points;
    uint8_t* status;
    double* obs_error;   // nullable
    double* angle;       // nullable
    sfm_tracks_info* info;
};

struct Options {
    int min_views, refine_steps;
    double min_angle, max_error;
};

// off[0 .. P], the flag and the info record zeroed
__global__ __launch_bounds__(kThreads) void tracks_init_kernel(int P, sfmorder::PointOrder o,
                                                               sfm_tracks_info* __restrict__ info) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i <= P) o.off[i] = 0;
    if (i == 0) {
        *o.flag = 0;
        *info = sfm_tracks_info{0, 0, 0, 0};
    }
}

// Thread p = point p.  Every lane of a wave reaches null_vector4 (lanes without a problem of their own solve the identity).
__global__ __launch_bounds__(kThreads) void tracks_point_kernel(int P, Obs obs, const double* __restrict__ poses,
                                                                PnPCamera k,
                                                                Options opt, sfmorder::PointOrder o, Out out) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const bool bad_index = *o.flag != 0;
    const bool mine = p < P && !bad_index;
    const int32_t* run = mine ? o.ord + o.off[p] : nullptr;
    const int n = mine ? o.off[p + 1] - o.off[p] : 0;
    const bool few = n < opt.min_views;

    // 1. linear estimate
    double R[4][4] = {};
    bool several = false;   // some observation's camera differs from the first one's
    if (mine && !few) {
        several = sfmtracks::dlt_triangle(run, n, obs, poses, k, AllObservations{}, R);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) R[j][j] = 1.0;
    }
    double v[4];
    sfmtracks::unit_null_vector(R, v);   // every lane of the wave: no lane has returned before this point
    int status = SFM_TRACKS_OK;
    if (bad_index)
        status = SFM_TRACKS_BAD_INDEX;
    else if (few)
        status = SFM_TRACKS_FEW_VIEWS;
    else if (!several || !sfmtracks::usable_null_vector(v))
        status = SFM_TRACKS_DEGENERATE;
    double X[3] = {NAN, NAN, NAN};
    double angle = NAN;
    int steps = 0;
    if (mine && status == SFM_TRACKS_OK) {
        X[0] = v[0] / v[3];
        X[1] = v[1] / v[3];
        X[2] = v[2] / v[3];
        // 2. refinement
        if (opt.refine_steps > 0) steps = sfmtracks::refine_point(X, run, n, obs, poses, k, AllObservations{}, opt.refine_steps);
        // 3. quality: e per observation, cheirality, the smallest cosine between two rays (O(n^2) pairs)
        double max_e = 0.0, min_cos = 1.0;
        bool front = true;
        for (int i = 0; i < n; ++i) {
            const int m = run[i];
            const double* pose = poses + 12 * (int64_t)obs.cam[m];
            const double e = pnp_score(pose, k, X[0], X[1], X[2], obs.uv[2 * (int64_t)m], obs.uv[2 * (int64_t)m + 1]);
            const double c2 = ((pose[6] * X[0] + pose[7] * X[1]) + pose[8] * X[2]) + pose[11];
            front = front && c2 > 0.0;
            max_e = fmax(max_e, e);
            if (out.obs_error) out.obs_error[m] = e;
            double di[3];
            ray(pose, X, di);
            for (int j = i + 1; j < n; ++j) {
                double dj[3];
                ray(poses + 12 * (int64_t)obs.cam[run[j]], X, dj);
                min_cos = fmin(min_cos, (di[0] * dj[0] + di[1] * dj[1]) + di[2] * dj[2]);
            }
        }
        angle = acos(fmin(1.0, fmax(-1.0, min_cos)));
        if (!front)
            status = SFM_TRACKS_BEHIND;
        else if (angle < opt.min_angle)
            status = SFM_TRACKS_SMALL_ANGLE;
        else if (max_e > opt.max_error)
            status = SFM_TRACKS_LARGE_ERROR;
    } else if (mine && out.obs_error) {
        for (int i = 0; i < n; ++i) out.obs_error[run[i]] = NAN;
    }
    if (p < P) {
        out.points[3 * (int64_t)p] = X[0];
        out.points[3 * (int64_t)p + 1] = X[1];
        out.points[3 * (int64_t)p + 2] = X[2];
        out.status[p] = (uint8_t)status;
        if (out.angle) out.angle[p] = angle;
    }

    // info: the OK points and the most LM steps, one atomic per wave (every lane is still active here)
    const uint64_t ok = __ballot(p < P && status == SFM_TRACKS_OK);
    int most = steps;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) most = max(most, __shfl_xor(most, d, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (ok) atomicAdd(reinterpret_cast<unsigned long long*>(&out.info->points_ok), (unsigned long long)__popcll(ok));
        if (most > 0)
            atomicMax(reinterpret_cast<unsigned long long*>(&out.info->max_refine_steps_taken), (unsigned long long)most);
    }
}

// an index out of range: every observation's error is NaN and info.status = 1
__global__ __launch_bounds__(kThreads) void tracks_bad_index_kernel(int M, sfmorder::PointOrder o, Out out) {
    if (*o.flag == 0) return;
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    if (out.obs_error) out.obs_error[m] = NAN;
    if (m == 0) out.info->status = 1;
}

}  // namespace

extern "C" {

int64_t sfm_tracks_workspace_bytes(int64_t points, int64_t observations) {
    if (points < 0 || observations < 0 || points > 0x7FFFFFFE || observations > 0x7FFFFFFF) return -1;
    return (int64_t)layout(points, observations).total;
}

int sfm_triangulate_tracks(const double* K, int64_t cameras, int64_t points, int64_t observations, const double* poses,
                           const int32_t* camera_index, const int32_t* point_index, const double* pixels, int min_views,
                           double min_angle, double max_error, int refine_steps, double* points_out, uint8_t* status,
                           double* obs_error, double* angle, sfm_tracks_info* info, void* workspace,
                           int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 0 || points < 0 || observations < 0) return fail(SFM_EINVAL, "sfm_triangulate_tracks: negative size");
    if (cameras > 0x7FFFFFFF || points > 0x7FFFFFFE || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_triangulate_tracks: cameras, points and observations must be below 2^31");
    if (min_views < 2) return fail(SFM_EINVAL, "sfm_triangulate_tracks: min_views must be at least 2");
    if (!(min_angle >= 0.0) || isinf(min_angle))
        return fail(SFM_EINVAL, "sfm_triangulate_tracks: min_angle must be finite and >= 0");
    if (!(max_error >= 0.0)) return fail(SFM_EINVAL, "sfm_triangulate_tracks: max_error must be >= 0 (+inf allowed)");
    if (refine_steps < 0) return fail(SFM_EINVAL, "sfm_triangulate_tracks: refine_steps must be >= 0");
    PnPCamera cam;
    const int rc = camera_from(K, cam, "sfm_triangulate_tracks");
    if (rc != SFM_OK) return rc;
    if (!info || !workspace || (cameras > 0 && !poses) || (points > 0 && (!points_out || !status)) ||
        (observations > 0 && (!camera_index || !point_index || !pixels)))
        return fail(SFM_EINVAL, "sfm_triangulate_tracks: null pointer");
    const int64_t C = cameras, P = points, M = observations;
    const Layout L = layout(P, M);
    if (workspace_bytes < (int64_t)L.total) return fail(SFM_EINVAL, "sfm_triangulate_tracks: workspace too small");
    if (((uintptr_t)workspace & 15) != 0) return fail(SFM_EINVAL, "sfm_triangulate_tracks: workspace must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    char* b = static_cast<char*>(workspace);
    const sfmorder::PointOrder o{reinterpret_cast<int32_t*>(b + L.off), reinterpret_cast<int32_t*>(b + L.fill),
                                 reinterpret_cast<int32_t*>(b + L.ord), reinterpret_cast<int32_t*>(b + L.tile_sum),
                                 reinterpret_cast<int32_t*>(b + L.flag)};
    const Obs obs{camera_index, pixels};
    const Out out{points_out, status, obs_error, angle, info};
    const Options opt{min_views, refine_steps, min_angle, max_error};

    hipLaunchKernelGGL(tracks_init_kernel, dim3(sfmhost::grid_for(P + 1, kThreads)), dim3(kThreads), 0, st, (int)P, o, info);
    sfmorder::launch_point_order(camera_index, point_index, M, C, P, o, st);
    if (P > 0)
        hipLaunchKernelGGL(tracks_point_kernel, dim3(sfmhost::grid_for(P, kThreads)), dim3(kThreads), 0, st, (int)P, obs, poses,
                           cam, opt, o, out);
    if (M > 0)
        hipLaunchKernelGGL(tracks_bad_index_kernel, dim3(sfmhost::grid_for(M, kThreads)), dim3(kThreads), 0, st, (int)M, o, out);
    return check_launch("sfm_triangulate_tracks");
}

}  // extern "C"
