// Outlier-robust triangulation of multi-view tracks: per-track RANSAC over two-view hypotheses, MSAC scoring over the
// whole track, a refit on the winner's inliers and an inlier flag per observation, in the observation layout of
// sfm_triangulate_tracks (the NumPy definition is tests/robust_tracks_oracle.py).  fp64 throughout.
//
// Set-up, once per call: the point-major order of sfm_obs_order.h, as sfm_tracks.hip.  Main pass, thread p for point p,
// whose observations are o_0 .. o_{k-1} in increasing observation index:
//   1. hypotheses: the pairs i < j of its observations in lexicographic order, all T = k (k - 1) / 2 of them or, beyond
//      max_hypotheses, evenly spaced ranks (integer arithmetic; no random numbers).  A hypothesis is the two-view DLT of
//      its pair (sfm::null_vector4 on the four rows); it is valid when the two cameras differ, the unit null vector is
//      finite and not at infinity, the point is in front of both cameras and their rays open at least min_angle;
//   2. score of a valid hypothesis: n = the observations of the track with e <= max_error (sfm_pnp_score's e), c = the
//      sum of min(e, max_error) in run order.  The winner: largest n, then smallest c, then smallest rank;
//   3. refit: the N-view DLT and the optional LM of sfm_tracks_device.h over the winner's inliers only;
//   4. e of every observation at the final X, the final inlier flags, and the angle over the pairs of final inliers.
// The winner's inlier set lives in the `inlier` output array between 2 and 4: each thread reads back only what it wrote.
// sfm::null_vector4 decides per wave, so every lane reaches every call of it: the hypothesis loop runs to the wave's
// largest count, and a lane without a hypothesis of its own solves the identity.  A point's lane is fixed by its index.
// No floating-point atomics: a call is bit-identical from run to run, and to any call whose observations keep each
// point's own order.
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
using sfmtracks::FlaggedObservations;
using sfmtracks::Obs;
using sfmtracks::ray;

constexpr int kThreads = 256;
constexpr int kMaxHypotheses = 1024;

static_assert(sizeof(sfm_tracks_robust_info) == 48, "sfm_tracks_robust_info layout is part of the ABI");

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
    uint8_t* inlier;
    double* angle;       // nullable
    sfm_tracks_robust_info* info;
};

struct Options {
    int min_views, refine_steps, max_hypotheses;
    double min_angle, max_error;
};

// off[0 .. P], the flag and the info record zeroed
__global__ __launch_bounds__(kThreads) void robust_init_kernel(int P, sfmorder::PointOrder o,
                                                               sfm_tracks_robust_info* __restrict__ info) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i <= P) o.off[i] = 0;
    if (i == 0) {
        *o.flag = 0;
        *info = sfm_tracks_robust_info{0, 0, 0, 0, 0, 0};
    }
}

// first rank of the pairs (i, .) among the pairs i < j of n items in lexicographic order; i <= n - 1 < 2^31
SFM_DEVICE int64_t row_start(int64_t i, int64_t n) { return (int64_t)(((uint64_t)i * (uint64_t)(2 * n - i - 1)) >> 1); }

// the pair (i, j) of rank r, 0 <= r < n (n - 1) / 2: a floating-point guess of the row, corrected by exact integers
SFM_DEVICE void unrank_pair(int64_t r, int n, int& i, int& j) {
    const double b = 2.0 * (double)n - 1.0;
    int64_t row = (int64_t)((b - sqrt(fmax(b * b - 8.0 * (double)r, 0.0))) * 0.5);
    row = row < 0 ? 0 : (row > n - 2 ? n - 2 : row);
    while (row > 0 && row_start(row, n) > r) --row;
    while (row < n - 2 && row_start(row + 1, n) <= r) ++row;
    i = (int)row;
    j = (int)(r - row_start(row, n) + row + 1);
}

SFM_DEVICE double depth(const double* pose, const double (&X)[3]) {
    return ((pose[6] * X[0] + pose[7] * X[1]) + pose[8] * X[2]) + pose[11];
}

SFM_DEVICE double error_of(int m, const double (&X)[3], const Obs& obs, const double* __restrict__ poses, const PnPCamera& k) {
    return pnp_score(poses + 12 * (int64_t)obs.cam[m], k, X[0], X[1], X[2], obs.uv[2 * (int64_t)m], obs.uv[2 * (int64_t)m + 1]);
}

// Thread p = point p.  Every lane of a wave reaches every unit_null_vector (lanes without a problem of their own solve the
// identity).
__global__ __launch_bounds__(kThreads) void robust_point_kernel(int P, Obs obs, const double* __restrict__ poses, PnPCamera k,
                                                                Options opt, sfmorder::PointOrder o, Out out) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const bool bad_index = *o.flag != 0;
    const bool mine = p < P && !bad_index;
    const int32_t* run = mine ? o.ord + o.off[p] : nullptr;
    const int n = mine ? o.off[p + 1] - o.off[p] : 0;

    // 0. early statuses
    bool several = false;
    for (int q = 1; q < n; ++q) several = several || obs.cam[run[q]] != obs.cam[run[0]];
    int status = SFM_TRACKS_OK;
    if (bad_index)
        status = SFM_TRACKS_BAD_INDEX;
    else if (n < opt.min_views)
        status = SFM_TRACKS_FEW_VIEWS;
    else if (!several)
        status = SFM_TRACKS_DEGENERATE;
    bool live = mine && status == SFM_TRACKS_OK;

    // 1. and 2. hypotheses, scored as they come
    const int64_t T = live ? (int64_t)n * (n - 1) / 2 : 0;
    const int H = (int)(T < opt.max_hypotheses ? T : opt.max_hypotheses);
    const int64_t stride = T / opt.max_hypotheses, extra = T % opt.max_hypotheses;   // used when T > max_hypotheses
    int wave_H = H;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) wave_H = max(wave_H, __shfl_xor(wave_H, d, kWave));
    int best_n = -1, scored = 0;
    double best_c = INFINITY;
    double best_X[3] = {NAN, NAN, NAN};
    for (int h = 0; h < wave_H; ++h) {
        double A[4][4] = {};
        int mi = 0, mj = 0;
        bool paired = false;
        if (h < H) {
            const int64_t r = T <= opt.max_hypotheses ? (int64_t)h : h * stride + (h < extra ? (int64_t)h : extra);
            int i, j;
            unrank_pair(r, n, i, j);
            mi = run[i];
            mj = run[j];
            paired = obs.cam[mi] != obs.cam[mj];
        }
        if (paired) {
            sfmtracks::dlt_rows(poses + 12 * (int64_t)obs.cam[mi], k, obs.uv[2 * (int64_t)mi], obs.uv[2 * (int64_t)mi + 1], A[0], A[1]);
            sfmtracks::dlt_rows(poses + 12 * (int64_t)obs.cam[mj], k, obs.uv[2 * (int64_t)mj], obs.uv[2 * (int64_t)mj + 1], A[2], A[3]);
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) A[d][d] = 1.0;
        }
        double v[4];
        sfmtracks::unit_null_vector(A, v);   // every lane of the wave
        if (paired && sfmtracks::usable_null_vector(v)) {
            const double X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
            const double* pose_i = poses + 12 * (int64_t)obs.cam[mi];
            const double* pose_j = poses + 12 * (int64_t)obs.cam[mj];
            bool valid = depth(pose_i, X) > 0.0 && depth(pose_j, X) > 0.0;
            if (valid) {
                double di[3], dj[3];
                ray(pose_i, X, di);
                ray(pose_j, X, dj);
                const double cosine = (di[0] * dj[0] + di[1] * dj[1]) + di[2] * dj[2];
                valid = acos(fmin(1.0, fmax(-1.0, cosine))) >= opt.min_angle;
            }
            if (valid) {
                ++scored;
                int count = 0;
                double cost = 0.0;
                for (int q = 0; q < n; ++q) {
                    const double e = error_of(run[q], X, obs, poses, k);
                    const bool in = e <= opt.max_error;
                    count += in;
                    cost += in ? e : opt.max_error;
                }
                if (count > best_n || (count == best_n && cost < best_c)) {   // strict: the smallest h wins a tie
                    best_n = count;
                    best_c = cost;
                    best_X[0] = X[0];
                    best_X[1] = X[1];
                    best_X[2] = X[2];
                }
            }
        }
    }
    if (live && best_n < opt.min_views) {   // no valid hypothesis leaves best_n = -1
        status = SFM_TRACKS_NO_CONSENSUS;
        live = false;
    }

    // 3. the winner's inliers into the flags, then the refit over them
    double R[4][4] = {};
    bool refit = false;
    if (live) {
        for (int q = 0; q < n; ++q) {
            const int m = run[q];
            out.inlier[m] = error_of(m, best_X, obs, poses, k) <= opt.max_error;
        }
        refit = sfmtracks::dlt_triangle(run, n, obs, poses, k, FlaggedObservations{out.inlier}, R);
        if (!refit) {   // the winner's inliers name one camera
            status = SFM_TRACKS_NO_CONSENSUS;
            live = false;
        }
    }
    if (!refit) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) R[i][j] = i == j ? 1.0 : 0.0;
    }
    double v[4];
    sfmtracks::unit_null_vector(R, v);   // every lane of the wave
    if (live && !sfmtracks::usable_null_vector(v)) {
        status = SFM_TRACKS_DEGENERATE;
        live = false;
    }

    double X[3] = {NAN, NAN, NAN};
    double angle = NAN;
    int steps = 0, inliers = 0;
    if (live) {
        X[0] = v[0] / v[3];
        X[1] = v[1] / v[3];
        X[2] = v[2] / v[3];
        if (opt.refine_steps > 0)
            steps = sfmtracks::refine_point(X, run, n, obs, poses, k, FlaggedObservations{out.inlier}, opt.refine_steps);
        // 4. e of every observation and the final flags (the refit has read the winner's: they may be overwritten now)
        int32_t first = 0;
        bool spread = false;
        for (int q = 0; q < n; ++q) {
            const int m = run[q];
            const double e = error_of(m, X, obs, poses, k);
            const bool in = e <= opt.max_error;
            if (out.obs_error) out.obs_error[m] = e;
            out.inlier[m] = in;
            if (in) {
                const int32_t c = obs.cam[m];
                first = inliers ? first : c;
                spread = spread || c != first;
                ++inliers;
            }
        }
        if (inliers < opt.min_views || !spread) {
            status = SFM_TRACKS_NO_CONSENSUS;
            live = false;
        } else {
            // the smallest cosine between the rays of two final inliers (O(n^2) pairs)
            double min_cos = 1.0;
            for (int i = 0; i < n; ++i) {
                if (!out.inlier[run[i]]) continue;
                double di[3];
                ray(poses + 12 * (int64_t)obs.cam[run[i]], X, di);
                for (int j = i + 1; j < n; ++j) {
                    if (!out.inlier[run[j]]) continue;
                    double dj[3];
                    ray(poses + 12 * (int64_t)obs.cam[run[j]], X, dj);
                    min_cos = fmin(min_cos, (di[0] * dj[0] + di[1] * dj[1]) + di[2] * dj[2]);
                }
            }
            angle = acos(fmin(1.0, fmax(-1.0, min_cos)));
            if (angle < opt.min_angle) status = SFM_TRACKS_SMALL_ANGLE;
        }
    }
    if (mine && !live) {   // no estimate: NaN errors and no flags
        X[0] = X[1] = X[2] = NAN;
        for (int q = 0; q < n; ++q) {
            if (out.obs_error) out.obs_error[run[q]] = NAN;
            out.inlier[run[q]] = 0;
        }
    }
    if (p < P) {
        out.points[3 * (int64_t)p] = X[0];
        out.points[3 * (int64_t)p + 1] = X[1];
        out.points[3 * (int64_t)p + 2] = X[2];
        out.status[p] = (uint8_t)status;
        if (out.angle) out.angle[p] = angle;
    }

    // info: integer sums and a maximum, one atomic each per wave (every lane is still active here)
    const bool ok = p < P && status == SFM_TRACKS_OK;
    const uint64_t oks = __ballot(ok);
    int most = steps;
    long long flags = ok ? inliers : 0, hyps = scored;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        most = max(most, __shfl_xor(most, d, kWave));
        flags += __shfl_xor(flags, d, kWave);
        hyps += __shfl_xor(hyps, d, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        auto word = [](int64_t* at) { return reinterpret_cast<unsigned long long*>(at); };
        if (oks) atomicAdd(word(&out.info->points_ok), (unsigned long long)__popcll(oks));
        if (most > 0) atomicMax(word(&out.info->max_refine_steps_taken), (unsigned long long)most);
        if (flags) atomicAdd(word(&out.info->inlier_observations), (unsigned long long)flags);
        if (hyps) atomicAdd(word(&out.info->hypotheses), (unsigned long long)hyps);
    }
}

// an index out of range: every observation's error is NaN, every flag 0 and info.status = 1
__global__ __launch_bounds__(kThreads) void robust_bad_index_kernel(int M, sfmorder::PointOrder o, Out out) {
    if (*o.flag == 0) return;
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    if (out.obs_error) out.obs_error[m] = NAN;
    out.inlier[m] = 0;
    if (m == 0) out.info->status = 1;
}

}  // namespace

extern "C" {

int64_t sfm_tracks_robust_workspace_bytes(int64_t points, int64_t observations) {
    if (points < 0 || observations < 0 || points > 0x7FFFFFFE || observations > 0x7FFFFFFF) return -1;
    return (int64_t)layout(points, observations).total;
}

int sfm_triangulate_tracks_robust(const double* K, int64_t cameras, int64_t points, int64_t observations, const double* poses,
                                  const int32_t* camera_index, const int32_t* point_index, const double* pixels,
                                  int min_views, double min_angle, double max_error, int refine_steps, int max_hypotheses,
                                  double* points_out, uint8_t* status, double* obs_error, uint8_t* inlier, double* angle,
                                  sfm_tracks_robust_info* info, void* workspace, int64_t workspace_bytes, void* stream) {
    // every check before the first launch: a refused call has enqueued nothing
    if (cameras < 0 || points < 0 || observations < 0) return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: negative size");
    if (cameras > 0x7FFFFFFF || points > 0x7FFFFFFE || observations > 0x7FFFFFFF)
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: cameras, points and observations must be below 2^31");
    if (min_views < 2) return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: min_views must be at least 2");
    if (!(min_angle >= 0.0) || isinf(min_angle))
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: min_angle must be finite and >= 0");
    if (!(max_error >= 0.0) || isinf(max_error))
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: max_error must be finite and >= 0");
    if (refine_steps < 0) return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: refine_steps must be >= 0");
    if (max_hypotheses < 1 || max_hypotheses > kMaxHypotheses)
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: max_hypotheses must be in 1 .. 1024");
    PnPCamera cam;
    const int rc = camera_from(K, cam, "sfm_triangulate_tracks_robust");
    if (rc != SFM_OK) return rc;
    if (!info || !workspace || (cameras > 0 && !poses) || (points > 0 && (!points_out || !status)) ||
        (observations > 0 && (!camera_index || !point_index || !pixels || !inlier)))
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: null pointer");
    const int64_t C = cameras, P = points, M = observations;
    const Layout L = layout(P, M);
    if (workspace_bytes < (int64_t)L.total) return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: workspace too small");
    if (((uintptr_t)workspace & 15) != 0)
        return fail(SFM_EINVAL, "sfm_triangulate_tracks_robust: workspace must be 16-byte aligned");

    hipStream_t st = (hipStream_t)stream;
    char* b = static_cast<char*>(workspace);
    const sfmorder::PointOrder o{reinterpret_cast<int32_t*>(b + L.off), reinterpret_cast<int32_t*>(b + L.fill),
                                 reinterpret_cast<int32_t*>(b + L.ord), reinterpret_cast<int32_t*>(b + L.tile_sum),
                                 reinterpret_cast<int32_t*>(b + L.flag)};
    const Obs obs{camera_index, pixels};
    const Out out{points_out, status, obs_error, inlier, angle, info};
    const Options opt{min_views, refine_steps, max_hypotheses, min_angle, max_error};

    hipLaunchKernelGGL(robust_init_kernel, dim3(sfmhost::grid_for(P + 1, kThreads)), dim3(kThreads), 0, st, (int)P, o, info);
    sfmorder::launch_point_order(camera_index, point_index, M, C, P, o, st);
    if (P > 0)
        hipLaunchKernelGGL(robust_point_kernel, dim3(sfmhost::grid_for(P, kThreads)), dim3(kThreads), 0, st, (int)P, obs, poses,
                           cam, opt, o, out);
    if (M > 0)
        hipLaunchKernelGGL(robust_bad_index_kernel, dim3(sfmhost::grid_for(M, kThreads)), dim3(kThreads), 0, st, (int)M, o, out);
    return check_launch("sfm_triangulate_tracks_robust");
}

}  // extern "C"
