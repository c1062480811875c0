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

namespace {

using sfmhost::check_launch;
using sfmhost::fail;
using sfmpnp::camera_from;
using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr int kThreads = 256;
constexpr double kMinW = 1e-12;   // |v3| of the unit null vector at or below this: the point is at infinity

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

struct Obs {
    const int32_t* cam;
    const double* uv;
};

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

// unit vector from the centre -R^T t of camera `pose` to X
SFM_DEVICE void ray(const double* pose, const double (&X)[3], double (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = X[k] + ((pose[k] * pose[9] + pose[3 + k] * pose[10]) + pose[6 + k] * pose[11]);
    const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] /= n;
}

// row a (4) rotated into the upper triangle of R by Givens rotations; a is consumed
SFM_DEVICE void givens_add(double (&R)[4][4], double (&a)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (a[j] != 0.0) {
            const double r = hypot(R[j][j], a[j]);
            const double c = R[j][j] / r, s = a[j] / r;
            R[j][j] = r;
#pragma unroll
            for (int k = j + 1; k < 4; ++k) {
                const double rk = R[j][k];
                R[j][k] = c * rk + s * a[k];
                a[k] = c * a[k] - s * rk;
            }
        }
    }
}

// F, H (packed upper 3 x 3) and g = J^T r of the point X over its run.  An observation behind the camera makes F infinite
// and adds nothing to H or g.  J: the point rows of sfmpnp::jacobians, one add per row.
SFM_DEVICE double point_system(const double (&X)[3], const int32_t* run, int n, const Obs& obs,
                               const double* __restrict__ poses, const PnPCamera& k, double (&H)[6], double (&g)[3]) {
    double F = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) H[i] = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    for (int q = 0; q < n; ++q) {
        const int m = run[q];
        const double* pose = poses + 12 * (int64_t)obs.cam[m];
        const double u = obs.uv[2 * (int64_t)m], v = obs.uv[2 * (int64_t)m + 1];
        F += pnp_score(pose, k, X[0], X[1], X[2], u, v);
        double r[2], Jc[2][6], Jp[2][3];
        if (!sfmpnp::jacobians(pose, k, X[0], X[1], X[2], Jc, Jp, r, u, v)) continue;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const double(&J)[3] = Jp[row];
            H[0] += J[0] * J[0];
            H[1] += J[0] * J[1];
            H[2] += J[0] * J[2];
            H[3] += J[1] * J[1];
            H[4] += J[1] * J[2];
            H[5] += J[2] * J[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) g[j] += J[j] * r[row];
        }
    }
    return F;
}

// Cholesky of the packed symmetric 3 x 3 M: false when a pivot is not above rel times its diagonal entry.
// Not sfmlm::factor<3>, and to stay so: the last pivot here, and the triangular solves of refine_point, subtract the
// accumulated sum, M - (a + b), where the shared factor subtracts term by term, (M - a) - b.  This is the order
// tests/tracks_oracle.py defines, and test_parity_with_oracle pins the step counts that follow from it.
SFM_DEVICE bool cholesky3(const double (&M)[6], double rel, double (&L)[6]) {
    // L packed lower: L00, L10, L11, L20, L21, L22
    const double s0 = M[0];
    if (!(s0 > rel * M[0])) return false;
    L[0] = sqrt(s0);
    L[1] = M[1] / L[0];
    L[3] = M[2] / L[0];
    const double s1 = M[3] - L[1] * L[1];
    if (!(s1 > rel * M[3])) return false;
    L[2] = sqrt(s1);
    L[4] = (M[4] - L[3] * L[1]) / L[2];
    const double s2 = M[5] - (L[3] * L[3] + L[4] * L[4]);
    if (!(s2 > rel * M[5])) return false;
    L[5] = sqrt(s2);
    return true;
}

// LM on the point alone (the constants and rules of sfm_lm.h): returns the trial steps taken
SFM_DEVICE int refine_point(double (&X)[3], const int32_t* run, int n, const Obs& obs, const double* __restrict__ poses,
                            const PnPCamera& k, int max_steps) {
    double H[6], g[3], L[6];
    double F = point_system(X, run, n, obs, poses, k, H, g);
    if (!isfinite(F) || !cholesky3(H, sfmlm::kRankFloor, L)) return 0;
    double lambda = sfmlm::kLambda0;
    int steps = 0;
    while (!sfmlm::exhausted(steps, max_steps, lambda)) {
        ++steps;
        const double D[6] = {H[0] + lambda * H[0], H[1], H[2], H[3] + lambda * H[3], H[4], H[5] + lambda * H[5]};
        if (!cholesky3(D, 0.0, L)) {
            lambda = sfmlm::more_damping(lambda);
            continue;
        }
        const double y0 = -g[0] / L[0];
        const double y1 = (-g[1] - L[1] * y0) / L[2];
        const double y2 = (-g[2] - (L[3] * y0 + L[4] * y1)) / L[5];
        const double d2 = y2 / L[5];
        const double d1 = (y1 - L[4] * d2) / L[2];
        const double d0 = (y0 - (L[1] * d1 + L[3] * d2)) / L[0];
        if (!(isfinite(d0) && isfinite(d1) && isfinite(d2))) {
            lambda = sfmlm::more_damping(lambda);
            continue;
        }
        const double dn = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        const double xn = sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]);
        if (sfmlm::small_step(dn, xn)) break;
        const double Xt[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
        double Ht[6], gt[3];
        const double Ft = point_system(Xt, run, n, obs, poses, k, Ht, gt);
        if (sfmlm::improved(Ft, F)) {
            const bool last = sfmlm::converged(F, Ft);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                X[i] = Xt[i];
                g[i] = gt[i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) H[i] = Ht[i];
            F = Ft;
            lambda = sfmlm::less_damping(lambda);
            if (last) break;
        } else {
            lambda = sfmlm::more_damping(lambda);
        }
    }
    return steps;
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
        const int32_t first = obs.cam[run[0]];
        for (int q = 0; q < n; ++q) {
            const int m = run[q];
            several = several || obs.cam[m] != first;
            const double* pose = poses + 12 * (int64_t)obs.cam[m];
            const double x = obs.uv[2 * (int64_t)m], y = obs.uv[2 * (int64_t)m + 1];
            double Pm[3][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double r0 = pose[j < 3 ? j : 9], r1 = pose[j < 3 ? 3 + j : 10], r2 = pose[j < 3 ? 6 + j : 11];
                Pm[0][j] = (k.k00 * r0 + k.k01 * r1) + k.k02 * r2;
                Pm[1][j] = (k.k10 * r0 + k.k11 * r1) + k.k12 * r2;
                Pm[2][j] = r2;
            }
            double a[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = y * Pm[2][j] - Pm[1][j];
                b[j] = Pm[0][j] - x * Pm[2][j];
            }
            givens_add(R, a);
            givens_add(R, b);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) R[j][j] = 1.0;
    }
    double v[4];
    sfm::null_vector4(R, v);   // every lane of the wave: no lane has returned before this point
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] /= vn;
    int status = SFM_TRACKS_OK;
    if (bad_index)
        status = SFM_TRACKS_BAD_INDEX;
    else if (few)
        status = SFM_TRACKS_FEW_VIEWS;
    else if (!several || !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3])) || !(fabs(v[3]) > kMinW))
        status = SFM_TRACKS_DEGENERATE;
    double X[3] = {NAN, NAN, NAN};
    double angle = NAN;
    int steps = 0;
    if (mine && status == SFM_TRACKS_OK) {
        X[0] = v[0] / v[3];
        X[1] = v[1] / v[3];
        X[2] = v[2] / v[3];
        // 2. refinement
        if (opt.refine_steps > 0) steps = refine_point(X, run, n, obs, poses, k, opt.refine_steps);
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
