// Device code shared by the two triangulators of multi-view tracks, sfm_tracks.hip and
// sfm_tracks_robust.hip: the DLT rows of one observation, the Givens accumulation of a track's rows into a
// 4 x 4 triangle, the ray of a camera, and the per-point Levenberg-Marquardt (its normal equations, its 3 x 3 Cholesky
// and its loop).  fp64 throughout.
//
// Every function that walks a track takes the set of its observations to use, a callable `use(m)` over observation
// indices.  AllObservations is the plain triangulator's: it is constant, so that instantiation compiles to the loops the
// plain kernel had before the set existed, in the same operation order (its tests pin the step counts that follow from
// it).  FlaggedObservations reads a uint8 per observation (the robust triangulator's inlier flags, kept in its output
// array: a mask-indexed per-thread array would end up in LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_lm.h"
#include "sfm_math.h"
#include "sfm_pnp.h"

namespace sfmtracks {

using sfmpnp::pnp_score;
using sfmpnp::PnPCamera;

constexpr double kMinW = 1e-12;   // |v3| of the unit null vector at or below this: the point is at infinity

struct Obs {
    const int32_t* cam;
    const double* uv;
};

struct AllObservations {
    SFM_DEVICE bool operator()(int) const { return true; }
};

struct FlaggedObservations {
    const uint8_t* flag;
    SFM_DEVICE bool operator()(int m) const { return flag[m] != 0; }
};

// unit vector from the centre -R^T t of camera `pose` to X
SFM_DEVICE void ray(const double* pose, const double (&X)[3], double (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = X[k] + ((pose[k] * pose[9] + pose[3 + k] * pose[10]) + pose[6 + k] * pose[11]);
    const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] /= n;
}

// the reference's two DLT rows of pixel (x, y) in camera `pose`: a = y P3 - P2, b = P1 - x P3 with P = K [R | t]
SFM_DEVICE void dlt_rows(const double* pose, const PnPCamera& k, double x, double y, double (&a)[4], double (&b)[4]) {
    double Pm[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double r0 = pose[j < 3 ? j : 9], r1 = pose[j < 3 ? 3 + j : 10], r2 = pose[j < 3 ? 6 + j : 11];
        Pm[0][j] = (k.k00 * r0 + k.k01 * r1) + k.k02 * r2;
        Pm[1][j] = (k.k10 * r0 + k.k11 * r1) + k.k12 * r2;
        Pm[2][j] = r2;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = y * Pm[2][j] - Pm[1][j];
        b[j] = Pm[0][j] - x * Pm[2][j];
    }
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

// The DLT rows of the used observations of a run, streamed into the triangle R (zero on entry) in run order.  Returns
// whether two used observations name different cameras (false for an empty set).
template <class Use>
SFM_DEVICE bool dlt_triangle(const int32_t* run, int n, const Obs& obs, const double* __restrict__ poses, const PnPCamera& k,
                             const Use& use, double (&R)[4][4]) {
    bool several = false, any = false;
    int32_t first = 0;
    for (int q = 0; q < n; ++q) {
        const int m = run[q];
        if (!use(m)) continue;
        const int32_t c = obs.cam[m];
        first = any ? first : c;
        any = true;
        several = several || c != first;
        double a[4], b[4];
        dlt_rows(poses + 12 * (int64_t)c, k, obs.uv[2 * (int64_t)m], obs.uv[2 * (int64_t)m + 1], a, b);
        givens_add(R, a);
        givens_add(R, b);
    }
    return several;
}

// F, H (packed upper 3 x 3) and g = J^T r of the point X over the used observations of its run.  An observation behind
// the camera makes F infinite and adds nothing to H or g.  J: the point rows of sfmpnp::jacobians, one add per row.
template <class Use>
SFM_DEVICE double point_system(const double (&X)[3], const int32_t* run, int n, const Obs& obs,
                               const double* __restrict__ poses, const PnPCamera& k, const Use& use, double (&H)[6],
                               double (&g)[3]) {
    double F = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) H[i] = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    for (int q = 0; q < n; ++q) {
        const int m = run[q];
        if (!use(m)) continue;
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

// LM on the point alone over the used observations of its run (the constants and rules of sfm_lm.h):
// returns the trial steps taken
template <class Use>
SFM_DEVICE int refine_point(double (&X)[3], const int32_t* run, int n, const Obs& obs, const double* __restrict__ poses,
                            const PnPCamera& k, const Use& use, int max_steps) {
    double H[6], g[3], L[6];
    double F = point_system(X, run, n, obs, poses, k, use, H, g);
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
        const double Ft = point_system(Xt, run, n, obs, poses, k, use, Ht, gt);
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

// the unit null vector of R's triangle: every lane of the wave must call this (sfm::null_vector4 decides per wave)
SFM_DEVICE void unit_null_vector(const double (&R)[4][4], double (&v)[4]) {
    sfm::null_vector4(R, v);
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] /= vn;
}

// finite, and not at infinity
SFM_DEVICE bool usable_null_vector(const double (&v)[4]) {
    return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]) && fabs(v[3]) > kMinW;
}

}  // namespace sfmtracks
