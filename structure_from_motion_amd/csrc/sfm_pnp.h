// The PnP camera and squared reprojection error shared by the PnP kernels (sfm_pnp.hip) and the refinement of the
// winner (sfm_pnp_refine.hip): both must compute the same e for the same item bit for bit.  Also the pose model's
// Jacobian rows, update and camera centre, shared by the refinement, the bundle adjusters (sfm_bundle_lm.h) and the
// per-point refinement of sfm_tracks.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmpnp {

constexpr int kPnPFields = 5;  // X, Y, Z, u, v

struct PnPCamera {
    double k00, k01, k02, k10, k11, k12;  // rows 0 and 1 of K; row 2 is (0, 0, 1)
    int general;                          // k01 or k10 is not exactly zero (decided on the host: uniform over a launch)
};

// Pixel -> normalised image coordinates, (x, y, 1) = K^-1 (u, v, 1): the 2 x 2 block of K inverted by Cramer's rule, in the
// operation order of sfmp3p::bearing, pnp/pnp.py::normalized_coords and tests/pnp_oracle.py::normalized_coords.  A camera
// with k01 = k10 = 0 keeps the two plain divisions (u - k02) / k00, (v - k12) / k11, so its results keep their bits.
SFM_DEVICE void normalized_coords(const PnPCamera& k, double u, double v, double& x, double& y) {
    const double du = u - k.k02;
    const double dv = v - k.k12;
    if (k.general) {
        const double det = k.k00 * k.k11 - k.k01 * k.k10;
        x = (du * k.k11 - k.k01 * dv) / det;
        y = (k.k00 * dv - k.k10 * du) / det;
    } else {
        x = du / k.k00;
        y = dv / k.k11;
    }
}

// --------------------------------------------------------------------------------------------------
// Squared reprojection error in pixels of one item under one model m = {R (9) | t (3)}.
// Operation order is the contract shared with the NumPy oracle of tests/test_pnp_host.py and the host scorer
// structure_from_motion_amd/pnp/pnp.py::calculate_reprojection_score (the build uses -ffp-contract=off):
//   c_r = ((R_r0 X + R_r1 Y) + R_r2 Z) + t_r                 r = 0, 1, 2
//   p_r = (K_r0 c_0 + K_r1 c_1) + K_r2 c_2                    r = 0, 1   (p_2 = c_2: row 2 of K is (0, 0, 1))
//   e   = (p_0 / c_2 - u)^2 + (p_1 / c_2 - v)^2,  du * du + dv * dv
//   c_2 <= 0 (behind the camera): e = +inf.
// --------------------------------------------------------------------------------------------------
SFM_DEVICE double pnp_score(const double m[12], const PnPCamera& k, double X, double Y, double Z, double u, double v) {
    const double c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[9];
    const double c1 = ((m[3] * X + m[4] * Y) + m[5] * Z) + m[10];
    const double c2 = ((m[6] * X + m[7] * Y) + m[8] * Z) + m[11];
    const double p0 = (k.k00 * c0 + k.k01 * c1) + k.k02 * c2;
    const double p1 = (k.k10 * c0 + k.k11 * c1) + k.k12 * c2;
    const double du = p0 / c2 - u;
    const double dv = p1 / c2 - v;
    const double e = du * du + dv * dv;
    return c2 <= 0.0 ? INFINITY : e;
}

// The Jacobian rows of one observation in front of the camera, in pose coordinates (omega, dt) and point coordinates,
// with the residual r = (w_0 - u, w_1 - v) when r is given.  With c = R X + t, w = K c / c_2:
//   dr/dc = (1 / c_2) [[K00, K01, K02 - w_0], [K10, K11, K12 - w_1]],  dc/domega = -[R X]x,  dc/dt = I,  dc/dX = R,
// so row k of Jc is (R X  x  A_k, A_k) and row k of Jp is A_k R, A_k row k of dr/dc.  False behind the camera (c_2 <= 0).
SFM_DEVICE bool jacobians(const double m[12], const PnPCamera& k, double X, double Y, double Z, double (&Jc)[2][6],
                          double (&Jp)[2][3], double* r = nullptr, double u = 0.0, double v = 0.0) {
    const double r0 = (m[0] * X + m[1] * Y) + m[2] * Z;
    const double r1 = (m[3] * X + m[4] * Y) + m[5] * Z;
    const double r2 = (m[6] * X + m[7] * Y) + m[8] * Z;
    const double c0 = r0 + m[9], c1 = r1 + m[10], c2 = r2 + m[11];
    if (!(c2 > 0.0)) return false;
    const double w0 = ((k.k00 * c0 + k.k01 * c1) + k.k02 * c2) / c2;
    const double w1 = ((k.k10 * c0 + k.k11 * c1) + k.k12 * c2) / c2;
    if (r) {
        r[0] = w0 - u;
        r[1] = w1 - v;
    }
    const double ic = 1.0 / c2;
    const double A[2][3] = {{k.k00 * ic, k.k01 * ic, (k.k02 - w0) * ic}, {k.k10 * ic, k.k11 * ic, (k.k12 - w1) * ic}};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        Jc[q][0] = r1 * A[q][2] - r2 * A[q][1];
        Jc[q][1] = r2 * A[q][0] - r0 * A[q][2];
        Jc[q][2] = r0 * A[q][1] - r1 * A[q][0];
        Jc[q][3] = A[q][0];
        Jc[q][4] = A[q][1];
        Jc[q][5] = A[q][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) Jp[q][j] = (A[q][0] * m[j] + A[q][1] * m[3 + j]) + A[q][2] * m[6 + j];
    }
    return true;
}

// out = {exp([omega]x) R | t + dt} for delta = (omega, dt): Rodrigues, exp(W) = I + A W + B W^2 with A = sin(th) / th and
// B = (1 - cos(th)) / th^2 = 2 sin^2(th / 2) / th^2, their Taylor forms below th = 1e-6.
SFM_DEVICE void apply_step(const double* pose, const double* delta, double* out) {
    const double w0 = delta[0], w1 = delta[1], w2 = delta[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    const double th = sqrt(th2);
    double A, B;
    if (th < 1e-6) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double s = sin(0.5 * th);
        A = sin(th) / th;
        B = 2.0 * s * s / th2;
    }
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double E[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double W2 = (W[r][0] * W[0][c] + W[r][1] * W[1][c]) + W[r][2] * W[2][c];
            E[r][c] = ((r == c ? 1.0 : 0.0) + A * W[r][c]) + B * W2;
        }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (E[r][0] * pose[c] + E[r][1] * pose[3 + c]) + E[r][2] * pose[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[9 + r] = pose[9 + r] + delta[3 + r];
}

// The camera centre -R^T t of a pose.
SFM_DEVICE void centre(const double* pose, double (&c)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = -((pose[k] * pose[9] + pose[3 + k] * pose[10]) + pose[6 + k] * pose[11]);
}

// Rows 0 and 1 of a host camera matrix K [9]; SFM_EINVAL unless row 2 is (0, 0, 1) and the 2 x 2 block of rows 0 and 1
// is invertible (K00 K11 - K01 K10 neither zero nor NaN).
inline int camera_from(const double* K, PnPCamera& cam, const char* fn) {
    if (!K) return sfmhost::fail(SFM_EINVAL, "sfm_pnp: null camera matrix");
    char msg[160];
    if (K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) {
        snprintf(msg, sizeof msg, "%s: row 2 of the camera matrix must be (0, 0, 1)", fn);
        return sfmhost::fail(SFM_EINVAL, msg);
    }
    const double det = K[0] * K[4] - K[1] * K[3];
    if (det == 0.0 || det != det) {   // zero or NaN
        snprintf(msg, sizeof msg, "%s: the camera matrix is singular (K00 K11 - K01 K10 is zero or not a number)", fn);
        return sfmhost::fail(SFM_EINVAL, msg);
    }
    cam = PnPCamera{K[0], K[1], K[2], K[3], K[4], K[5], (K[1] != 0.0 || K[3] != 0.0) ? 1 : 0};
    return SFM_OK;
}

}  // namespace sfmpnp
