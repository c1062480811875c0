// Essential-matrix decomposition (eight_point.py:245-280): E = U S V^T, t = vee(U Z U^T) = u3, R1 = U W^T V^T, R2 = U W V^T
// with U, V made proper rotations.  One matrix per lane; the body of decompose_essential_kernel (sfm_kernels.hip), moved here
// unchanged so that the ragged pose kernel of a view graph (sfm_view_graph_pose.hip) decomposes with the same instructions.
#pragma once
#include "sfm_common.h"
#include "sfm_fit.h"
#include "sfm_math.h"

namespace sfmdec {

constexpr double kSigma3Noise = 1e-12;   // sigma_3 <= kSigma3Noise sigma_1: a rank-2 matrix in double precision

// e: 9 doubles, row-major.  An `active` lane writes out[48] = the four candidates (R1,t), (R1,-t), (R2,t), (R2,-t), each R (9,
// row-major) | t (3), and *status = 0, or 1 when sigma_3 is not ~0.  Every lane of the wave must call it (the Jacobi sweeps end
// on a wave vote); an inactive lane passes any valid matrix and stores nothing.
SFM_DEVICE void decompose_essential(const double* __restrict__ e, bool active, double* __restrict__ out,
                                    int32_t* __restrict__ status) {
    // E can have any magnitude (the reference's SVD does not care): scaled exactly into the unit range for the Jacobi
    // sweeps, singular values scaled back for the absolute part of the sigma_3 ~ 0 test (pow2_unit_scale)
    const double scale = sfmfit::pow2_unit_scale(e);
    double g[3][3], v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) g[c][r] = e[r * 3 + c] * scale;
    sfm::hestenes_svd<3>(g, v);
    double sig[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sig[c] = sqrt(g[c][0] * g[c][0] + g[c][1] * g[c][1] + g[c][2] * g[c][2]);  // of the scaled E
    // order columns by decreasing singular value: (i0, i1, i2)
    int i0 = 0, i1 = 1, i2 = 2;
    if (sig[i0] < sig[i1]) { int t = i0; i0 = i1; i1 = t; }
    if (sig[i1] < sig[i2]) { int t = i1; i1 = i2; i2 = t; }
    if (sig[i0] < sig[i1]) { int t = i0; i0 = i1; i1 = t; }
    double u[3][3], vt[3][3];  // u[col][row], vt[col][row] = V columns
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double g0 = 0, g1 = 0, v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g0 = (c == i0) ? g[c][r] : g0;
            g1 = (c == i1) ? g[c][r] : g1;
            v0 = (c == i0) ? v[c][r] : v0;
            v1 = (c == i1) ? v[c][r] : v1;
            v2 = (c == i2) ? v[c][r] : v2;
        }
        u[0][r] = g0;
        u[1][r] = g1;
        vt[0][r] = v0;
        vt[1][r] = v1;
        vt[2][r] = v2;
    }
    double s0 = 0, s1v = 0, s2v = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s0 = (c == i0) ? sig[c] : s0;
        s1v = (c == i1) ? sig[c] : s1v;
        s2v = (c == i2) ? sig[c] : s2v;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u[0][r] /= s0;
        u[1][r] /= s1v;
    }
    // third left singular vector from the cross product: U is a proper rotation by construction,
    // which is what the det(U) == -1 -> U *= -1 branch (eight_point.py:263-264) establishes.
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    // make V proper as well: flip v3 if det(V) < 0 (the reference flips all of V^T; R1/R2 below are
    // then the same pair of rotations)
    const double cx = vt[0][1] * vt[1][2] - vt[0][2] * vt[1][1];
    const double cy = vt[0][2] * vt[1][0] - vt[0][0] * vt[1][2];
    const double cz = vt[0][0] * vt[1][1] - vt[0][1] * vt[1][0];
    const double detv = cx * vt[2][0] + cy * vt[2][1] + cz * vt[2][2];
    if (detv < 0.0) {
        vt[2][0] = -vt[2][0];
        vt[2][1] = -vt[2][1];
        vt[2][2] = -vt[2][2];
    }
    // np.isclose(0, s[-1]) with atol 1e-8 (eight_point.py:268), or sigma_3 at the rounding level of sigma_1: the fit's
    // E / E[2][2] of a motion with E[2][2] = 0 has a magnitude of 1e12 .. 1e19, and the absolute test alone refuses the
    // rounding noise of such a matrix
    const double s2_true = s2v / scale;   // exact: scale is a power of two
    const int st = (s2_true <= 1e-8 + 1e-5 * s2_true || s2v <= kSigma3Noise * s0) ? 0 : 1;
    // R1 = U W^T V^T, R2 = U W V^T with W = [[0,-1,0],[1,0,0],[0,0,1]]:
    //   U W^T = [-u2, u1, u3] columns -> R1 = -u2 v1^T + u1 v2^T + u3 v3^T
    //   U W   = [ u2,-u1, u3]         -> R2 =  u2 v1^T - u1 v2^T + u3 v3^T
    if (active) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double r1 = (-(u[1][r] * vt[0][c]) + u[0][r] * vt[1][c]) + u[2][r] * vt[2][c];
                const double r2 = (u[1][r] * vt[0][c] - u[0][r] * vt[1][c]) + u[2][r] * vt[2][c];
                out[0 * 12 + r * 3 + c] = r1;
                out[1 * 12 + r * 3 + c] = r1;
                out[2 * 12 + r * 3 + c] = r2;
                out[3 * 12 + r * 3 + c] = r2;
            }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            // t = vee(U Z U^T) = u1 x u2 = u3
            out[0 * 12 + 9 + r] = u[2][r];
            out[1 * 12 + 9 + r] = -u[2][r];
            out[2 * 12 + 9 + r] = u[2][r];
            out[3 * 12 + 9 + r] = -u[2][r];
        }
        *status = st;
    }
}

}  // namespace sfmdec
