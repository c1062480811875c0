// Device definitions that the dense stage's translation units share: the pinhole camera, the bilinear cell
// formula and the winner over the depth hypotheses.  Every function is fp64 + - * / in a written order (the build has
// -ffp-contract=off) and is stated once more in NumPy by tests/plane_sweep_oracle.py; reordering an addition here changes bytes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sfm_math.h"   // SFM_DEVICE

namespace sfmdense {

// every 3-term product sum of the dense stage
SFM_DEVICE double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

struct Mat3 {
    double m[3][3];
};

SFM_DEVICE Mat3 mul3(const Mat3& A, const Mat3& B) {
    Mat3 C;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C.m[i][j] = dot3(A.m[i][0], B.m[0][j], A.m[i][1], B.m[1][j], A.m[i][2], B.m[2][j]);
    return C;
}

// K from its five entries, and its inverse in closed form
SFM_DEVICE void camera_matrices(const double* __restrict__ K, Mat3& Km, Mat3& Ki) {
    const double fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
    Km = Mat3{{{fx, sk, cx}, {0.0, fy, cy}, {0.0, 0.0, 1.0}}};
    const double ff = fx * fy;
    Ki = Mat3{{{1.0 / fx, -sk / ff, (sk * cy - cx * fy) / ff}, {0.0, 1.0 / fy, -cy / fy}, {0.0, 0.0, 1.0}}};
}

// A pixel (x, y) of a view (pose P = R row-major, then t) at depth d in the world: R^T (d K^-1 (x, y, 1) - t).
SFM_DEVICE void back_project(const Mat3& Ki, const double* __restrict__ P, double x, double y, double d, double* Xw) {
    double e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = ((Ki.m[i][0] * x + Ki.m[i][1] * y) + Ki.m[i][2]) * d - P[9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) Xw[i] = dot3(P[i], e[0], P[3 + i], e[1], P[6 + i], e[2]);
}

// A world point in a view: its camera depth z and, for z whatever, the pixel (u, v) = K Y / (K Y)_2 with Y = R X + t.
SFM_DEVICE void project(const Mat3& Km, const double* __restrict__ P, const double* Xw, double& u, double& v, double& z) {
    double Y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Y[i] = dot3(P[3 * i], Xw[0], P[3 * i + 1], Xw[1], P[3 * i + 2], Xw[2]) + P[9 + i];
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = dot3(Km.m[i][0], Y[0], Km.m[i][1], Y[1], Km.m[i][2], Y[2]);
    u = p[0] / p[2];
    v = p[1] / p[2];
    z = Y[2];
}

// The bilinear value of the cell whose top-left texel is *p, rows `stride` texels apart, at the fractions (fx, fy) from that
// texel.  Which cell a position falls into is the caller's rule (the sweep: floor; the track refinement: capped at the edge).
// The stride is 64 bits wide as the callers' row offsets are: a 32-bit one costs plane_sweep_kernel a scalar register.
SFM_DEVICE double bilinear_cell(const uint8_t* p, int64_t stride, double fx, double fy) {
    const double p00 = (double)p[0], p10 = (double)p[1], p01 = (double)p[stride], p11 = (double)p[stride + 1];
    const double top = p00 + fx * (p10 - p00), bot = p01 + fx * (p11 - p01);
    return top + fy * (bot - top);
}

// The running winner over the depth hypotheses of a pixel, offered in index order: the lowest cost that is not a NaN, ties to
// the lower index, with the costs of the hypotheses before and after it.
struct DepthWinner {
    int best = -1;
    double best_cost = NAN, cost_before = NAN, cost_after = NAN, previous = NAN;

    SFM_DEVICE void offer(int d, double cost) {
        if (cost == cost && (best < 0 || cost < best_cost)) {
            best = d;
            best_cost = cost;
            cost_before = previous;
            cost_after = NAN;
        } else if (d == best + 1 && best >= 0) {
            cost_after = cost;
        }
        previous = cost;
    }

    // The winner's depth among z[0 .. D - 1] (NaN without a winner), moved by the parabola through the three costs in inverse
    // depth when the winner is an inner hypothesis, both neighbours have a cost and the parabola opens upwards.
    SFM_DEVICE double depth(const double* z, int D) const {
        double out = NAN;
        if (best >= 0) {
            const double zi = z[best];
            out = zi;
            if (best > 0 && best < D - 1 && cost_before == cost_before && cost_after == cost_after) {
                const double den = (cost_before - best_cost) + (cost_after - best_cost);
                if (den > 0.0) {
                    const double o = 0.5 * (cost_before - cost_after) / den;
                    const double zj = z[o > 0.0 ? best + 1 : best - 1];
                    const double q = 1.0 / zi + fabs(o) * (1.0 / zj - 1.0 / zi);
                    out = 1.0 / q;
                }
            }
        }
        return out;
    }
};

}  // namespace sfmdense
