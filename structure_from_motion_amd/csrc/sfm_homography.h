// The four-point homography solver and the symmetric transfer error as device routines: what the single-pair pass
// (sfm_homography.hip) and the ragged pass over a match graph (sfm_view_graph.hip) share.  DESIGN.md §6p.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmhg {

constexpr int kHomographySample = 4;
// A sample is degenerate when sigma_8 / sigma_1 of its conditioned 8 x 9 DLT system is below this (or not a number): a repeated
// item or three points collinear in both images leave two null vectors, and the ratio is at the rounding level (~1e-16).
constexpr double kHomographyDegenerateFloor = 1e-9;

// --------------------------------------------------------------------------------------------------
// Four-point DLT fit of one hypothesis (the steps of epipolar/homography.py::homography_model_fitter):
//   1. each side conditioned on its own: centroid of the four points subtracted, scaled to mean distance sqrt(2);
//   2. the 8 x 9 system with rows [x, y, 1, 0, 0, 0, -u x, -u y, -u] and [0, 0, 0, x, y, 1, -v x, -v y, -v]; its null vector,
//      the last column of Q of a Householder QR of the transposed system, is H~;
//   3. flag: sigma_8 / sigma_1 of the system (the singular values of the 8 x 8 triangle R) below the floor or not a number
//      — four coincident points give a non-finite scale and end here — or a sample index out of range.  det H is NOT tested:
//      three points collinear in one image only give a singular H, which scores +inf or very large values and cannot win;
//   4. H = T_b^-1 H~ T_a in closed form, scaled to ||H||_F = 1, negated when det H < 0 (points in front of both cameras on
//      one side of the plane have det(R + t n^T / d) > 0).
// The model of a flagged hypothesis is written as it comes out; the selection never takes it.
// --------------------------------------------------------------------------------------------------
struct homography_solver {
    static constexpr int kSample = kHomographySample, kModel = 9;
    static constexpr const char* kName = "minimal_fit_kernel<homography_solver>";
    using Data = const Corr*;
    SFM_DEVICE static Data from(Data corr, int64_t first) { return corr + first; }
    SFM_DEVICE static int fit(Data corr, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[9]);
};

// centroid (cx, cy) and scale s = sqrt(2) / mean distance of four points
SFM_DEVICE void condition4(const double (&x)[4], const double (&y)[4], double& cx, double& cy, double& s) {
    cx = (((x[0] + x[1]) + x[2]) + x[3]) / 4.0;
    cy = (((y[0] + y[1]) + y[2]) + y[3]) / 4.0;
    double dist = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double dx = x[i] - cx, dy = y[i] - cy;
        dist += sqrt(dx * dx + dy * dy);
    }
    s = sqrt(2.0) / (dist / 4.0);
}

SFM_DEVICE int homography_solver::fit(Data corr, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[9]) {
    const Corr* __restrict__ pts = corr + b * n;
    bool bad = false;
    double xa[4], ya[4], xb[4], yb[4];
#pragma unroll
    for (int i = 0; i < kHomographySample; ++i) {
        const Corr p = pts[checked_index(idx[i], n, bad)];
        xa[i] = p.xa;
        ya[i] = p.ya;
        xb[i] = p.xb;
        yb[i] = p.yb;
    }
    double cax, cay, sa, cbx, cby, sb;
    condition4(xa, ya, cax, cay, sa);
    condition4(xb, yb, cbx, cby, sb);

    // the design rows as the columns of the 9 x 8 matrix that qr_null_vector factors
    double col[8][9];
#pragma unroll
    for (int i = 0; i < kHomographySample; ++i) {
        const double x = (xa[i] - cax) * sa, y = (ya[i] - cay) * sa;
        const double u = (xb[i] - cbx) * sb, v = (yb[i] - cby) * sb;
        double* r0 = col[2 * i];
        double* r1 = col[2 * i + 1];
        r0[0] = x;   r0[1] = y;   r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -u * x; r0[7] = -u * y; r0[8] = -u;
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x;   r1[4] = y;   r1[5] = 1.0; r1[6] = -v * x; r1[7] = -v * y; r1[8] = -v;
    }
    double rdiag[8], ht[9];
    sfm::qr_null_vector(col, rdiag, ht);
    // the singular values of the system are those of R (col[c][k], k < c, and rdiag)
    double g[8][8], sq[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) g[c][k] = (k < c) ? col[c][k] : ((k == c) ? rdiag[c] : 0.0);
    sfm::singular_values_sq<8>(g, sq);
    double smallest = sq[0], largest = sq[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        smallest = fmin(smallest, sq[k]);
        largest = fmax(largest, sq[k]);
    }
    // (a system that is not finite is NaN throughout after the first reflection: the ratio is NaN and the comparison fails)
    const bool degenerate = bad || !(sqrt(smallest) / sqrt(largest) >= kHomographyDegenerateFloor);

    // M = H~ T_a with T_a = [[sa, 0, -sa cax], [0, sa, -sa cay], [0, 0, 1]]; H = T_b^-1 M with T_b^-1 = [[1/sb, 0, cbx], [0, 1/sb, cby], [0, 0, 1]]
    double m[9], h[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = sa * ht[3 * r];
        m[3 * r + 1] = sa * ht[3 * r + 1];
        m[3 * r + 2] = ht[3 * r + 2] - sa * (ht[3 * r] * cax + ht[3 * r + 1] * cay);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h[c] = m[c] / sb + cbx * m[6 + c];
        h[3 + c] = m[3 + c] / sb + cby * m[6 + c];
        h[6 + c] = m[6 + c];
    }
    double norm2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) norm2 += h[k] * h[k];
    const double norm = sqrt(norm2);
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] /= norm;
    const double det = (h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6])) + h[2] * (h[3] * h[7] - h[4] * h[6]);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = det < 0.0 ? -h[k] : h[k];
    return degenerate ? SFM_FIT_DEGENERATE : 0;
}

// --------------------------------------------------------------------------------------------------
// Symmetric transfer error of one correspondence under H and G = adj(H) (so G ~ H^-1 up to the factor det H, which the
// divisions cancel).  Operation order is the contract shared with the NumPy definition of tests/homography_oracle.py and the
// host scorer epipolar/homography.py::calculate_transfer_error_score (the build uses -ffp-contract=off):
//   p_k = (H[3k] xa + H[3k+1] ya) + H[3k+2],  q_k = (G[3k] xb + G[3k+1] yb) + G[3k+2]
//   e = ((p0/p2 - xb)^2 + (p1/p2 - yb)^2) + ((q0/q2 - xa)^2 + (q1/q2 - ya)^2)
//   p2 <= 0 or q2 <= 0 (a point mapped through the line at infinity): e = +inf.
// --------------------------------------------------------------------------------------------------
SFM_DEVICE void adjugate(const double (&h)[9], double (&g)[9]) {
    g[0] = h[4] * h[8] - h[5] * h[7];
    g[1] = h[2] * h[7] - h[1] * h[8];
    g[2] = h[1] * h[5] - h[2] * h[4];
    g[3] = h[5] * h[6] - h[3] * h[8];
    g[4] = h[0] * h[8] - h[2] * h[6];
    g[5] = h[2] * h[3] - h[0] * h[5];
    g[6] = h[3] * h[7] - h[4] * h[6];
    g[7] = h[1] * h[6] - h[0] * h[7];
    g[8] = h[0] * h[4] - h[1] * h[3];
}

SFM_DEVICE double transfer_error(const double (&h)[9], const double (&g)[9], double xa, double ya, double xb, double yb) {
    const double p0 = (h[0] * xa + h[1] * ya) + h[2];
    const double p1 = (h[3] * xa + h[4] * ya) + h[5];
    const double p2 = (h[6] * xa + h[7] * ya) + h[8];
    const double q0 = (g[0] * xb + g[1] * yb) + g[2];
    const double q1 = (g[3] * xb + g[4] * yb) + g[5];
    const double q2 = (g[6] * xb + g[7] * yb) + g[8];
    const double du = p0 / p2 - xb, dv = p1 / p2 - yb;
    const double eu = q0 / q2 - xa, ev = q1 / q2 - ya;
    const double e = (du * du + dv * dv) + (eu * eu + ev * ev);
    return (p2 <= 0.0 || q2 <= 0.0) ? INFINITY : e;
}

// The `Model` of sfm_minimal_score.h: H and adj(H) in registers, the symmetric transfer error of a correspondence.
struct homography_model {
    using Stored = Corr;
    using Item = Corr;
    static constexpr int kStride = 1, kModel = 9;
    double m[9], g[9];
    SFM_DEVICE explicit homography_model(const double* model) {
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = model[i];
        adjugate(m, g);
    }
    SFM_DEVICE static void load(const Corr* items, int64_t i, Corr& slot) { slot = items[i]; }
    SFM_DEVICE double error(const Corr& t) const { return transfer_error(m, g, t.xa, t.ya, t.xb, t.yb); }
};

}  // namespace sfmhg
