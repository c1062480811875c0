// The logarithm of a rotation matrix (tests/rotation_averaging_oracle.py states the same operations in the
// same order).  For D row-major 3 x 3:
//   v = vee(D - D^T) / 2 = (D21 - D12, D02 - D20, D10 - D01) / 2,  s = |v| = sin(theta)
//   c = ((D00 + D11) + D22 - 1) / 2 clamped to [-1, 1] = cos(theta),  theta = atan2(s, c)
//   c >  kHalfTurnCosine (below 120 degrees):  r = v (theta / s) for s >= kTinySine, r = v below it (theta ~ s)
//   c <= kHalfTurnCosine:  the axis from the symmetric part (D + D^T) / 2 = c I + (1 - c) a a^T, which stays well conditioned up
//                          to the half turn, where v vanishes and carries only its rounding: the column of (D + D^T) / 2 - c I
//                          with the largest diagonal entry (the first of equals), normalised, signed by v = s a (at the half
//                          turn itself both signs are logarithms), times theta
#pragma once
#include <math.h>

#include "sfm_math.h"

namespace sfmso3 {

constexpr double kTinySine = 1e-10;
constexpr double kHalfTurnCosine = -0.5;

SFM_DEVICE void log_map(const double* D, double (&r)[3]) {
    const double v[3] = {0.5 * (D[7] - D[5]), 0.5 * (D[2] - D[6]), 0.5 * (D[3] - D[1])};
    const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double c = fmin(1.0, fmax(-1.0, 0.5 * (((D[0] + D[4]) + D[8]) - 1.0)));
    const double theta = atan2(s, c);
    if (c > kHalfTurnCosine) {
        const double f = s >= kTinySine ? theta / s : 1.0;   // v * 1 is v to the last bit
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = v[k] * f;
        return;
    }
    const double b[3] = {D[0] - c, D[4] - c, D[8] - c};
    int k = 0;
    if (b[1] > b[k]) k = 1;
    if (b[2] > b[k]) k = 2;
    double col[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) col[m] = m == k ? b[k] : 0.5 * (D[3 * m + k] + D[3 * k + m]);
    const double n = sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]);
    const double g = (col[0] * v[0] + col[1] * v[1]) + col[2] * v[2] < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) r[m] = (g * theta) * (col[m] / n);
}

}  // namespace sfmso3
