// The logarithm of a rotation matrix (tests/rotation_averaging_oracle.py states the same operations in the
// same order).  For D row-major 3 x 3:
//   v = vee(D - D^T) / 2 = (D21 - D12, D02 - D20, D10 - D01) / 2,  s = |v| = sin(theta)
//   c = ((D00 + D11) + D22 - 1) / 2 clamped to [-1, 1] = cos(theta),  theta = atan2(s, c)
//   s >= kTinySine:  r = v (theta / s)
//   s <  kTinySine and c > 0:  r = v (theta ~ s)
//   s <  kTinySine and c <= 0 (theta ~ pi):  r = theta a, a the normalised column of (D + I) / 2 = a a^T (at theta = pi) with
//                                            the largest diagonal entry (the first of equals)
#pragma once
#include <math.h>

#include "sfm_math.h"

namespace sfmso3 {

constexpr double kTinySine = 1e-10;

SFM_DEVICE void log_map(const double* D, double (&r)[3]) {
    const double v[3] = {0.5 * (D[7] - D[5]), 0.5 * (D[2] - D[6]), 0.5 * (D[3] - D[1])};
    const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double c = fmin(1.0, fmax(-1.0, 0.5 * (((D[0] + D[4]) + D[8]) - 1.0)));
    const double theta = atan2(s, c);
    if (s >= kTinySine) {
        const double f = theta / s;
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = v[k] * f;
        return;
    }
    if (c > 0.0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = v[k];
        return;
    }
    const double b[3] = {0.5 * (D[0] + 1.0), 0.5 * (D[4] + 1.0), 0.5 * (D[8] + 1.0)};
    int k = 0;
    if (b[1] > b[k]) k = 1;
    if (b[2] > b[k]) k = 2;
    double col[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) col[m] = m == k ? b[k] : 0.5 * D[3 * m + k];
    const double n = sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]);
#pragma unroll
    for (int m = 0; m < 3; ++m) r[m] = theta * (col[m] / n);
}

}  // namespace sfmso3
