// The PnP camera and squared reprojection error shared by the PnP kernels (sfm_pnp.hip) and the refinement of the
// winner (sfm_pnp_refine.hip): both must compute the same e for the same item bit for bit.
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
};

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

// Rows 0 and 1 of a host camera matrix K [9]; SFM_EINVAL unless row 2 is (0, 0, 1).
inline int camera_from(const double* K, PnPCamera& cam, const char* fn) {
    if (!K) return sfmhost::fail(SFM_EINVAL, "sfm_pnp: null camera matrix");
    if (K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: row 2 of the camera matrix must be (0, 0, 1)", fn);
        return sfmhost::fail(SFM_EINVAL, msg);
    }
    cam = PnPCamera{K[0], K[1], K[2], K[3], K[4], K[5]};
    return SFM_OK;
}

}  // namespace sfmpnp
