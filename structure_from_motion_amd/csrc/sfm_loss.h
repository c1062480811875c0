// The robust losses of both bundle adjusters (the NumPy oracle is tests/bundle_robust_oracle.py, written in
// the operation order below).  With e the squared reprojection error of an observation in px^2 (sfmpnp::pnp_score), a the
// scale in pixels and a2 = a * a:
//   squared  rho = e                                        w = rho'(e) = 1
//   huber    rho = e if e <= a2, else (2 a) sqrt(e) - a2    w = 1 if e <= a2, else a / sqrt(e)
//   cauchy   rho = a2 log1p(e / a2)                         w = 1 / (1 + e / a2)
// The cost is the sum of rho.  The linearisation is iteratively reweighted least squares in its first-order form: r, Jc and
// Jp of every observation are multiplied by sqrt(w) at the linearisation point, everything after sees w J^T J and w J^T r.
// Both rho are concave in e, so rho(e) <= rho(e0) + w(e0) (e - e0): the weighted squared cost majorises the robust one and
// touches it at the linearisation point.  rho(+inf) = +inf and w(+inf) = 0 for both.
//
// The scale contract: a2 is computed in double, so a scale whose square is zero, subnormal or infinite is refused like a
// non-positive one (scale_ok; about 1.5e-154 <= a <= 1.3e154).  With a2 = 0 or inf Cauchy's rho is 0 * log1p(e / 0) or
// inf * log1p(0), NaN for every e, and every start would be BAD_START.  Within the contract rho is still +inf where e / a2
// overflows: a bad start, like a point behind a camera.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

namespace sfmloss {

// A loss scale every door accepts: positive, with a normal finite square (false for NaN: the first comparison fails).
inline bool scale_ok(double a) { return a > 0.0 && a * a >= DBL_MIN && a * a <= DBL_MAX; }

}  // namespace sfmloss

#ifdef __HIPCC__   // the rest is for the library's translation units; the host-only torch ops take scale_ok alone
#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmloss {

struct Loss {
    int32_t kind;   // SFM_BUNDLE_LOSS_*
    int32_t pad;
    double a, a2;   // the scale in pixels and its square
};

// NULL options: the squared loss.  False for a loss code outside 0..2, reserved != 0, or a scale that is not scale_ok.
inline bool from_options(const sfm_bundle_options* o, Loss& l) {
    l = Loss{SFM_BUNDLE_LOSS_SQUARED, 0, 1.0, 1.0};
    if (!o) return true;
    if (o->loss < SFM_BUNDLE_LOSS_SQUARED || o->loss > SFM_BUNDLE_LOSS_CAUCHY || o->reserved != 0) return false;
    if (!scale_ok(o->loss_scale)) return false;
    l = Loss{o->loss, 0, o->loss_scale, o->loss_scale * o->loss_scale};
    return true;
}

SFM_DEVICE double rho(const Loss& l, double e) {
    if (l.kind == SFM_BUNDLE_LOSS_HUBER) return e <= l.a2 ? e : (2.0 * l.a) * sqrt(e) - l.a2;
    if (l.kind == SFM_BUNDLE_LOSS_CAUCHY) return l.a2 * log1p(e / l.a2);
    return e;
}

SFM_DEVICE double weight(const Loss& l, double e) {
    if (l.kind == SFM_BUNDLE_LOSS_HUBER) return e <= l.a2 ? 1.0 : l.a / sqrt(e);
    if (l.kind == SFM_BUNDLE_LOSS_CAUCHY) return 1.0 / (1.0 + e / l.a2);
    return 1.0;
}

// sqrt(w) from the residual of sfmpnp::jacobians: e = r0 r0 + r1 r1 has the bits of pnp_score (both compute p / c2 - u).
SFM_DEVICE double sqrt_weight(const Loss& l, const double (&r)[2]) { return sqrt(weight(l, r[0] * r[0] + r[1] * r[1])); }

// Jc and Jp (and r) times s = sqrt(w)
SFM_DEVICE void scale(double s, double (&Jc)[2][6], double (&Jp)[2][3]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int i = 0; i < 6; ++i) Jc[q][i] *= s;
#pragma unroll
        for (int j = 0; j < 3; ++j) Jp[q][j] *= s;
    }
}

SFM_DEVICE void scale(double s, double (&r)[2], double (&Jc)[2][6], double (&Jp)[2][3]) {
    r[0] *= s;
    r[1] *= s;
    scale(s, Jc, Jp);
}

}  // namespace sfmloss
#endif  // __HIPCC__
