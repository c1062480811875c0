// P3P minimal solver of one hypothesis per lane (fp64): the device form of structure_from_motion_amd/pnp/p3p.py, step for
// step and in the same operation order (the build uses -ffp-contract=off).  See that module and DESIGN.md §6k.
//
// Items 0-2 are solved for: depths lambda_i > 0 with lambda_i^2 + lambda_j^2 - 2 c_ij lambda_i lambda_j = a_ij.  A singular
// member of the pencil of the two homogeneous forms D1, D2 (Lambda Twist's structure) splits into two planes through the
// solution rays; each plane meets the cone of the pencil in two rays.  Each of the up-to-four candidates is scaled, polished
// by three Newton steps, turned into a pose and scored on item 3 as soon as it is made: the lane keeps only the best so far
// (strict <, so the earliest on ties), never an array of candidates.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "sfm_common.h"
#include "sfm_pnp.h"

namespace sfmp3p {

// |(X1 - X0) x (X2 - X0)|^2 <= floor^2 |X1 - X0|^2 |X2 - X0|^2: collinear or coincident solve points (pnp/p3p.py)
constexpr double kCollinearFloor = 1e-9;
constexpr int kNewtonSteps = 3;
constexpr double kResidualTol = 1e-6;

struct V3 {
    double x, y, z;
};
struct Sym3 {
    double a00, a01, a02, a11, a12, a22;
};

SFM_DEVICE double dot3(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
SFM_DEVICE V3 cross3(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
SFM_DEVICE V3 sub3(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// normalise(K^-1 (u, v, 1)), rows 0 and 1 of K by Cramer's rule
SFM_DEVICE V3 bearing(double u, double v, const sfmpnp::PnPCamera& k) {
    const double du = u - k.k02;
    const double dv = v - k.k12;
    const double det = k.k00 * k.k11 - k.k01 * k.k10;
    const double x = (du * k.k11 - k.k01 * dv) / det;
    const double y = (k.k00 * dv - k.k10 * du) / det;
    const double inv = 1.0 / sqrt((x * x + y * y) + 1.0);
    return {x * inv, y * inv, inv};
}

SFM_DEVICE bool collinear(const V3& X0, const V3& X1, const V3& X2) {
    const V3 d01 = sub3(X1, X0), d02 = sub3(X2, X0);
    const V3 c = cross3(d01, d02);
    return !(dot3(c, c) > (kCollinearFloor * kCollinearFloor) * (dot3(d01, d01) * dot3(d02, d02)));
}

// cofactors (00, 11, 22, 01, 02, 12) of a symmetric 3 x 3
struct Cof {
    double c00, c11, c22, c01, c02, c12;
};
SFM_DEVICE Cof cofactors(const Sym3& A) {
    return {A.a11 * A.a22 - A.a12 * A.a12, A.a00 * A.a22 - A.a02 * A.a02, A.a00 * A.a11 - A.a01 * A.a01,
            A.a02 * A.a12 - A.a01 * A.a22, A.a01 * A.a12 - A.a02 * A.a11, A.a01 * A.a02 - A.a00 * A.a12};
}
SFM_DEVICE double trace_adj(const Cof& C, const Sym3& B) {
    return ((C.c00 * B.a00 + C.c11 * B.a11) + C.c22 * B.a22) + 2.0 * ((C.c01 * B.a01 + C.c02 * B.a02) + C.c12 * B.a12);
}

// One real root of x^3 + a x^2 + b x + c: Cardano (one real root) or the largest trigonometric root, then two Newton steps.
SFM_DEVICE double cubic_root(double a, double b, double c) {
    const double a3 = a / 3.0;
    const double p = b - a * a3;
    const double q = (2.0 * a3 * a3 * a3 - a3 * b) + c;
    const double h = 0.25 * q * q + (p * p * p) / 27.0;
    double y;
    if (h > 0.0) {
        const double w = -0.5 * q - copysign(sqrt(h), q);
        const double u = cbrt(w);
        y = u != 0.0 ? u - p / (3.0 * u) : 0.0;
    } else {
        const double r = sqrt(-p / 3.0);
        double cs = r > 0.0 ? -0.5 * q / (r * r * r) : 0.0;
        cs = fmin(1.0, fmax(-1.0, cs));
        y = 2.0 * r * cos(acos(cs) / 3.0);
    }
    double x = y - a3;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double fx = ((x + a) * x + b) * x + c;
        const double dfx = (3.0 * x + 2.0 * a) * x + b;
        x = dfx != 0.0 ? x - fx / dfx : x;
    }
    return x;
}

// the largest cross product of two rows of D - shift I, normalised
SFM_DEVICE V3 null_of(const Sym3& D, double shift) {
    const V3 r0{D.a00 - shift, D.a01, D.a02}, r1{D.a01, D.a11 - shift, D.a12}, r2{D.a02, D.a12, D.a22 - shift};
    const V3 v0 = cross3(r0, r1), v1 = cross3(r0, r2), v2 = cross3(r1, r2);
    const double n0 = dot3(v0, v0), n1 = dot3(v1, v1), n2 = dot3(v2, v2);
    // component-wise selects: a selected struct would be addressed through the stack
    const bool t1 = n1 > n0;
    const double m1 = t1 ? n1 : n0;
    const bool t2 = n2 > m1;
    const double n = t2 ? n2 : m1;
    const double x = t2 ? v2.x : (t1 ? v1.x : v0.x);
    const double y = t2 ? v2.y : (t1 ? v1.y : v0.y);
    const double z = t2 ? v2.z : (t1 ? v1.z : v0.z);
    const double inv = 1.0 / sqrt(n);
    return {x * inv, y * inv, z * inv};
}

// p^T E q
SFM_DEVICE double quad(const Sym3& E, const V3& p, const V3& q) {
    return (p.x * ((E.a00 * q.x + E.a01 * q.y) + E.a02 * q.z) + p.y * ((E.a01 * q.x + E.a11 * q.y) + E.a12 * q.z)) +
           p.z * ((E.a02 * q.x + E.a12 * q.y) + E.a22 * q.z);
}

struct Eqs {
    double a01, a02, a12, c01, c02, c12;
};

SFM_DEVICE void residuals(const V3& l, const Eqs& e, double& r01, double& r02, double& r12) {
    r01 = ((l.x * l.x + l.y * l.y) - 2.0 * e.c01 * l.x * l.y) - e.a01;
    r02 = ((l.x * l.x + l.z * l.z) - 2.0 * e.c02 * l.x * l.z) - e.a02;
    r12 = ((l.y * l.y + l.z * l.z) - 2.0 * e.c12 * l.y * l.z) - e.a12;
}

SFM_DEVICE V3 newton(const V3& l, const Eqs& e) {
    double r01, r02, r12;
    residuals(l, e, r01, r02, r12);
    const double j00 = 2.0 * (l.x - e.c01 * l.y), j01 = 2.0 * (l.y - e.c01 * l.x);
    const double j10 = 2.0 * (l.x - e.c02 * l.z), j12 = 2.0 * (l.z - e.c02 * l.x);
    const double j21 = 2.0 * (l.y - e.c12 * l.z), j22 = 2.0 * (l.z - e.c12 * l.y);
    // J = [[j00, j01, 0], [j10, 0, j12], [0, j21, j22]]
    const double det = -(j00 * j12) * j21 - (j01 * j10) * j22;
    if (!(det != 0.0 && isfinite(det))) return l;
    const double d0 = (-(r01 * j12) * j21 - j01 * (r02 * j22 - j12 * r12)) / det;
    const double d1 = (j00 * (r02 * j22 - j12 * r12) - (r01 * j10) * j22) / det;
    const double d2 = ((-(j00 * r02) * j21 - (j01 * j10) * r12) + (r01 * j10) * j21) / det;
    return {l.x - d0, l.y - d1, l.z - d2};
}

// The fixed 3-D side of every candidate's pose: the inverse of [d01, d02, d01 x d02] by rows, times det.
struct Frame {
    V3 m0, m1, m2;
    double det;
};

// One ray of a plane: scale, polish, pose, score on item 3, keep if strictly better than `best`.
SFM_DEVICE void try_ray(V3 l, const Eqs& e, const V3& f0, const V3& f1, const V3& f2, const V3& X0, const Frame& F,
                        const sfmpnp::PnPCamera& k, const double* q3, double& best, double out[12]) {
    const double asum = (e.a01 + e.a02) + e.a12;
    const double qs = (((l.x * l.x + l.y * l.y) - 2.0 * e.c01 * l.x * l.y) + ((l.x * l.x + l.z * l.z) - 2.0 * e.c02 * l.x * l.z)) +
                      ((l.y * l.y + l.z * l.z) - 2.0 * e.c12 * l.y * l.z);
    double sc = qs > 0.0 ? sqrt(asum / qs) : NAN;
    sc = (l.x + l.y) + l.z < 0.0 ? -sc : sc;
    l = {l.x * sc, l.y * sc, l.z * sc};
#pragma unroll
    for (int i = 0; i < kNewtonSteps; ++i) l = newton(l, e);
    double r01, r02, r12;
    residuals(l, e, r01, r02, r12);
    const double tol = kResidualTol * asum;
    if (!(l.x > 0.0 && l.y > 0.0 && l.z > 0.0 && fabs(r01) <= tol && fabs(r02) <= tol && fabs(r12) <= tol)) return;
    const V3 Y0{l.x * f0.x, l.x * f0.y, l.x * f0.z};
    const V3 Y1{l.y * f1.x, l.y * f1.y, l.y * f1.z};
    const V3 Y2{l.z * f2.x, l.z * f2.y, l.z * f2.z};
    const V3 e01 = sub3(Y1, Y0), e02 = sub3(Y2, Y0);
    const V3 nY = cross3(e01, e02);
    const double a[3] = {e01.x, e01.y, e01.z}, b[3] = {e02.x, e02.y, e02.z}, n[3] = {nY.x, nY.y, nY.z};
    const double M0[3] = {F.m0.x, F.m0.y, F.m0.z}, M1[3] = {F.m1.x, F.m1.y, F.m1.z}, M2[3] = {F.m2.x, F.m2.y, F.m2.z};
    const double x0[3] = {X0.x, X0.y, X0.z}, y0[3] = {Y0.x, Y0.y, Y0.z};
    double m[12];
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) m[3 * r + c] = ((a[r] * M0[c] + b[r] * M1[c]) + n[r] * M2[c]) / F.det;
        m[9 + r] = y0[r] - ((m[3 * r] * x0[0] + m[3 * r + 1] * x0[1]) + m[3 * r + 2] * x0[2]);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) finite = finite && isfinite(m[i]);
    if (!finite) return;
    const double s = sfmpnp::pnp_score(m, k, q3[0], q3[1], q3[2], q3[3], q3[4]);
    if (s < best) {
        best = s;
#pragma unroll
        for (int i = 0; i < 12; ++i) out[i] = m[i];
    }
}

// The P3P fit of one hypothesis: p[i] = {X, Y, Z, u, v} of sample item i (0-2 solved for, 3 picks).  Writes the chosen
// model, or 12 NaNs when no candidate scores below +inf; returns false when items 0-2 are collinear or coincide (the model
// is then 12 NaNs as well).
SFM_DEVICE bool p3p_fit_one(const double* p0, const double* p1, const double* p2, const double* p3, const sfmpnp::PnPCamera& k,
                            double out[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = NAN;
    const V3 X0{p0[0], p0[1], p0[2]}, X1{p1[0], p1[1], p1[2]}, X2{p2[0], p2[1], p2[2]};
    if (collinear(X0, X1, X2)) return false;
    const V3 f0 = bearing(p0[3], p0[4], k), f1 = bearing(p1[3], p1[4], k), f2 = bearing(p2[3], p2[4], k);
    const V3 d01 = sub3(X1, X0), d02 = sub3(X2, X0), d12 = sub3(X2, X1);
    const Eqs e{dot3(d01, d01), dot3(d02, d02), dot3(d12, d12), dot3(f0, f1), dot3(f0, f2), dot3(f1, f2)};
    const Sym3 D1{e.a12, -e.a12 * e.c01, 0.0, e.a12 - e.a01, e.a01 * e.c12, -e.a01};
    const Sym3 D2{e.a12, 0.0, -e.a12 * e.c02, -e.a02, e.a02 * e.c12, e.a12 - e.a02};
    const Cof C1 = cofactors(D1), C2 = cofactors(D2);
    const double k0 = (D1.a00 * C1.c00 + D1.a01 * C1.c01) + D1.a02 * C1.c02;
    const double k3 = (D2.a00 * C2.c00 + D2.a01 * C2.c01) + D2.a02 * C2.c02;
    const double k1 = trace_adj(C1, D2);
    const double k2 = trace_adj(C2, D1);
    const bool d1_leads = fabs(k3) >= fabs(k0);
    const Sym3 A = d1_leads ? D1 : D2, B = d1_leads ? D2 : D1;
    const double g = d1_leads ? (k3 != 0.0 ? cubic_root(k2 / k3, k1 / k3, k0 / k3) : 0.0) : cubic_root(k1 / k0, k2 / k0, k3 / k0);
    const Sym3 D0{A.a00 + g * B.a00, A.a01 + g * B.a01, A.a02 + g * B.a02, A.a11 + g * B.a11, A.a12 + g * B.a12, A.a22 + g * B.a22};
    const Sym3 E = fabs(g) <= 1.0 ? B : A;
    const Cof C0 = cofactors(D0);
    const double tr = (D0.a00 + D0.a11) + D0.a22;
    const double mm = (C0.c00 + C0.c11) + C0.c22;
    const double sq = sqrt(fmax(tr * tr - 4.0 * mm, 0.0));
    const double s1 = tr >= 0.0 ? 0.5 * (tr + sq) : 0.5 * (tr - sq);
    const double s2 = mm / s1;
    const V3 e1 = null_of(D0, s1);
    const V3 e3 = null_of(D0, 0.0);
    const V3 e2 = cross3(e3, e1);
    const double s = sqrt(fmax(-s2 / s1, 0.0));
    const V3 nX = cross3(d01, d02);
    const Frame F{cross3(d02, nX), cross3(nX, d01), nX, dot3(nX, nX)};
    double best = INFINITY;
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
        const double sign = plane == 0 ? 1.0 : -1.0;
        const V3 n{e1.x + sign * s * e2.x, e1.y + sign * s * e2.y, e1.z + sign * s * e2.z};
        const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
        const int kk = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
        const V3 axis{kk == 0 ? 1.0 : 0.0, kk == 1 ? 1.0 : 0.0, kk == 2 ? 1.0 : 0.0};
        const V3 p = cross3(n, axis);
        const V3 q = cross3(n, p);
        const double G00 = quad(E, p, p), G01 = quad(E, p, q), G11 = quad(E, q, q);
        const double disc = G01 * G01 - G00 * G11;
        if (!(disc >= 0.0)) continue;
        const double sd = sqrt(disc);
        const bool p_side = fabs(G00) >= fabs(G11);
        const double lead = p_side ? G00 : G11, tail = p_side ? G11 : G00;
        const double r1 = (-G01 - copysign(sd, G01)) / lead;
        const double r2 = tail / (lead * r1);
#pragma unroll
        for (int ray = 0; ray < 2; ++ray) {
            const double r = ray == 0 ? r1 : r2;
            const V3 l = p_side ? V3{r * p.x + q.x, r * p.y + q.y, r * p.z + q.z} : V3{p.x + r * q.x, p.y + r * q.y, p.z + r * q.z};
            try_ray(l, e, f0, f1, f2, X0, F, k, p3, best, out);
        }
    }
    return true;
}

}  // namespace sfmp3p
