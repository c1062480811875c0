// The similarity model b ~ s R a + t between two point clouds as device routines: the closed-form least-squares
// solve from centred moments (Umeyama 1991; Horn 1987), the three-item solver of the shared fit kernel (sfm_minimal_fit.h), the
// error of one pair and the `Model` of the shared scoring and mask kernels (sfm_minimal_score.h).  What the minimal fit, the
// masked fit and the refinement of sfm_similarity.hip share, so that all three run the same operations in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfmsim {

constexpr int kSimilaritySample = 3;
constexpr int kSimilarityModel = 13;   // R row-major (9) | t (3) | s
// The rotation is determined iff d = sigma_2 + sign(det M) sigma_3 > 0 (half the gap between the two largest eigenvalues of
// Horn's 4 x 4 matrix); a set is degenerate when d is not above this share of sqrt(sigma_a^2 sigma_b^2).
constexpr double kSimilarityDegenerateFloor = 1e-9;

// One pair {a, b}: 48 bytes, read as three 16-byte loads.
struct alignas(16) SimPair {
    double ax, ay, az, bx, by, bz;
};
static_assert(sizeof(SimPair) == 48, "a pair is six doubles");

// The centred moments of an index set I: M = sum b' a'^T (row-major, M[3r + c] = sum b'_r a'_c), sa2 = sum |a'|^2,
// sb2 = sum |b'|^2, with the means mu_a, mu_b over I.
struct Moments {
    double M[9], sa2, sb2, mua[3], mub[3];
};

// --------------------------------------------------------------------------------------------------
// The least-squares model of a set from its moments:
//   1. one-sided Jacobi SVD of M (sfm::hestenes_svd: the columns of g become sigma_k u_k, v holds V);
//   2. the column of smallest norm is dropped and its left vector completed as det(V) (u_p x u_q) from the two kept ones, in
//      cyclic order: R = sum u_k v_k^T is then a proper rotation whatever the rank (2 for a three-item sample) and whatever the
//      sign of det M — this is U diag(1, 1, det U det V) V^T;
//   3. s = tr(R^T M) / sa2, t = mu_b - s R mu_a;
//   4. flag: d <= floor sqrt(sa2 sb2) with d = sigma_2 + sign(det M) sigma_3 (det M from its entries; d = sigma_2 when it is 0),
//      sa2 = 0, s not finite or <= 0, or anything not a number.
// Every index is a compile-time constant: the choice of the dropped column is made by selects, so nothing is addressed at
// run time.  The model of a flagged set is written as it comes out; the selection never takes it.
// --------------------------------------------------------------------------------------------------
SFM_DEVICE int solve(const Moments& mo, double (&out)[kSimilarityModel]) {
    const double* M = mo.M;
    double g[3][3], v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) g[c][r] = M[3 * r + c];
    sfm::hestenes_svd<3>(g, v);
    double n2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) n2[c] = (g[c][0] * g[c][0] + g[c][1] * g[c][1]) + g[c][2] * g[c][2];
    const bool drop0 = n2[0] <= n2[1] && n2[0] <= n2[2];
    const bool drop1 = !drop0 && n2[1] <= n2[2];
    // (p, q, dropped) is a cyclic permutation of (0, 1, 2)
    double gp[3], gq[3], vp[3], vq[3], vd[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        gp[r] = drop0 ? g[1][r] : (drop1 ? g[2][r] : g[0][r]);
        gq[r] = drop0 ? g[2][r] : (drop1 ? g[0][r] : g[1][r]);
        vp[r] = drop0 ? v[1][r] : (drop1 ? v[2][r] : v[0][r]);
        vq[r] = drop0 ? v[2][r] : (drop1 ? v[0][r] : v[1][r]);
        vd[r] = drop0 ? v[0][r] : (drop1 ? v[1][r] : v[2][r]);
    }
    const double np2 = drop0 ? n2[1] : (drop1 ? n2[2] : n2[0]);
    const double nq2 = drop0 ? n2[2] : (drop1 ? n2[0] : n2[1]);
    const double nd2 = drop0 ? n2[0] : (drop1 ? n2[1] : n2[2]);
    const double sp = sqrt(np2), sq = sqrt(nq2), sd = sqrt(nd2);
    double up[3], uq[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        up[r] = gp[r] / sp;
        uq[r] = gq[r] / sq;
    }
    const double det_v = (v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0])) +
                         v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double sign_v = det_v < 0.0 ? -1.0 : 1.0;
    const double ud[3] = {sign_v * (up[1] * uq[2] - up[2] * uq[1]), sign_v * (up[2] * uq[0] - up[0] * uq[2]),
                          sign_v * (up[0] * uq[1] - up[1] * uq[0])};
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (up[r] * vp[c] + uq[r] * vq[c]) + ud[r] * vd[c];
    double trace = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) trace += R[k] * M[k];
    const double s = trace / mo.sa2;
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        t[r] = mo.mub[r] - s * ((R[3 * r] * mo.mua[0] + R[3 * r + 1] * mo.mua[1]) + R[3 * r + 2] * mo.mua[2]);

    const double det_m = (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    const double sigma2 = fmin(sp, sq);
    const double d = det_m < 0.0 ? sigma2 - sd : (det_m > 0.0 ? sigma2 + sd : sigma2);
    bool ok = d > kSimilarityDegenerateFloor * sqrt(mo.sa2 * mo.sb2);   // false for a NaN on either side
    ok = ok && mo.sa2 > 0.0 && s > 0.0 && s < INFINITY;
    double check = s;
#pragma unroll
    for (int k = 0; k < 9; ++k) check += R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) check += t[k];
    ok = ok && check == check && fabs(check) < INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[9 + k] = t[k];
    out[12] = s;
    return ok ? 0 : SFM_FIT_DEGENERATE;
}

// --------------------------------------------------------------------------------------------------
// The error of one pair under a model m = R | t | s, squared and in the units of side B.  Operation order is the contract shared
// with the NumPy definition of tests/similarity_oracle.py (the build uses -ffp-contract=off):
//   p_k = (R[3k] ax + R[3k+1] ay) + R[3k+2] az,  r_k = (s p_k + t_k) - b_k,  e = (r_0^2 + r_1^2) + r_2^2.
// --------------------------------------------------------------------------------------------------
SFM_DEVICE double pair_error(const double (&m)[kSimilarityModel], const SimPair& q) {
    const double p0 = (m[0] * q.ax + m[1] * q.ay) + m[2] * q.az;
    const double p1 = (m[3] * q.ax + m[4] * q.ay) + m[5] * q.az;
    const double p2 = (m[6] * q.ax + m[7] * q.ay) + m[8] * q.az;
    const double r0 = (m[12] * p0 + m[9]) - q.bx;
    const double r1 = (m[12] * p1 + m[10]) - q.by;
    const double r2 = (m[12] * p2 + m[11]) - q.bz;
    return (r0 * r0 + r1 * r1) + r2 * r2;
}

// The three-item solver of sfmmin::minimal_fit_kernel: means, centred moments in item order, solve().
struct similarity_solver {
    static constexpr int kSample = kSimilaritySample, kModel = kSimilarityModel;
    static constexpr const char* kName = "minimal_fit_kernel<similarity_solver>";
    using Data = const SimPair*;
    SFM_DEVICE static Data from(Data pairs, int64_t first) { return pairs + first; }
    SFM_DEVICE static int fit(Data pairs, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[kSimilarityModel]) {
        const SimPair* __restrict__ items = pairs + b * n;
        bool bad = false;
        double a[3][3], c[3][3];
#pragma unroll
        for (int i = 0; i < kSimilaritySample; ++i) {
            const SimPair q = items[checked_index(idx[i], n, bad)];
            a[i][0] = q.ax; a[i][1] = q.ay; a[i][2] = q.az;
            c[i][0] = q.bx; c[i][1] = q.by; c[i][2] = q.bz;
        }
        Moments mo;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mo.mua[k] = ((a[0][k] + a[1][k]) + a[2][k]) / 3.0;
            mo.mub[k] = ((c[0][k] + c[1][k]) + c[2][k]) / 3.0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) mo.M[k] = 0.0;
        mo.sa2 = mo.sb2 = 0.0;
#pragma unroll
        for (int i = 0; i < kSimilaritySample; ++i) {
            double da[3], db[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                da[k] = a[i][k] - mo.mua[k];
                db[k] = c[i][k] - mo.mub[k];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) mo.M[3 * r + k] += db[r] * da[k];
            mo.sa2 += (da[0] * da[0] + da[1] * da[1]) + da[2] * da[2];
            mo.sb2 += (db[0] * db[0] + db[1] * db[1]) + db[2] * db[2];
        }
        const int flag = solve(mo, out);
        return bad ? SFM_FIT_DEGENERATE : flag;
    }
};

// The `Model` of sfm_minimal_score.h: the 13 doubles in registers, the error of a pair.
struct similarity_model {
    using Stored = SimPair;
    using Item = SimPair;
    static constexpr int kStride = 1, kModel = kSimilarityModel;
    double m[kSimilarityModel];
    SFM_DEVICE explicit similarity_model(const double* model) {
#pragma unroll
        for (int i = 0; i < kSimilarityModel; ++i) m[i] = model[i];
    }
    SFM_DEVICE static void load(const SimPair* items, int64_t i, SimPair& slot) { slot = items[i]; }
    SFM_DEVICE double error(const SimPair& q) const { return pair_error(m, q); }
};

}  // namespace sfmsim
