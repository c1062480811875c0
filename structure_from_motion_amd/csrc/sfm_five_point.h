// Five-point essential-matrix solver (Nister, PAMI 2004): the device form of structure_from_motion_amd/epipolar/five_point.py,
// same steps and the same operation order, fp64, one sample per lane with every array indexed at compile time (the loops are
// unrolled; the pivot rows of the elimination are exchanged by selects, never by a runtime index).  DESIGN.md §6l.
//   1. null basis of the 5 x 9 epipolar system: Householder QR of its 9 x 5 transpose, the last four columns of Q mixed by
//      the fixed orthogonal kMix into X, Y, Z, W (the last column alone is orthogonal to the true E when E[2][2] = 0);
//   2. the 10 x 20 coefficient matrix of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 for E = x X + y Y + z Z + W, its left
//      10 x 10 block Gauss-Jordan eliminated with partial pivoting;
//   3. the 3 x 3 polynomial matrix B(z) from rows e - z f, g - z h, i - z j and its determinant n(z) of degree 10;
//   4. real roots of n in ascending order: a Sturm sequence, bisection on its sign-change count, Newton in the bracket;
//   5. per root: (x, y, 1) from the cross product of the two rows of B(z) with the largest third component, (x, y, z)
//      polished by kRefineSteps Newton steps on B(z) (x, y, 1)^T = 0 and kConstraintSteps Gauss-Newton steps on the ten
//      constraints of E = x X + y Y + z Z + W themselves, then E, scaled to ||E||_F = sqrt(2) with its largest-magnitude
//      entry positive, handed to the caller.  The order of the candidates is that of the roots of n before the polish,
//      which can move z past a neighbour; two nearly double roots can be polished onto one solution and come twice.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sfm_common.h"
#include "sfm_math.h"

namespace sfm5 {

constexpr double kRankFloor = 1e-9;   // numerical rank < 5: min |r_kk| <= kRankFloor * max |r_kk|
constexpr int kIsolateSteps = 80;
constexpr int kPolishSteps = 100;
constexpr int kRefineSteps = 2;
constexpr int kConstraintSteps = 2;
constexpr int kMaxCandidates = 10;

// X, Y, Z, W = kMix (the last four columns of Q): the left-multiplication matrix of the quaternion (2, 4, 5, 6) over its norm
constexpr double kMix[4][4] = {{2.0 / 9.0, -4.0 / 9.0, -5.0 / 9.0, -6.0 / 9.0},
                               {4.0 / 9.0, 2.0 / 9.0, -6.0 / 9.0, 5.0 / 9.0},
                               {5.0 / 9.0, 6.0 / 9.0, 2.0 / 9.0, -4.0 / 9.0},
                               {6.0 / 9.0, -5.0 / 9.0, 4.0 / 9.0, 2.0 / 9.0}};

// products of monomials (five_point.py LMUL / QMUL): linear (x, y, z, 1) x linear -> QUAD, QUAD x linear -> CUBIC
constexpr int kLMul[4][4] = {{0, 1, 2, 6}, {1, 3, 4, 7}, {2, 4, 5, 8}, {6, 7, 8, 9}};
constexpr int kQMul[10][4] = {{0, 2, 4, 5},  {2, 3, 8, 9},    {4, 8, 10, 11},  {3, 1, 6, 7},    {8, 6, 13, 14},
                              {10, 13, 16, 17}, {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};

SFM_DEVICE void mul_ll(const double (&a)[4], const double (&b)[4], double (&out)[10]) {
#pragma unroll
    for (int k = 0; k < 10; ++k) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[kLMul[i][j]] = out[kLMul[i][j]] + a[i] * b[j];
}

SFM_DEVICE void mul_ql(const double (&q)[10], const double (&a)[4], double (&out)[20]) {
#pragma unroll
    for (int k = 0; k < 20; ++k) out[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[kQMul[k][i]] = out[kQMul[k][i]] + q[k] * a[i];
}

// Step 1.  Returns true when the sample is degenerate (numerical rank < 5 or an input not finite).
SFM_DEVICE bool null_basis(const double (&xa)[5], const double (&ya)[5], const double (&xb)[5], const double (&yb)[5],
                           double (&basis)[4][9]) {
    double A[9][5];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        A[0][i] = xb[i] * xa[i];
        A[1][i] = xb[i] * ya[i];
        A[2][i] = xb[i];
        A[3][i] = yb[i] * xa[i];
        A[4][i] = yb[i] * ya[i];
        A[5][i] = yb[i];
        A[6][i] = xa[i];
        A[7][i] = ya[i];
        A[8][i] = 1.0;
        finite = finite && isfinite(xa[i]) && isfinite(ya[i]) && isfinite(xb[i]) && isfinite(yb[i]);
    }
    double v[5][9];   // v[k][t]: entry k + t of the k-th Householder vector
    double beta[5];
    double rmax = 0.0, rmin = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double ss = 0.0;
#pragma unroll
        for (int i = k; i < 9; ++i) ss = ss + A[i][k] * A[i][k];
        const double norm = sqrt(ss);
        const double alpha = A[k][k] >= 0.0 ? -norm : norm;
#pragma unroll
        for (int t = 0; t < 9 - k; ++t) v[k][t] = A[k + t][k];
        v[k][0] = v[k][0] - alpha;
        double vv = 0.0;
#pragma unroll
        for (int t = 0; t < 9 - k; ++t) vv = vv + v[k][t] * v[k][t];
        beta[k] = vv > 0.0 ? 2.0 / vv : 0.0;
#pragma unroll
        for (int j = k + 1; j < 5; ++j) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < 9 - k; ++t) s = s + v[k][t] * A[k + t][j];
            s = s * beta[k];
#pragma unroll
            for (int t = 0; t < 9 - k; ++t) A[k + t][j] = A[k + t][j] - s * v[k][t];
        }
        const double r = fabs(alpha);
        rmax = k == 0 ? r : fmax(rmax, r);
        rmin = k == 0 ? r : fmin(rmin, r);
    }
    double q[4][9];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        double y[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) y[i] = i == 5 + m ? 1.0 : 0.0;
#pragma unroll
        for (int k = 4; k >= 0; --k) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < 9 - k; ++t) s = s + v[k][t] * y[k + t];
            s = s * beta[k];
#pragma unroll
            for (int t = 0; t < 9 - k; ++t) y[k + t] = y[k + t] - s * v[k][t];
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) q[m][i] = y[i];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 9; ++i)
            basis[m][i] = ((kMix[m][0] * q[0][i] + kMix[m][1] * q[1][i]) + kMix[m][2] * q[2][i]) + kMix[m][3] * q[3][i];
    return !(rmin > kRankFloor * rmax) || !finite;
}

// Step 2: row 0 det E, rows 1..9 (2 E E^T E - tr(E E^T) E)_ij row-major, columns in Nister's monomial order.
SFM_DEVICE void coefficient_matrix(const double (&basis)[4][9], double (&M)[10][20]) {
    double e[9][4];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int m = 0; m < 4; ++m) e[i][m] = basis[m][i];
    {
        double cof[3][10], t0[10], t1[10];
        mul_ll(e[4], e[8], t0);
        mul_ll(e[5], e[7], t1);
#pragma unroll
        for (int c = 0; c < 10; ++c) cof[0][c] = t0[c] - t1[c];
        mul_ll(e[3], e[8], t0);
        mul_ll(e[5], e[6], t1);
#pragma unroll
        for (int c = 0; c < 10; ++c) cof[1][c] = t0[c] - t1[c];
        mul_ll(e[3], e[7], t0);
        mul_ll(e[4], e[6], t1);
#pragma unroll
        for (int c = 0; c < 10; ++c) cof[2][c] = t0[c] - t1[c];
        double d0[20], d1[20], d2[20];
        mul_ql(cof[0], e[0], d0);
        mul_ql(cof[1], e[1], d1);
        mul_ql(cof[2], e[2], d2);
#pragma unroll
        for (int c = 0; c < 20; ++c) M[0][c] = (d0[c] - d1[c]) + d2[c];
    }
    double eet[3][3][10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            double m0[10], m1[10], m2[10];
            mul_ll(e[3 * i], e[3 * j], m0);
            mul_ll(e[3 * i + 1], e[3 * j + 1], m1);
            mul_ll(e[3 * i + 2], e[3 * j + 2], m2);
#pragma unroll
            for (int c = 0; c < 10; ++c) {
                eet[i][j][c] = (m0[c] + m1[c]) + m2[c];
                eet[j][i][c] = eet[i][j][c];
            }
        }
    double tr[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) tr[c] = (eet[0][0][c] + eet[1][1][c]) + eet[2][2][c];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double lam[3][10];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 10; ++c) lam[k][c] = i == k ? 2.0 * eet[i][k][c] - tr[c] : 2.0 * eet[i][k][c];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double c0[20], c1[20], c2[20];
            mul_ql(lam[0], e[j], c0);
            mul_ql(lam[1], e[3 + j], c1);
            mul_ql(lam[2], e[6 + j], c2);
#pragma unroll
            for (int c = 0; c < 20; ++c) M[1 + 3 * i + j][c] = (c0[c] + c1[c]) + c2[c];
        }
    }
}

// Gauss-Jordan elimination of the left 10 x 10 block with partial pivoting (the first row of largest magnitude); the
// right block of M is left as the reduced system.  The pivot row is exchanged by selects over the candidate rows.
SFM_DEVICE void gauss_jordan(double (&M)[10][20]) {
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        int p = c;
        double big = fabs(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < 10; ++r) {
            const bool take = fabs(M[r][c]) > big;
            big = take ? fabs(M[r][c]) : big;
            p = take ? r : p;
        }
        double piv[20];
#pragma unroll
        for (int j = c; j < 20; ++j) piv[j] = M[c][j];
#pragma unroll
        for (int r = c + 1; r < 10; ++r) {
            const bool hit = p == r;
#pragma unroll
            for (int j = c; j < 20; ++j) {
                const double mine = M[r][j];
                M[r][j] = hit ? piv[j] : mine;
                piv[j] = hit ? mine : piv[j];
            }
        }
        const double inv = 1.0 / piv[c];
#pragma unroll
        for (int j = c + 1; j < 20; ++j) M[c][j] = piv[j] * inv;
        M[c][c] = 1.0;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = M[r][c];
#pragma unroll
            for (int j = c + 1; j < 20; ++j) M[r][j] = M[r][j] - f * M[c][j];
            M[r][c] = 0.0;
        }
    }
}

template <int NA, int NB>
SFM_DEVICE void conv(const double (&a)[NA], const double (&b)[NB], double (&out)[NA + NB - 1]) {
#pragma unroll
    for (int k = 0; k < NA + NB - 1; ++k) out[k] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) out[i + j] = out[i + j] + a[i] * b[j];
}

template <int N>
SFM_DEVICE double horner(const double (&c)[N], double x) {
    double v = c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = v * x + c[i];
    return v;
}

template <int N>
SFM_DEVICE double horner_d(const double (&c)[N], double x) {   // the derivative of c at x
    double v = (double)(N - 1) * c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 1; --i) v = v * x + (double)i * c[i];
    return v;
}

SFM_DEVICE double det3(const double (&m)[3][3]) {
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// det E and 2 E E^T E - tr(E E^T) E (row-major) of e -> F, with G = E E^T, its trace and the cofactors of E.
SFM_DEVICE void constraints(const double (&e)[9], double (&F)[10], double (&G)[3][3], double& tr, double (&cof)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r][c] = (e[3 * r] * e[3 * c] + e[3 * r + 1] * e[3 * c + 1]) + e[3 * r + 2] * e[3 * c + 2];
    tr = (G[0][0] + G[1][1]) + G[2][2];
    cof[0] = e[4] * e[8] - e[5] * e[7];
    cof[1] = e[5] * e[6] - e[3] * e[8];
    cof[2] = e[3] * e[7] - e[4] * e[6];
    cof[3] = e[7] * e[2] - e[8] * e[1];
    cof[4] = e[8] * e[0] - e[6] * e[2];
    cof[5] = e[6] * e[1] - e[7] * e[0];
    cof[6] = e[1] * e[5] - e[2] * e[4];
    cof[7] = e[2] * e[3] - e[0] * e[5];
    cof[8] = e[0] * e[4] - e[1] * e[3];
    F[0] = (e[0] * cof[0] + e[1] * cof[1]) + e[2] * cof[2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            F[1 + 3 * r + c] = 2.0 * ((G[r][0] * e[c] + G[r][1] * e[3 + c]) + G[r][2] * e[6 + c]) - tr * e[3 * r + c];
}

// The derivative of `constraints` at e in the direction d.
SFM_DEVICE void constraints_along(const double (&e)[9], const double (&d)[9], const double (&G)[3][3], double tr,
                                  const double (&cof)[9], double (&out)[10]) {
    double H[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r][c] = (d[3 * r] * e[3 * c] + d[3 * r + 1] * e[3 * c + 1]) + d[3 * r + 2] * e[3 * c + 2];
    const double dtr = 2.0 * ((H[0][0] + H[1][1]) + H[2][2]);
    double dF = cof[0] * d[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) dF = dF + cof[i] * d[i];
    out[0] = dF;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = ((H[r][0] + H[0][r]) * e[c] + (H[r][1] + H[1][r]) * e[3 + c]) + (H[r][2] + H[2][r]) * e[6 + c];
            const double b = (G[r][0] * d[c] + G[r][1] * d[3 + c]) + G[r][2] * d[6 + c];
            out[1 + 3 * r + c] = (2.0 * (a + b) - dtr * e[3 * r + c]) - tr * d[3 * r + c];
        }
}

template <int N>
SFM_DEVICE double horner_at(const double* c, double x) {   // c: N coefficients at a compile-time offset of an unrolled array
    double v = c[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = v * x + c[i];
    return v;
}

// Step 3 on rows (e, f) of the reduced system: the x, y and 1 coefficients of <e> - z <f>, ascending in z.
SFM_DEVICE void reduced_rows(const double (&be)[20], const double (&bf)[20], double (&px)[4], double (&py)[4], double (&p1)[5]) {
    const double* Be = be + 10;
    const double* Bf = bf + 10;
    px[0] = Be[2]; px[1] = Be[1] - Bf[2]; px[2] = Be[0] - Bf[1]; px[3] = -Bf[0];
    py[0] = Be[5]; py[1] = Be[4] - Bf[5]; py[2] = Be[3] - Bf[4]; py[3] = -Bf[3];
    p1[0] = Be[9]; p1[1] = Be[8] - Bf[9]; p1[2] = Be[7] - Bf[8]; p1[3] = Be[6] - Bf[7]; p1[4] = -Bf[6];
}

// Sturm chain s_0..s_10 of n (s_k of degree 10 - k at offset kOff[k] of one flat array, each scaled to max |coef| = 1).
constexpr int kChain = 66;
constexpr int kOff[11] = {0, 11, 21, 30, 38, 45, 51, 56, 60, 63, 65};

template <int N>
SFM_DEVICE double max_abs(const double* c) {
    double m = fabs(c[0]);
#pragma unroll
    for (int i = 1; i < N; ++i) m = fmax(m, fabs(c[i]));
    return m;
}

// Sign changes of the chain at x (zeros skipped).
SFM_DEVICE int sign_changes(const double (&s)[kChain], double x) {
    int changes = 0, last = 0;
#define SFM5_STEP(K)                                                                  \
    {                                                                                 \
        const double v = horner_at<11 - (K)>(s + kOff[K], x);                         \
        const int sg = (v > 0.0) - (v < 0.0);                                         \
        changes += (sg != 0 && last != 0 && sg != last) ? 1 : 0;                      \
        last = sg != 0 ? sg : last;                                                   \
    }
    SFM5_STEP(0) SFM5_STEP(1) SFM5_STEP(2) SFM5_STEP(3) SFM5_STEP(4) SFM5_STEP(5)
    SFM5_STEP(6) SFM5_STEP(7) SFM5_STEP(8) SFM5_STEP(9) SFM5_STEP(10)
#undef SFM5_STEP
    return changes;
}

// The whole solver on one sample.  visit(const double (&E)[9]) is called for every candidate in the order of the roots of n (step 5).
// Returns true when the sample is degenerate (nothing is visited then).
template <class Visit>
SFM_DEVICE bool solve(const double (&xa)[5], const double (&ya)[5], const double (&xb)[5], const double (&yb)[5], Visit&& visit) {
    double basis[4][9];
    const bool degenerate = null_basis(xa, ya, xb, yb, basis);
    if (degenerate) return true;
    double rx[3][4], ry[3][4], r1[3][5], n[11];   // rows k, l, m of B(z): the x, y and 1 coefficients
    {
        double M[10][20];
        coefficient_matrix(basis, M);
        gauss_jordan(M);
        reduced_rows(M[4], M[5], rx[0], ry[0], r1[0]);
        reduced_rows(M[6], M[7], rx[1], ry[1], r1[1]);
        reduced_rows(M[8], M[9], rx[2], ry[2], r1[2]);
        const double (&kx)[4] = rx[0], (&ky)[4] = ry[0], (&lx)[4] = rx[1], (&ly)[4] = ry[1], (&mx)[4] = rx[2], (&my)[4] = ry[2];
        const double (&k1)[5] = r1[0], (&l1)[5] = r1[1], (&m1)[5] = r1[2];
        double p1[8], p2[8], p3[7];
        double u[8], w[8], u7[7], w7[7];
        conv(ky, l1, u);
        conv(k1, ly, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) p1[i] = u[i] - w[i];
        conv(k1, lx, u);
        conv(kx, l1, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) p2[i] = u[i] - w[i];
        conv(kx, ly, u7);
        conv(ky, lx, w7);
#pragma unroll
        for (int i = 0; i < 7; ++i) p3[i] = u7[i] - w7[i];
        double t1[11], t2[11], t3[11];
        conv(p1, mx, t1);
        conv(p2, my, t2);
        conv(p3, m1, t3);
#pragma unroll
        for (int i = 0; i < 11; ++i) n[i] = (t1[i] + t2[i]) + t3[i];
    }
    // Step 4: the Sturm chain of the normalised n
    double s[kChain];
    double dn[10];
    bool ok = true;
    {
        const double scale = max_abs<11>(n);
#pragma unroll
        for (int i = 0; i < 11; ++i) n[i] = n[i] / scale;
#pragma unroll
        for (int i = 0; i < 10; ++i) dn[i] = (double)(i + 1) * n[i + 1];
        const double ds = max_abs<10>(dn);
#pragma unroll
        for (int i = 0; i < 11; ++i) s[i] = n[i];
#pragma unroll
        for (int i = 0; i < 10; ++i) s[kOff[1] + i] = dn[i] / ds;
#pragma unroll
        for (int k = 2; k < 11; ++k) {
            const double* a = s + kOff[k - 2];
            const double* b = s + kOff[k - 1];
            const int db = 11 - k;   // degree of b (compile time after unrolling)
            const double q1 = a[db + 1] / b[db];
            const double q0 = (a[db] - q1 * b[db - 1]) / b[db];
            double r[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                if (i < db) r[i] = i > 0 ? (a[i] - q1 * b[i - 1]) - q0 * b[i] : a[0] - q0 * b[0];
            }
            double rs = fabs(r[0]);
#pragma unroll
            for (int i = 1; i < 10; ++i)
                if (i < db) rs = fmax(rs, fabs(r[i]));
#pragma unroll
            for (int i = 0; i < 10; ++i)
                if (i < db) s[kOff[k] + i] = -(r[i] / rs);
        }
#pragma unroll
        for (int i = 0; i < kChain; ++i) ok = ok && isfinite(s[i]);
        ok = ok && n[10] != 0.0;
    }
    // Fujiwara's bound on the roots
    double bound;
    {
        const double lead = fabs(n[10]);
        double m = fabs(n[9]) / lead;
#pragma unroll
        for (int k = 2; k < 11; ++k) {
            double q = fabs(n[10 - k]) / lead;
            if (k == 10) q = 0.5 * q;
            m = fmax(m, pow(q, 1.0 / (double)k));
        }
        bound = 2.0 * m;
    }
    ok = ok && isfinite(bound);
    if (!ok) return false;
    double lo = -bound;
    int vlo = sign_changes(s, lo);
    const int v_end = sign_changes(s, bound);
    for (int slot = 0; slot < kMaxCandidates && vlo - v_end > 0; ++slot) {
        double hi = bound;
        int vhi = v_end;
        for (int it = 0; it < kIsolateSteps && vlo - vhi > 1; ++it) {   // the smallest root of (lo, bound] alone in (lo, hi]
            const double mid = 0.5 * (lo + hi);
            const int vm = sign_changes(s, mid);
            if (vlo - vm >= 1) {
                hi = mid;
                vhi = vm;
            } else {
                lo = mid;
                vlo = vm;
            }
        }
        double ba = lo, bb = hi;
        double fa = horner(n, ba);
        double z = 0.5 * (ba + bb);
        for (int it = 0; it < kPolishSteps; ++it) {   // Newton inside the bracket
            const double f = horner(n, z);
            const double df = horner(dn, z);
            const bool hit = f == 0.0;
            const bool same = f * fa > 0.0;
            ba = same ? z : ba;
            fa = same ? f : fa;
            bb = same ? bb : z;
            double zn = z - f / df;
            const bool conv = fabs(zn - z) <= 1e-15 * fabs(z);
            zn = ((zn > ba && zn < bb) || conv) ? zn : 0.5 * (ba + bb);
            z = hit ? z : zn;
            if (hit || conv) break;
        }
        // Step 5
        double x = 0.0, y = 0.0;
        {
            double a[3], b[3], c[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                a[r] = horner(rx[r], z);
                b[r] = horner(ry[r], z);
                c[r] = horner(r1[r], z);
            }
            double w = 0.0;
#pragma unroll
            for (int pair = 0; pair < 3; ++pair) {   // rows (0, 1), (0, 2), (1, 2)
                const int r = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
                const double u0 = b[r] * c[q] - c[r] * b[q];
                const double u1 = c[r] * a[q] - a[r] * c[q];
                const double u2 = a[r] * b[q] - b[r] * a[q];
                const bool take = pair == 0 || fabs(u2) > fabs(w);
                x = take ? u0 : x;
                y = take ? u1 : y;
                w = take ? u2 : w;
            }
            x = x / w;
            y = y / w;
        }
        for (int it = 0; it < kRefineSteps; ++it) {   // Newton on F_r = a_r(z) x + b_r(z) y + c_r(z) (Cramer's rule)
            double F[3], J[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double a = horner(rx[r], z), b = horner(ry[r], z), c = horner(r1[r], z);
                const double da = horner_d(rx[r], z), db = horner_d(ry[r], z), dc = horner_d(r1[r], z);
                F[r] = (a * x + b * y) + c;
                J[r][0] = a;
                J[r][1] = b;
                J[r][2] = (da * x + db * y) + dc;
            }
            const double D = det3(J);
            double C[3][3];
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) C[r][j] = j == k ? F[r] : J[r][j];
                d[k] = det3(C) / D;
            }
            const bool step = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);   // a singular Jacobian: keep the point
            x = step ? x - d[0] : x;
            y = step ? y - d[1] : y;
            z = step ? z - d[2] : z;
        }
        double E[9];
        for (int it = 0; it < kConstraintSteps; ++it) {   // Gauss-Newton on the constraints of E = x X + y Y + z Z + W
#pragma unroll
            for (int i = 0; i < 9; ++i) E[i] = ((x * basis[0][i] + y * basis[1][i]) + z * basis[2][i]) + basis[3][i];
            double F[10], G[3][3], tr, cof[9], J[3][10];
            constraints(E, F, G, tr, cof);
#pragma unroll
            for (int m = 0; m < 3; ++m) constraints_along(E, basis[m], G, tr, cof, J[m]);
            double A[3][3], g[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = a; b < 3; ++b) {
                    double acc = J[a][0] * J[b][0];
#pragma unroll
                    for (int k = 1; k < 10; ++k) acc = acc + J[a][k] * J[b][k];
                    A[a][b] = acc;
                    A[b][a] = acc;
                }
                double acc = J[a][0] * F[0];
#pragma unroll
                for (int k = 1; k < 10; ++k) acc = acc + J[a][k] * F[k];
                g[a] = acc;
            }
            const double D = det3(A);
            double C[3][3];
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) C[r][j] = j == k ? g[r] : A[r][j];
                d[k] = det3(C) / D;
            }
            const bool step = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
            x = step ? x - d[0] : x;
            y = step ? y - d[1] : y;
            z = step ? z - d[2] : z;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = ((x * basis[0][i] + y * basis[1][i]) + z * basis[2][i]) + basis[3][i];
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) ss = ss + E[i] * E[i];
        const double scale = sqrt(2.0 / ss);
        double big = fabs(E[0]), lead = E[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) {
            const bool take = fabs(E[i]) > big;
            big = take ? fabs(E[i]) : big;
            lead = take ? E[i] : lead;
        }
        const double sg = lead < 0.0 ? -scale : scale;
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = E[i] * sg;
        visit(E);
        lo = hi;
        vlo = vhi;
    }
    return false;
}

// ---- the solver of the shared fit kernel (sfm_minimal_fit.h); also what the ragged pass of sfm_view_graph.hip fits with ----
constexpr int kFiveSample = 6;   // five items solved for, the sixth picks the solution

// The items of one sample; bad when an index is out of range.
SFM_DEVICE void load_items(const Corr* __restrict__ pts, int64_t n, const int32_t (&idx)[8], double (&xa)[5], double (&ya)[5],
                           double (&xb)[5], double (&yb)[5], Corr& item5, bool& bad) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const Corr p = pts[checked_index(idx[i], n, bad)];
        xa[i] = p.xa;
        ya[i] = p.ya;
        xb[i] = p.xb;
        yb[i] = p.yb;
    }
    item5 = pts[checked_index(idx[5], n, bad)];
}

// Five-point fit of one hypothesis: SFM_FIT_DEGENERATE for a degenerate sample or an index out of range (E = 9 NaNs then),
// otherwise the candidate with the strictly smallest SED on item 5, or 9 NaNs when there is none (flag 0).
struct five_point_solver {
    static constexpr int kSample = kFiveSample, kModel = 9;
    static constexpr const char* kName = "minimal_fit_kernel<five_point_solver>";
    using Data = const Corr*;
    SFM_DEVICE static Data from(Data corr, int64_t first) { return corr + first; }
    SFM_DEVICE static int fit(Data corr, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[9]);
};

SFM_DEVICE int five_point_solver::fit(Data corr, int64_t b, int64_t n, const int32_t (&idx)[8], double (&out)[9]) {
    const Corr* __restrict__ pts = corr + b * n;
    double xa[5], ya[5], xb[5], yb[5];
    Corr q;
    bool bad = false;
    load_items(pts, n, idx, xa, ya, xb, yb, q, bad);
    double best = INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = NAN;
    bool degenerate = true;
    if (!bad) {
        degenerate = sfm5::solve(xa, ya, xb, yb, [&](const double (&E)[9]) {
            const double sed = sfm::sed_value(E, q.xa, q.ya, q.xb, q.yb);
            const bool take = sed < best;
            best = take ? sed : best;
#pragma unroll
            for (int i = 0; i < 9; ++i) out[i] = take ? E[i] : out[i];
        });
    }
    return (bad || degenerate) ? SFM_FIT_DEGENERATE : 0;
}

// The `Model` of sfm_minimal_score.h: E in registers, the symmetric epipolar distance of a correspondence.
struct essential_model {
    using Stored = Corr;
    using Item = Corr;
    static constexpr int kStride = 1, kModel = 9;
    double m[9];
    SFM_DEVICE explicit essential_model(const double* model) {
#pragma unroll
        for (int i = 0; i < 9; ++i) m[i] = model[i];
    }
    SFM_DEVICE static void load(const Corr* items, int64_t i, Corr& slot) { slot = items[i]; }
    SFM_DEVICE double error(const Corr& t) const { return sfm::sed_value(m, t.xa, t.ya, t.xb, t.yb); }
};

}  // namespace sfm5
