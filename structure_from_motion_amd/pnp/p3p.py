"""P3P minimal solver: the host definition of the device fit in ``csrc/sfm_p3p.h`` (same steps, same operation order, fp64).

Three bearings f_i (unit vectors of K^-1 (u, v, 1)) and three 3-D points X_i; the depths lambda_i > 0 satisfy
    q_ij(lambda) = lambda_i^2 + lambda_j^2 - 2 c_ij lambda_i lambda_j = a_ij,   c_ij = f_i . f_j,  a_ij = |X_i - X_j|^2
for the pairs 01, 02, 12.  The structure is that of Lambda Twist (Persson & Nordberg, ECCV 2018):
  1. two homogeneous forms D1 = a12 M01 - a01 M12, D2 = a12 M02 - a02 M12 (M_ij the matrix of q_ij) vanish at every
     solution; a singular member D0 = A + g B of their pencil (one real root g of the cubic det(A + g B) = 0, the larger
     of |det D1|, |det D2| leading) is a pair of planes through the solution rays;
  2. D0 = s1 e1 e1^T + s2 e2 e2^T (its third eigenvalue is 0): the planes are (e1 +- s e2) . lambda = 0, s = sqrt(-s2 / s1);
  3. on each plane, the restriction of the better-conditioned form of the pencil is a binary quadratic: two rays per plane;
  4. each ray scaled to sum(q_ij) = sum(a_ij), then three Newton steps on the three equations;
  5. a ray is a candidate iff its three depths are > 0, its residuals are at most 1e-6 sum(a_ij) and its pose is finite;
     the pose maps [X1 - X0, X2 - X0, (X1 - X0) x (X2 - X0)] onto the same matrix of Y_i = lambda_i f_i.
Up to four candidates, in the order plane +, plane -, and within a plane the two roots of step 3 in their fixed order.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

# |(X1 - X0) x (X2 - X0)|^2 <= floor^2 |X1 - X0|^2 |X2 - X0|^2: the three solve points are collinear or coincide.  This is
# sin^2 of the angle at X0; 1e-9 is far below any triangle a P3P solve can use (the depths then lose all their digits) and
# far above the rounding level of a truly collinear triple (~1e-16), as the DLT's floor on sigma_11 / sigma_1.
COLLINEAR_FLOOR = 1e-9
NEWTON_STEPS = 3
RESIDUAL_TOL = 1e-6


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def bearing(u: float, v: float, K) -> Tuple[float, float, float]:
    """normalise(K^-1 (u, v, 1)) with rows 0 and 1 of K solved by Cramer's rule (row 2 is (0, 0, 1))."""
    k00, k01, k02, k10, k11, k12 = K[0][0], K[0][1], K[0][2], K[1][0], K[1][1], K[1][2]
    du = u - k02
    dv = v - k12
    det = k00 * k11 - k01 * k10
    x = (du * k11 - k01 * dv) / det
    y = (k00 * dv - k10 * du) / det
    inv = 1.0 / math.sqrt((x * x + y * y) + 1.0)
    return (x * inv, y * inv, inv)


def collinear(X0, X1, X2) -> bool:
    d01 = _sub(X1, X0)
    d02 = _sub(X2, X0)
    c = _cross(d01, d02)
    return not (_dot(c, c) > (COLLINEAR_FLOOR * COLLINEAR_FLOOR) * (_dot(d01, d01) * _dot(d02, d02)))


def _cofactors(A):
    """Cofactors (00, 11, 22, 01, 02, 12) of a symmetric 3 x 3 given as (00, 01, 02, 11, 12, 22)."""
    a00, a01, a02, a11, a12, a22 = A
    return (a11 * a22 - a12 * a12, a00 * a22 - a02 * a02, a00 * a11 - a01 * a01,
            a02 * a12 - a01 * a22, a01 * a12 - a02 * a11, a01 * a02 - a00 * a12)


def _trace_adj(C, B):
    """tr(adj(A) B) for the cofactors C of A."""
    b00, b01, b02, b11, b12, b22 = B
    return ((C[0] * b00 + C[1] * b11) + C[2] * b22) + 2.0 * ((C[3] * b01 + C[4] * b02) + C[5] * b12)


def cubic_root(a: float, b: float, c: float) -> float:
    """One real root of x^3 + a x^2 + b x + c: closed form (Cardano with one real root, else the largest of the
    trigonometric three), then two Newton steps, each taken only when the derivative is non-zero."""
    a3 = a / 3.0
    p = b - a * a3
    q = (2.0 * a3 * a3 * a3 - a3 * b) + c
    h = 0.25 * q * q + (p * p * p) / 27.0
    if h > 0.0:
        w = -0.5 * q - math.copysign(math.sqrt(h), q)
        u = math.copysign(abs(w) ** (1.0 / 3.0), w)
        y = u - p / (3.0 * u) if u != 0.0 else 0.0
    else:
        r = math.sqrt(-p / 3.0)
        cs = -0.5 * q / (r * r * r) if r > 0.0 else 0.0
        cs = min(1.0, max(-1.0, cs))
        y = 2.0 * r * math.cos(math.acos(cs) / 3.0)
    x = y - a3
    for _ in range(2):
        fx = ((x + a) * x + b) * x + c
        dfx = (3.0 * x + 2.0 * a) * x + b
        x = x - fx / dfx if dfx != 0.0 else x
    return x


def _null_of(D, shift):
    """The largest cross product of two rows of D - shift I (a null vector when shift is an eigenvalue), normalised."""
    a00, a01, a02, a11, a12, a22 = D
    r0 = (a00 - shift, a01, a02)
    r1 = (a01, a11 - shift, a12)
    r2 = (a02, a12, a22 - shift)
    v0, v1, v2 = _cross(r0, r1), _cross(r0, r2), _cross(r1, r2)
    n0, n1, n2 = _dot(v0, v0), _dot(v1, v1), _dot(v2, v2)
    v, n = v0, n0
    if n1 > n:
        v, n = v1, n1
    if n2 > n:
        v, n = v2, n2
    inv = 1.0 / math.sqrt(n)
    return (v[0] * inv, v[1] * inv, v[2] * inv)


def _quad(E, p, q):
    """p^T E q for a symmetric E given as (00, 01, 02, 11, 12, 22)."""
    e00, e01, e02, e11, e12, e22 = E
    return ((p[0] * ((e00 * q[0] + e01 * q[1]) + e02 * q[2]) + p[1] * ((e01 * q[0] + e11 * q[1]) + e12 * q[2]))
            + p[2] * ((e02 * q[0] + e12 * q[1]) + e22 * q[2]))


def _residuals(l, c01, c02, c12, a01, a02, a12):
    r01 = ((l[0] * l[0] + l[1] * l[1]) - 2.0 * c01 * l[0] * l[1]) - a01
    r02 = ((l[0] * l[0] + l[2] * l[2]) - 2.0 * c02 * l[0] * l[2]) - a02
    r12 = ((l[1] * l[1] + l[2] * l[2]) - 2.0 * c12 * l[1] * l[2]) - a12
    return r01, r02, r12


def _newton(l, c01, c02, c12, a01, a02, a12):
    """One Newton step on the three distance equations (Cramer's rule); no step when the Jacobian is singular."""
    r01, r02, r12 = _residuals(l, c01, c02, c12, a01, a02, a12)
    j00, j01 = 2.0 * (l[0] - c01 * l[1]), 2.0 * (l[1] - c01 * l[0])
    j10, j12 = 2.0 * (l[0] - c02 * l[2]), 2.0 * (l[2] - c02 * l[0])
    j21, j22 = 2.0 * (l[1] - c12 * l[2]), 2.0 * (l[2] - c12 * l[1])
    # J = [[j00, j01, 0], [j10, 0, j12], [0, j21, j22]]
    det = -(j00 * j12) * j21 - (j01 * j10) * j22
    if not (det != 0.0 and math.isfinite(det)):
        return l
    d0 = (-(r01 * j12) * j21 - j01 * (r02 * j22 - j12 * r12)) / det
    d1 = (j00 * (r02 * j22 - j12 * r12) - (r01 * j10) * j22) / det
    d2 = ((-(j00 * r02) * j21 - (j01 * j10) * r12) + (r01 * j10) * j21) / det
    return (l[0] - d0, l[1] - d1, l[2] - d2)


def p3p_solve(X: Sequence[Sequence[float]], f: Sequence[Sequence[float]]) -> List[Tuple[list, list]]:
    """Candidate poses ((R rows), t) of three points X[0..2] seen along unit bearings f[0..2], in the solver's fixed order.
    The caller checks collinearity first (``collinear``)."""
    X0, X1, X2 = (tuple(float(v) for v in x) for x in X[:3])
    f0, f1, f2 = (tuple(float(v) for v in y) for y in f[:3])
    d01, d02, d12 = _sub(X1, X0), _sub(X2, X0), _sub(X2, X1)
    a01, a02, a12 = _dot(d01, d01), _dot(d02, d02), _dot(d12, d12)
    c01, c02, c12 = _dot(f0, f1), _dot(f0, f2), _dot(f1, f2)
    D1 = (a12, -a12 * c01, 0.0, a12 - a01, a01 * c12, -a01)
    D2 = (a12, 0.0, -a12 * c02, -a02, a02 * c12, a12 - a02)
    C1, C2 = _cofactors(D1), _cofactors(D2)
    k0 = (D1[0] * C1[0] + D1[1] * C1[3]) + D1[2] * C1[4]
    k3 = (D2[0] * C2[0] + D2[1] * C2[3]) + D2[2] * C2[4]
    k1 = _trace_adj(C1, D2)
    k2 = _trace_adj(C2, D1)
    if abs(k3) >= abs(k0):
        A, B = D1, D2
        g = cubic_root(k2 / k3, k1 / k3, k0 / k3) if k3 != 0.0 else 0.0
    else:
        A, B = D2, D1
        g = cubic_root(k1 / k0, k2 / k0, k3 / k0)
    D0 = tuple(A[i] + g * B[i] for i in range(6))
    E = B if abs(g) <= 1.0 else A   # on the planes A = -g B: the restriction of the larger one
    # eigen-decomposition of D0 with its known zero eigenvalue
    C0 = _cofactors(D0)
    tr = (D0[0] + D0[3]) + D0[5]
    m = (C0[0] + C0[1]) + C0[2]
    sq = math.sqrt(max(tr * tr - 4.0 * m, 0.0))
    s1 = 0.5 * (tr + sq) if tr >= 0.0 else 0.5 * (tr - sq)
    s2 = m / s1
    e1 = _null_of(D0, s1)
    e3 = _null_of(D0, 0.0)
    e2 = _cross(e3, e1)
    s = math.sqrt(max(-s2 / s1, 0.0))
    # the pose's fixed 3-D side: the inverse of [d01, d02, d01 x d02] by rows (b x c, c x a, a x b) / det
    nX = _cross(d01, d02)
    detX = _dot(nX, nX)
    Minv = (_cross(d02, nX), _cross(nX, d01), nX)
    asum = (a01 + a02) + a12
    out = []
    for sign in (1.0, -1.0):
        n = (e1[0] + sign * s * e2[0], e1[1] + sign * s * e2[1], e1[2] + sign * s * e2[2])
        an = (abs(n[0]), abs(n[1]), abs(n[2]))
        k = 0 if an[0] <= an[1] and an[0] <= an[2] else (1 if an[1] <= an[2] else 2)
        axis = (1.0 if k == 0 else 0.0, 1.0 if k == 1 else 0.0, 1.0 if k == 2 else 0.0)
        p = _cross(n, axis)
        q = _cross(n, p)
        G00, G01, G11 = _quad(E, p, p), _quad(E, p, q), _quad(E, q, q)
        disc = G01 * G01 - G00 * G11
        if not disc >= 0.0:
            continue
        sd = math.sqrt(disc)
        if abs(G00) >= abs(G11):
            r1 = (-G01 - math.copysign(sd, G01)) / G00
            r2 = G11 / (G00 * r1)
            rays = [(r * p[0] + q[0], r * p[1] + q[1], r * p[2] + q[2]) for r in (r1, r2)]
        else:
            r1 = (-G01 - math.copysign(sd, G01)) / G11
            r2 = G00 / (G11 * r1)
            rays = [(p[0] + r * q[0], p[1] + r * q[1], p[2] + r * q[2]) for r in (r1, r2)]
        for l in rays:
            qs = ((((l[0] * l[0] + l[1] * l[1]) - 2.0 * c01 * l[0] * l[1])
                   + ((l[0] * l[0] + l[2] * l[2]) - 2.0 * c02 * l[0] * l[2]))
                  + ((l[1] * l[1] + l[2] * l[2]) - 2.0 * c12 * l[1] * l[2]))
            sc = math.sqrt(asum / qs) if qs > 0.0 else math.nan
            sc = -sc if (l[0] + l[1]) + l[2] < 0.0 else sc
            l = (l[0] * sc, l[1] * sc, l[2] * sc)
            for _ in range(NEWTON_STEPS):
                l = _newton(l, c01, c02, c12, a01, a02, a12)
            r01, r02, r12 = _residuals(l, c01, c02, c12, a01, a02, a12)
            tol = RESIDUAL_TOL * asum
            if not (l[0] > 0.0 and l[1] > 0.0 and l[2] > 0.0 and abs(r01) <= tol and abs(r02) <= tol and abs(r12) <= tol):
                continue
            Y0 = (l[0] * f0[0], l[0] * f0[1], l[0] * f0[2])
            Y1 = (l[1] * f1[0], l[1] * f1[1], l[1] * f1[2])
            Y2 = (l[2] * f2[0], l[2] * f2[1], l[2] * f2[2])
            e01, e02 = _sub(Y1, Y0), _sub(Y2, Y0)
            nY = _cross(e01, e02)
            R = [[((e01[r] * Minv[0][c] + e02[r] * Minv[1][c]) + nY[r] * Minv[2][c]) / detX for c in range(3)]
                 for r in range(3)]
            t = [Y0[r] - ((R[r][0] * X0[0] + R[r][1] * X0[1]) + R[r][2] * X0[2]) for r in range(3)]
            if all(math.isfinite(v) for v in R[0] + R[1] + R[2] + t):
                out.append((R, t))
    return out
