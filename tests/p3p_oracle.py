"""NumPy oracle of the P3P fitter (structure_from_motion_amd/pnp/p3p.py, csrc/sfm_p3p.h) by a different method.

Grunert's substitution: with lambda_1 = u lambda_0 and lambda_2 = v lambda_0 the three distance equations
    lambda_0^2 (1 + u^2 - 2 c01 u) = a01,  lambda_0^2 (1 + v^2 - 2 c02 v) = a02,  lambda_0^2 (u^2 + v^2 - 2 c12 u v) = a12
lose lambda_0 in two ratios, F(u, v) = 0 and G(u, v) = 0, both quadratic in u.  Their resultant in u is a quartic in v,
solved by ``numpy.roots``; u follows from F - G (linear in u), lambda_0 from the second equation.  Each real root is
polished by Newton on the three equations (``numpy.linalg.solve``) and the pose is the SVD alignment (Kabsch) of the three
points onto lambda_i f_i.  The selection rule of the product (item 3, strict <, earliest first) is applied on top.
"""
import numpy as np
from numpy.polynomial import polynomial as P

import pnp_oracle
from structure_from_motion_amd.synthetic import planar_pnp_scene  # noqa: F401  (the planar scene of the tests)

COLLINEAR_FLOOR = 1e-9


class Degenerate(Exception):
    pass


def bearings(uv, K):
    """Unit vectors of K^-1 (u, v, 1), (m, 3)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    h = np.linalg.solve(np.asarray(K, dtype=np.float64), np.column_stack([uv, np.ones(len(uv))]).T).T
    return h / np.linalg.norm(h, axis=1, keepdims=True)


def collinear(X):
    d1, d2 = X[1] - X[0], X[2] - X[0]
    c = np.cross(d1, d2)
    return not (c @ c > COLLINEAR_FLOOR**2 * (d1 @ d1) * (d2 @ d2))


def _equations(X, f):
    a = np.array([np.sum((X[i] - X[j]) ** 2) for i, j in ((0, 1), (0, 2), (1, 2))])
    c = np.array([f[i] @ f[j] for i, j in ((0, 1), (0, 2), (1, 2))])
    return a, c


def _residual(lam, a, c):
    pairs = ((0, 1), (0, 2), (1, 2))
    return np.array([lam[i] ** 2 + lam[j] ** 2 - 2 * c[k] * lam[i] * lam[j] - a[k] for k, (i, j) in enumerate(pairs)])


def _jacobian(lam, a, c):
    J = np.zeros((3, 3))
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        J[k, i] = 2 * (lam[i] - c[k] * lam[j])
        J[k, j] = 2 * (lam[j] - c[k] * lam[i])
    return J


def kabsch(X, Y):
    """The proper rotation R and t with R X_i + t = Y_i in the least-squares sense."""
    cx, cy = X.mean(axis=0), Y.mean(axis=0)
    H = (X - cx).T @ (Y - cy)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cy - R @ cx


def depth_candidates(X, f):
    """Positive depth triples (lambda_0, lambda_1, lambda_2) of every real solution."""
    a, c = _equations(X, f)
    a01, a02, a12 = a
    c01, c02, c12 = c
    w = np.array([1.0, -2 * c02, 1.0])                     # 1 - 2 c02 v + v^2 (coefficients in increasing powers of v)
    # F = a02 u^2 - 2 a02 c01 u + (a02 - a01 w);  G = a02 u^2 - 2 a02 c12 v u + (a02 v^2 - a12 w)
    f2, f1, f0 = np.array([a02]), np.array([-2 * a02 * c01]), P.polysub([a02], a01 * w)
    g2, g1, g0 = np.array([a02]), np.array([0.0, -2 * a02 * c12]), P.polysub([0.0, 0.0, a02], a12 * w)
    m = P.polymul
    res = P.polysub(m(P.polysub(m(f2, g0), m(f0, g2)), P.polysub(m(f2, g0), m(f0, g2))),
                    m(P.polysub(m(f2, g1), m(f1, g2)), P.polysub(m(f1, g0), m(f0, g1))))
    res = np.trim_zeros(res, "b")
    out = []
    for v in np.roots(res[::-1]):
        if abs(v.imag) > 1e-6 * max(1.0, abs(v.real)):
            continue
        v = v.real
        den = 2 * a02 * (c01 - c12 * v)
        u = (P.polyval(v, P.polysub(f0, g0))) / den        # F - G = 2 a02 (c12 v - c01) u + (f0 - g0)
        q = 1 - 2 * c02 * v + v * v
        if not (q > 0 and np.isfinite(u)):
            continue
        lam = np.sqrt(a02 / q) * np.array([1.0, u, v])
        for _ in range(6):
            try:
                lam = lam - np.linalg.solve(_jacobian(lam, a, c), _residual(lam, a, c))
            except np.linalg.LinAlgError:
                break
        if np.all(lam > 0) and np.max(np.abs(_residual(lam, a, c))) <= 1e-6 * a.sum():
            if not any(np.allclose(lam, o, rtol=1e-9, atol=0) for o in out):
                out.append(lam)
    return out


def candidates(X, uv, K):
    """Candidate poses (R, t) of the first three items; raises Degenerate for a collinear triple."""
    X = np.asarray(X, dtype=np.float64)[:3]
    if collinear(X):
        raise Degenerate()
    f = bearings(np.asarray(uv)[:3], K)
    return [kabsch(X, lam[:, None] * f) for lam in depth_candidates(X, f)]


def fit(X, uv, K):
    """(R, t) chosen by item 3 (strict <, earliest first), or NaNs when no candidate scores below +inf."""
    X = np.asarray(X, dtype=np.float64)
    uv = np.asarray(uv, dtype=np.float64)
    best, best_e = (np.full((3, 3), np.nan), np.full(3, np.nan)), np.inf
    for R, t in candidates(X, uv, K):
        e = pnp_oracle.score_one(R, t, K, X[3], uv[3, 0], uv[3, 1])
        if e < best_e:
            best, best_e = (R, t), e
    return best


def condition(X, R, t):
    """Sensitivity of the pose to rounding: |lambda change per unit relative residual| (the depth Jacobian's smallest
    singular value against sum a_ij) times the norm of the inverse 3-D frame [X1 - X0, X2 - X0, n] the pose is read from.
    The P3P problem is ill-conditioned near the danger cylinder (the camera centre on the cylinder through the three
    points, perpendicular to their plane), where the depth Jacobian is singular: pose errors of any solver scale with it."""
    X = np.asarray(X, dtype=np.float64)[:3]
    Y = X @ np.asarray(R).T + np.asarray(t)
    lam = np.linalg.norm(Y, axis=1)
    a, c = _equations(X, Y / lam[:, None])
    J = _jacobian(lam, a, c)
    d1, d2 = X[1] - X[0], X[2] - X[0]
    M = np.column_stack([d1, d2, np.cross(d1, d2)])
    return a.sum() / np.linalg.svd(J, compute_uv=False)[-1] * np.linalg.norm(np.linalg.inv(M), 2) * np.sqrt(a.sum())


def rotation_angle(R1, R2):
    """Angle in rad between two rotations, accurate for small angles (from the chord, not the trace)."""
    return 2.0 * np.arcsin(min(1.0, np.linalg.norm(np.asarray(R1) - np.asarray(R2)) / (2.0 * np.sqrt(2.0))))


def pose_error(R1, t1, R2, t2):
    """(rotation angle, |t1 - t2| / |t2|)."""
    return rotation_angle(R1, R2), float(np.linalg.norm(np.asarray(t1) - np.asarray(t2)) / np.linalg.norm(t2))
