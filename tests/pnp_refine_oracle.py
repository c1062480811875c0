"""NumPy oracle of the refinement of a PnP winner (csrc/sfm_pnp_refine.hip, sfm_pnp_refine): the same rounds, LM steps,
lambda schedule, stopping rules, rank check and accept rule, with e from pnp_oracle.score_values.  Only the summation
order differs from the device."""
import numpy as np

import pnp_oracle

MIN_ITEMS = 6
LAMBDA0 = 1e-3
LAMBDA_MAX = 1e16
MIN_DECREASE = 1e-12
MIN_STEP = 1e-12
RANK_FLOOR = 1e-10
SUM, SQUARE, MEAN, RMS = 0, 1, 2, 3


def system(R, t, K, pts):
    """(H (6, 6), g (6,), C) over the items pts (m, 5): J rows (R X x A_k, A_k), r = (q0 / c2 - u, q1 / c2 - v); an item
    behind the camera makes C infinite and adds nothing to H or g."""
    e = pnp_oracle.score_values(R, t, K, pts)
    C = float(np.sum(e))
    X = pts[:, :3]
    r = X @ R.T
    c = r + t
    front = c[:, 2] > 0.0
    r, c, uv = r[front], c[front], pts[front, 3:5]
    c2 = c[:, 2]
    w0 = ((K[0, 0] * c[:, 0] + K[0, 1] * c[:, 1]) + K[0, 2] * c2) / c2
    w1 = ((K[1, 0] * c[:, 0] + K[1, 1] * c[:, 1]) + K[1, 2] * c2) / c2
    res = np.column_stack([w0 - uv[:, 0], w1 - uv[:, 1]])
    ic = 1.0 / c2
    H = np.zeros((6, 6))
    g = np.zeros(6)
    for row, w in ((0, w0), (1, w1)):
        A = np.column_stack([K[row, 0] * ic, K[row, 1] * ic, (K[row, 2] - w) * ic])
        J = np.hstack([np.cross(r, A), A])
        H += J.T @ J
        g += J.T @ res[:, row]
    return H, g, C


def cholesky(M, rel):
    """Lower factor of M, or None when a pivot is not above rel times its diagonal entry (rel = 0: not positive)."""
    L = np.zeros((6, 6))
    for j in range(6):
        s = M[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > rel * M[j, j]:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (M[j, i] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def solve(H, g, lam):
    """delta of (H + lam diag H) delta = -g, or None when the factorisation fails or delta is not finite."""
    M = H.copy()
    M[np.diag_indices(6)] = np.diag(H) + lam * np.diag(H)
    L = cholesky(M, 0.0)
    if L is None:
        return None
    y = np.zeros(6)
    for j in range(6):
        y[j] = (-g[j] - np.dot(L[j, :j], y[:j])) / L[j, j]
    d = np.zeros(6)
    for j in range(5, -1, -1):
        d[j] = (y[j] - np.dot(L[j + 1:, j], d[j + 1:])) / L[j, j]
    return d if np.all(np.isfinite(d)) else None


def apply_step(R, t, delta):
    """(exp([w]x) R, t + dt) by the Rodrigues formula (Taylor form below th = 1e-6)."""
    w = delta[:3]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-6:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return (np.eye(3) + A * W + B * (W @ W)) @ R, t + delta[3:]


def lm(R, t, K, pts, max_steps):
    """Levenberg-Marquardt on the items pts: -> (R, t, steps).  Returns the start pose when its H is rank-deficient."""
    H, g, C = system(R, t, K, pts)
    if cholesky(H, RANK_FLOOR) is None:
        return R, t, 0
    lam, steps = LAMBDA0, 0
    while steps < max_steps and not lam > LAMBDA_MAX:
        steps += 1
        delta = solve(H, g, lam)
        if delta is None:
            lam *= 10.0
            continue
        if np.linalg.norm(delta) <= MIN_STEP * (1.0 + np.linalg.norm(t)):
            break
        R_new, t_new = apply_step(R, t, delta)
        H_new, g_new, C_new = system(R_new, t_new, K, pts)
        if np.isfinite(C_new) and C_new < C:
            decrease = C - C_new
            R, t, H, g, lam = R_new, t_new, H_new, g_new, lam / 10.0
            C_old, C = C, C_new
            if decrease < MIN_DECREASE * C_old:
                break
        else:
            lam *= 10.0
    return R, t, steps


def aggregate(method, count, e):
    with np.errstate(invalid="ignore", divide="ignore"):
        if method == SUM:
            return float(np.sum(e))
        if method == SQUARE:
            return float(np.sum(e * e))
        if method == MEAN:
            return float(np.sum(e)) / count
        return float(np.sqrt(np.sum(e * e) / count))


def refine(pts, R, t, K, mask, err, thr, method, rounds=1, max_steps=20):
    """One view: -> dict(R, t, mask (uint8, 1 = inlier), error, count, accepted, lm_steps)."""
    K = np.asarray(K, dtype=np.float64)
    mask = (np.asarray(mask) != 0).astype(np.uint8)
    best_cnt, best_err = int(np.count_nonzero(mask)), float(err)
    accepted = steps = 0
    for _ in range(rounds):
        if best_cnt < MIN_ITEMS:
            break
        R_new, t_new, s = lm(R, t, K, pts[mask != 0], max_steps)
        steps += s
        e = pnp_oracle.score_values(R_new, t_new, K, pts)
        with np.errstate(invalid="ignore"):
            inl = e <= thr
        cnt = int(np.count_nonzero(inl))
        new_err = aggregate(method, cnt, e[inl])
        if not (cnt > best_cnt or (cnt == best_cnt and new_err < best_err)):
            break
        R, t, mask, best_cnt, best_err = R_new, t_new, inl.astype(np.uint8), cnt, new_err
        accepted += 1
    return dict(R=R, t=t, mask=mask, error=best_err, count=best_cnt, accepted=accepted, lm_steps=steps)


def cost(R, t, K, pts):
    """C = sum of e over the items pts."""
    return float(np.sum(pnp_oracle.score_values(R, t, K, pts)))
