"""The NumPy definition of the refinement of every pair's relative pose (csrc/sfm_view_graph_refine.hip,
sfm_refine_pair_poses): the start set re-scored under the start pose, the rounds, the LM steps, the lambda
schedule, the stopping rules, the rank check and the accept rule, with the error of an item from
``oracle.sfm_oracle.sed_values`` under E = [t]x R.  Constants and loops are its own; E is formed in the entry's operation
order and the tangent basis follows the entry's rule.  Only the summation order differs from the device.  ``trace`` (a dict)
collects what the margin tests of tests/test_pair_refine_host.py need: every re-scored error and every accept test."""
import numpy as np

from oracle import sfm_oracle as orc

MIN_ITEMS = 6
UNKNOWNS = 5
LAMBDA0 = 1e-3
LAMBDA_MAX = 1e16
MIN_DECREASE = 1e-12
MIN_STEP = 1e-12
RANK_FLOOR = 1e-10
SUM, SQUARE, MEAN, RMS = 0, 1, 2, 3
OK, NO_POSE, TOO_FEW = range(3)
STATUS = ("ok", "no_pose", "too_few")
POSE_OK = 0
INFO_DTYPE = np.dtype([("start_error", "<f8"), ("error", "<f8"), ("start_count", "<i4"), ("count", "<i4"), ("accepted", "<i4"),
                       ("lm_steps", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
INFO_BYTES = 40


def essential(R, t):
    """[t]x R, each entry two products and one subtraction."""
    E = np.empty((3, 3))
    for j in range(3):
        E[0, j] = t[1] * R[2, j] - t[2] * R[1, j]
        E[1, j] = t[2] * R[0, j] - t[0] * R[2, j]
        E[2, j] = t[0] * R[1, j] - t[1] * R[0, j]
    return E


def tangent_basis(t):
    """(b1, b2): e the axis of the smallest |t_i| (the first on ties), b1 = (t x e) / |t x e|, b2 = t x b1."""
    e = np.zeros(3)
    e[int(np.argmin(np.abs(t)))] = 1.0   # argmin returns the first minimum
    c = np.array([t[1] * e[2] - t[2] * e[1], t[2] * e[0] - t[0] * e[2], t[0] * e[1] - t[1] * e[0]])
    b1 = c / np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    b2 = np.array([t[1] * b1[2] - t[2] * b1[1], t[2] * b1[0] - t[0] * b1[2], t[0] * b1[1] - t[1] * b1[0]])
    return b1, b2


def derivatives(R, t):
    """(5, 3, 3): dE / d omega_k = [t]x [e_k]x R, dE / da = [b1]x R, dE / db = [b2]x R."""
    G = [np.array([np.zeros(3), -R[2], R[1]]), np.array([R[2], np.zeros(3), -R[0]]), np.array([-R[1], R[0], np.zeros(3)])]
    b1, b2 = tangent_basis(t)
    return np.array([essential(g, t) for g in G] + [essential(R, b1), essential(R, b2)])


def residuals_and_jacobian(R, t, corr):
    """(res (m, 2), J (m, 2, 5)): the residuals r / sqrt(da), r / sqrt(db) of every item and their derivatives."""
    E = essential(R, t)
    xa, ya, xb, yb = (corr[:, k] for k in range(4))
    lb0 = (xb * E[0, 0] + yb * E[1, 0]) + E[2, 0]
    lb1 = (xb * E[0, 1] + yb * E[1, 1]) + E[2, 1]
    lb2 = (xb * E[0, 2] + yb * E[1, 2]) + E[2, 2]
    r = (lb0 * xa + lb1 * ya) + lb2
    la0 = (E[0, 0] * xa + E[0, 1] * ya) + E[0, 2]
    la1 = (E[1, 0] * xa + E[1, 1] * ya) + E[1, 2]
    da = la0 * la0 + la1 * la1
    db = lb0 * lb0 + lb1 * lb1
    ia, ib = 1.0 / np.sqrt(da), 1.0 / np.sqrt(db)
    ra, rb = r * ia, r * ib
    ca, cb = ra / da, rb / db
    J = np.empty((len(corr), 2, UNKNOWNS))
    for k, D in enumerate(derivatives(R, t)):
        v0 = (D[0, 0] * xa + D[0, 1] * ya) + D[0, 2]
        v1 = (D[1, 0] * xa + D[1, 1] * ya) + D[1, 2]
        v2 = (D[2, 0] * xa + D[2, 1] * ya) + D[2, 2]
        dr = (xb * v0 + yb * v1) + v2
        w0 = (xb * D[0, 0] + yb * D[1, 0]) + D[2, 0]
        w1 = (xb * D[0, 1] + yb * D[1, 1]) + D[2, 1]
        J[:, 0, k] = dr * ia - ca * (la0 * v0 + la1 * v1)
        J[:, 1, k] = dr * ib - cb * (lb0 * w0 + lb1 * w1)
    return np.column_stack([ra, rb]), J


def cost(R, t, corr):
    """C = sum of the scorer's error over the items corr."""
    return float(np.sum(orc.sed_values(essential(R, t), corr)))


def system(R, t, corr):
    """(H (5, 5), g (5,), C) over the items corr."""
    res, J = residuals_and_jacobian(R, t, corr)
    Jf = J.reshape(-1, UNKNOWNS)
    return Jf.T @ Jf, Jf.T @ res.reshape(-1), cost(R, t, corr)


def cholesky(M, rel):
    """Lower factor of M, or None when a pivot is not above rel times its diagonal entry (rel = 0: not positive)."""
    n = len(M)
    L = np.zeros((n, n))
    for j in range(n):
        s = M[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > rel * M[j, j]:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (M[j, i] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def solve(H, g, lam):
    """delta of (H + lam diag H) delta = -g, or None when the factorisation fails or delta is not finite."""
    n = len(g)
    M = H.copy()
    M[np.diag_indices(n)] = np.diag(H) + lam * np.diag(H)
    L = cholesky(M, 0.0)
    if L is None:
        return None
    y = np.zeros(n)
    for j in range(n):
        y[j] = (-g[j] - np.dot(L[j, :j], y[:j])) / L[j, j]
    d = np.zeros(n)
    for j in range(n - 1, -1, -1):
        d[j] = (y[j] - np.dot(L[j + 1:, j], d[j + 1:])) / L[j, j]
    return d if np.all(np.isfinite(d)) else None


def apply_step(R, t, delta):
    """(exp([w]x) R, (t + a b1 + b b2) / |t + a b1 + b b2|) for delta = (w, a, b): Rodrigues (Taylor form below th = 1e-6)."""
    w = delta[:3]
    th2 = float((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    th = np.sqrt(th2)
    if th < 1e-6:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    b1, b2 = tangent_basis(t)
    x = (t + delta[3] * b1) + delta[4] * b2
    return (np.eye(3) + A * W + B * (W @ W)) @ R, x / np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])


def lm(R, t, corr, max_steps, trace=None):
    """Levenberg-Marquardt on the items corr: -> (R, t, steps).  Returns the start pose when its H is rank-deficient."""
    H, g, C = system(R, t, corr)
    if cholesky(H, RANK_FLOOR) is None:
        return R, t, 0
    lam, steps = LAMBDA0, 0
    while steps < max_steps and not lam > LAMBDA_MAX:
        steps += 1
        delta = solve(H, g, lam)
        if delta is None:
            lam *= 10.0
            continue
        if np.linalg.norm(delta) <= MIN_STEP * (1.0 + 1.0):
            break
        R_new, t_new = apply_step(R, t, delta)
        H_new, g_new, C_new = system(R_new, t_new, corr)
        if trace is not None:
            trace.setdefault("accept_tests", []).append((C, C_new))
        if np.isfinite(C_new) and C_new < C:
            C_old = C
            R, t, H, g, C, lam = R_new, t_new, H_new, g_new, C_new, lam / 10.0
            if C_old - C < MIN_DECREASE * C_old:
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
            return float(np.float64(np.sum(e)) / np.float64(count))
        return float(np.sqrt(np.float64(np.sum(e * e)) / np.float64(count)))


def _score(R, t, corr, thr, trace):
    with np.errstate(invalid="ignore"):
        e = orc.sed_values(essential(R, t), corr) if len(corr) else np.zeros(0)
        inl = e <= thr
    if trace is not None:
        trace.setdefault("scores", []).append(e)
    return e, inl


def refine(corr, R, t, thr, method=RMS, rounds=2, max_steps=20, trace=None):
    """One pair with a pose: -> dict(R, t, mask (uint8, 1 = within thr under the kept pose), start_error, error, start_count,
    count, accepted, lm_steps, status)."""
    R, t = np.array(R, dtype=np.float64).reshape(3, 3), np.array(t, dtype=np.float64).reshape(3)
    e, inl = _score(R, t, corr, thr, trace)
    best_cnt = start_cnt = int(np.count_nonzero(inl))
    best_err = start_err = aggregate(method, best_cnt, e[inl])
    mask = inl
    accepted = steps = 0
    for _ in range(rounds):
        if best_cnt < MIN_ITEMS:
            break
        R_new, t_new, s = lm(R, t, corr[mask], max_steps, trace)
        steps += s
        e, inl = _score(R_new, t_new, corr, thr, trace)
        cnt = int(np.count_nonzero(inl))
        new_err = aggregate(method, cnt, e[inl])
        if not (cnt > best_cnt or (cnt == best_cnt and new_err < best_err)):
            break
        R, t, mask, best_cnt, best_err = R_new, t_new, inl, cnt, new_err
        accepted += 1
    return dict(R=R, t=t, mask=mask.astype(np.uint8), start_error=start_err, error=best_err, start_count=start_cnt,
                count=best_cnt, accepted=accepted, lm_steps=steps, status=OK if start_cnt >= MIN_ITEMS else TOO_FEW)


def refine_pairs(corr, offset, poses, thr, method=RMS, rounds=2, max_steps=20, reverse=False, traces=None):
    """The whole call: ``poses`` a list of dicts with status, R, t (view_graph_pose_oracle.decode's) -> (list of ``refine``
    dicts — for a pair without a pose R and t as given, NaN errors, zero counts, status NO_POSE — and the mask (N,) uint8).
    ``reverse``: every pair visits its items in reverse order (the masks are returned in the given order)."""
    out, mask = [], np.zeros(len(corr), dtype=np.uint8)
    for q, p in enumerate(poses):
        if p["status"] != POSE_OK:
            out.append(dict(R=p["R"], t=p["t"], start_error=np.nan, error=np.nan, start_count=0, count=0, accepted=0, lm_steps=0,
                            status=NO_POSE))
            continue
        lo, hi = int(offset[q]), int(offset[q + 1])
        items = corr[lo:hi][::-1] if reverse else corr[lo:hi]
        trace = None if traces is None else traces.setdefault(q, {})
        r = refine(items, p["R"], p["t"], thr, method, rounds, max_steps, trace)
        mask[lo:hi] = r["mask"][::-1] if reverse else r["mask"]
        out.append(r)
    return out, mask


def threshold_margin(trace, thr):
    """The least |e - thr| / thr over every re-scored item of a trace (inf without one)."""
    e = np.concatenate(trace.get("scores", [np.zeros(0)]))
    e = e[np.isfinite(e)]
    return float(np.min(np.abs(e - thr) / thr)) if len(e) else np.inf


def accept_margin(trace):
    """The least |C_new - C| / C over the accept tests of a trace (inf without one, or for a trial cost that is not finite)."""
    tests = [(c, n) for c, n in trace.get("accept_tests", []) if np.isfinite(n)]
    return min((abs(n - c) / c for c, n in tests), default=np.inf)


def decode_info(info_words):
    """An int64 (Q, 5) info table as a (Q,) array of INFO_DTYPE records."""
    assert INFO_DTYPE.itemsize == INFO_BYTES
    return np.ascontiguousarray(info_words).reshape(-1).view(INFO_DTYPE)


def rotation_error_deg(R, R_true):
    c = (np.trace(R_true.T @ R) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_error_deg(t, t_true):
    c = float(np.dot(t, t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true)))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
