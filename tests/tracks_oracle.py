"""NumPy oracle of the triangulation of multi-view tracks (csrc/sfm_tracks.hip, sfm_triangulate_tracks): the N-view DLT by
np.linalg.svd of the whole stacked A, the per-point Levenberg-Marquardt with the rules of pnp_refine_oracle.lm, the
quality checks and the status order of DESIGN.md §6i.  Vectorised over the points of one track length; only the
summation order and the SVD route differ from the device."""
import numpy as np

LAMBDA0 = 1e-3
LAMBDA_MAX = 1e16
MIN_DECREASE = 1e-12
MIN_STEP = 1e-12
RANK_FLOOR = 1e-10
MIN_W = 1e-12
OK, FEW_VIEWS, DEGENERATE, BEHIND, SMALL_ANGLE, LARGE_ERROR, BAD_INDEX = range(7)


def camera_coords(R, t, X):
    """c = R X + t in sfm_pnp_score's operation order; R (..., 3, 3), t (..., 3), X (..., 3)."""
    return np.stack([((R[..., k, 0] * X[..., 0] + R[..., k, 1] * X[..., 1]) + R[..., k, 2] * X[..., 2]) + t[..., k]
                     for k in range(3)], axis=-1)


def score(R, t, K, X, uv):
    """sfm_pnp_score's e (+inf behind the camera), broadcast over the leading axes."""
    c = camera_coords(R, t, X)
    p0 = (K[0, 0] * c[..., 0] + K[0, 1] * c[..., 1]) + K[0, 2] * c[..., 2]
    p1 = (K[1, 0] * c[..., 0] + K[1, 1] * c[..., 1]) + K[1, 2] * c[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        du = p0 / c[..., 2] - uv[..., 0]
        dv = p1 / c[..., 2] - uv[..., 1]
        e = du * du + dv * dv
    return np.where(c[..., 2] <= 0.0, np.inf, e), c


def point_system(X, R, t, K, uv):
    """(F (n,), H (n, 3, 3), g (n, 3)) of n points, each over its k observations: X (n, 3); R (n, k, 3, 3), t (n, k, 3),
    uv (n, k, 2).  F = sum of e; g = J^T r with J = A R (A = dr/dc); an observation behind its camera makes F infinite and
    adds nothing to H or g."""
    e, c = score(R, t, K, X[:, None, :], uv)
    F = np.sum(e, axis=1)
    front = c[..., 2] > 0.0
    c2 = np.where(front, c[..., 2], 1.0)
    w0 = ((K[0, 0] * c[..., 0] + K[0, 1] * c[..., 1]) + K[0, 2] * c[..., 2]) / c2
    w1 = ((K[1, 0] * c[..., 0] + K[1, 1] * c[..., 1]) + K[1, 2] * c[..., 2]) / c2
    ic = np.where(front, 1.0 / c2, 0.0)
    H = np.zeros(X.shape[:1] + (3, 3))
    g = np.zeros_like(X)
    for row, w, u in ((0, w0, uv[..., 0]), (1, w1, uv[..., 1])):
        A = np.stack([K[row, 0] * ic, K[row, 1] * ic, (K[row, 2] - w) * ic], axis=-1)     # (n, k, 3)
        J = np.einsum("nkj,nkji->nki", A, R)
        r = np.where(front, w - u, 0.0)
        H += np.einsum("nki,nkj->nij", J, J)
        g += np.einsum("nki,nk->ni", J, r)
    return F, H, g


def cholesky3(M, rel):
    """(L (n, 3, 3), ok (n,)): lower factors; ok is False where a pivot is not above rel times its diagonal entry."""
    L = np.zeros_like(M)
    ok = np.ones(M.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(3):
            s = M[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
            ok &= s > rel * M[:, j, j]
            L[:, j, j] = np.sqrt(np.where(ok, s, 1.0))
            for i in range(j + 1, 3):
                L[:, i, j] = (M[:, j, i] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    return L, ok


def refine(X, R, t, K, uv, max_steps):
    """LM on each point alone (pnp_refine_oracle.lm's rules): -> (X (n, 3), steps (n,))."""
    X = X.copy()
    n = X.shape[0]
    steps = np.zeros(n, dtype=np.int64)
    F, H, g = point_system(X, R, t, K, uv)
    active = np.isfinite(F) & cholesky3(H, RANK_FLOOR)[1]
    lam = np.full(n, LAMBDA0)
    diag = np.arange(3)
    while True:
        active &= (steps < max_steps) & ~(lam > LAMBDA_MAX)
        if not active.any():
            return X, steps
        steps[active] += 1
        D = H.copy()
        D[:, diag, diag] = H[:, diag, diag] + lam[:, None] * H[:, diag, diag]
        L, ok = cholesky3(D, 0.0)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            y = np.zeros_like(X)
            for j in range(3):
                y[:, j] = (-g[:, j] - np.sum(L[:, j, :j] * y[:, :j], axis=1)) / L[:, j, j]
            d = np.zeros_like(X)
            for j in range(2, -1, -1):
                d[:, j] = (y[:, j] - np.sum(L[:, j + 1:, j] * d[:, j + 1:], axis=1)) / L[:, j, j]
        solved = active & ok & np.all(np.isfinite(d), axis=1)
        lam = np.where(active & ~solved, lam * 10.0, lam)
        small = solved & (np.linalg.norm(d, axis=1) <= MIN_STEP * (1.0 + np.linalg.norm(X, axis=1)))
        active &= ~small
        trial = solved & ~small
        if not trial.any():
            continue
        Ft, Ht, gt = point_system(np.where(trial[:, None], X + d, X), R, t, K, uv)
        acc = trial & np.isfinite(Ft) & (Ft < F)
        with np.errstate(invalid="ignore"):
            done = acc & (F - Ft < MIN_DECREASE * F)
        X[acc] += d[acc]
        F = np.where(acc, Ft, F)
        H[acc], g[acc] = Ht[acc], gt[acc]
        lam = np.where(acc, lam / 10.0, np.where(trial, lam * 10.0, lam))
        active &= ~done


def rays(R, t, X):
    """Unit vectors from the camera centres -R^T t to X: R (n, k, 3, 3), t (n, k, 3), X (n, 3) -> (n, k, 3)."""
    centre = -np.einsum("nkji,nkj->nki", R, t)
    d = X[:, None, :] - centre
    with np.errstate(invalid="ignore", divide="ignore"):
        return d / np.linalg.norm(d, axis=2, keepdims=True)


def dlt_rows(P, uv):
    """The reference's two DLT rows per observation (y P3 - P2, P1 - x P3): P (n, k, 3, 4), uv (n, k, 2) -> (n, 2k, 4)."""
    a = uv[..., 1:2] * P[..., 2, :] - P[..., 1, :]
    b = P[..., 0, :] - uv[..., 0:1] * P[..., 2, :]
    return np.stack([a, b], axis=2).reshape(P.shape[0], -1, 4)


def triangulate(K, poses, cam, pt, uv, num_points, min_views=2, min_angle=0.0, max_error=np.inf, refine_steps=0):
    """-> dict(points (P, 3), status (P,) uint8, obs_error (M,), angle (P,) radians, info dict(status, points_ok,
    max_refine_steps_taken)).  min_angle in radians, max_error in px^2."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    Pn, M = int(num_points), len(cam)
    points = np.full((Pn, 3), np.nan)
    status = np.zeros(Pn, dtype=np.uint8)
    obs_error = np.full(M, np.nan)
    angle = np.full(Pn, np.nan)
    info = dict(status=0, points_ok=0, max_refine_steps_taken=0)
    out = dict(points=points, status=status, obs_error=obs_error, angle=angle, info=info)
    if M and (cam.min() < 0 or cam.max() >= len(poses) or pt.min() < 0 or pt.max() >= Pn):
        status[:] = BAD_INDEX
        info["status"] = 1
        return out
    order = np.lexsort((np.arange(M), pt))          # point-major, each run in observation order
    counts = np.bincount(pt, minlength=Pn)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    status[counts < min_views] = FEW_VIEWS
    Rall = poses[:, :9].reshape(-1, 3, 3)
    tall = poses[:, 9:]
    Pall = np.einsum("ij,cjk->cik", K, np.concatenate([Rall, tall[:, :, None]], axis=2))
    for k in np.unique(counts[counts >= min_views]):
        ps = np.nonzero(counts == k)[0]
        obs = order[starts[ps][:, None] + np.arange(k)[None, :]]          # (n, k)
        c, q = cam[obs], uv[obs]
        A = dlt_rows(Pall[c], q)
        finite = np.all(np.isfinite(A), axis=(1, 2))
        A[~finite] = 0.0
        v = np.linalg.svd(A)[2][:, -1, :]
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
        one_camera = np.all(c == c[:, :1], axis=1)   # the rays meet at that camera's centre: no point, whatever the pixels
        degenerate = one_camera | ~finite | ~np.all(np.isfinite(v), axis=1) | ~(np.abs(v[:, 3]) > MIN_W)
        status[ps[degenerate]] = DEGENERATE
        good = ~degenerate
        ps, obs, c, q, v = ps[good], obs[good], c[good], q[good], v[good]
        if len(ps) == 0:
            continue
        X = v[:, :3] / v[:, 3:4]
        R, t = Rall[c], tall[c]
        if refine_steps > 0:
            X, steps = refine(X, R, t, K, q, refine_steps)
            info["max_refine_steps_taken"] = max(info["max_refine_steps_taken"], int(steps.max()))
        e, cc = score(R, t, K, X[:, None, :], q)
        obs_error[obs] = e
        front = np.all(cc[..., 2] > 0.0, axis=1)
        d = rays(R, t, X)
        G = np.einsum("nid,njd->nij", d, d)
        iu = np.triu_indices(k, 1)
        min_cos = np.min(G[:, iu[0], iu[1]], axis=1)
        ang = np.arccos(np.clip(min_cos, -1.0, 1.0))
        st = np.full(len(ps), OK, dtype=np.uint8)
        st[~front] = BEHIND
        st[front & (ang < min_angle)] = SMALL_ANGLE
        st[front & ~(ang < min_angle) & (np.max(e, axis=1) > max_error)] = LARGE_ERROR
        status[ps], points[ps], angle[ps] = st, X, ang
    info["points_ok"] = int(np.count_nonzero(status == OK))
    return out


def triangulate_pair_dlt(K, pose_a, pose_b, xa, xb):
    """The two-view DLT of one correspondence under two arbitrary poses (the rows of the reference's triangulate_dlt)."""
    P = np.stack([K @ np.hstack([p[:9].reshape(3, 3), p[9:, None]]) for p in (pose_a, pose_b)])[None]
    v = np.linalg.svd(dlt_rows(P, np.stack([xa, xb])[None]))[2][0, -1]
    return v[:3] / v[3]
