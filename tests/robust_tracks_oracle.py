"""NumPy definition of the outlier-robust triangulation of multi-view tracks (csrc/sfm_tracks_robust.hip,
sfm_triangulate_tracks_robust): per-track RANSAC over two-view hypotheses from pairs of a track's
observations, MSAC scoring over the track, a refit on the winner's inliers and an inlier flag per observation.  Built on
tests/tracks_oracle.py (``score``, ``dlt_rows``, ``rays``, ``refine``), one point at a time; only the summation order inside
the LM and the SVD route differ from the device.

Besides the outputs of the device, ``triangulate`` returns ``clear`` (P,) bool: False where a decision of the point sits so
close to its limit that rounding may legitimately turn it on the device (``CLEAR_REL``, ``CLEAR_ANGLE``):
  * an |e - max_error| <= 1e-9 max_error at a scored hypothesis or at the final X;
  * a hypothesis' pair angle, or the final angle, within 1e-9 rad of min_angle;
  * a hypothesis with another inlier set that has the winner's n and a c within 1e-9 relative of the winner's.
"""
import math

import numpy as np

import tracks_oracle as to

OK, FEW_VIEWS, DEGENERATE, BEHIND, SMALL_ANGLE, LARGE_ERROR, BAD_INDEX, NO_CONSENSUS = range(8)
MIN_W = to.MIN_W
MAX_HYPOTHESES = 1024
CLEAR_REL = 1e-9
CLEAR_ANGLE = 1e-9


def hypothesis_ranks(k, max_hypotheses):
    """The ranks r_0 < r_1 < ... of the hypotheses of a track of k observations among its T = k (k - 1) / 2 pairs (Python
    integers: exact at any size)."""
    T = k * (k - 1) // 2
    if T <= max_hypotheses:
        return list(range(T))
    step, extra = divmod(T, max_hypotheses)
    return [h * step + min(h, extra) for h in range(max_hypotheses)]


def unrank_pair(r, k):
    """The pair (i, j), i < j < k, of rank r in lexicographic order: row i starts at i (2k - i - 1) / 2."""
    b = 2 * k - 1
    i = (b - math.isqrt(b * b - 8 * r)) // 2
    while i > 0 and i * (2 * k - i - 1) // 2 > r:
        i -= 1
    while (i + 1) * (2 * k - i - 2) // 2 <= r:
        i += 1
    return i, r - i * (2 * k - i - 1) // 2 + i + 1


def _null_vector(A):
    """Unit null vector of the stacked rows A (2n, 4), or None when A or the vector is not finite or |v3| <= MIN_W."""
    if not np.all(np.isfinite(A)):
        return None
    v = np.linalg.svd(A)[2][-1]
    v = v / np.linalg.norm(v)
    if not np.all(np.isfinite(v)) or not abs(v[3]) > MIN_W:
        return None
    return v


def _errors(R, t, K, X, uv):
    """(e (k,), c (k, 3)) of one point X over its observations."""
    e, c = to.score(R, t, K, X[None, :], uv)
    return e, c


def _angle(cosine):
    return float(np.arccos(min(1.0, max(-1.0, cosine))))


def _near(e, max_error):
    with np.errstate(invalid="ignore"):
        return bool(np.any(np.abs(e - max_error) <= CLEAR_REL * max_error))


def _msac(e, max_error):
    """(n, c, inlier (k,)): c summed in run order, one add per observation."""
    with np.errstate(invalid="ignore"):
        inlier = e <= max_error
    c = 0.0
    for value, flag in zip(e.tolist(), inlier.tolist()):
        c += value if flag else max_error
    return int(inlier.sum()), c, inlier


def triangulate_point(K, Pall, Rall, tall, c, q, min_views, min_angle, max_error, refine_steps, max_hypotheses, reverse=False):
    """One track: camera indices c (k,), pixels q (k, 2) in run order.  -> dict(status, step (the step of the definition that
    set the status: 0, 3, 4 or 5), X, e, inlier, angle, steps, hypotheses, clear).  ``reverse`` feeds the rows of every DLT and the LM's sums in reverse run order (the spread of the
    definition against itself; the hypotheses, their order and the MSAC sum stay)."""
    k = len(c)
    out = dict(status=OK, X=np.full(3, np.nan), e=np.full(k, np.nan), inlier=np.zeros(k, bool), angle=np.nan, steps=0,
               hypotheses=0, clear=True, step=0)
    if k < min_views:
        out["status"] = FEW_VIEWS
        return out
    if np.all(c == c[0]):
        out["status"] = DEGENERATE
        return out
    R, t = Rall[c], tall[c]
    best = None   # (n, c, h, X, inlier)
    scored = []
    for h, r in enumerate(hypothesis_ranks(k, max_hypotheses)):
        i, j = unrank_pair(r, k)
        if c[i] == c[j]:
            continue
        pair = [j, i] if reverse else [i, j]
        v = _null_vector(to.dlt_rows(Pall[c[pair]][None], q[pair][None])[0])
        if v is None:
            continue
        X = v[:3] / v[3]
        e, cc = _errors(R, t, K, X, q)
        if not (cc[i, 2] > 0.0 and cc[j, 2] > 0.0):
            continue
        d = to.rays(R[[i, j]][None], t[[i, j]][None], X[None])[0]
        angle = _angle(float(np.dot(d[0], d[1])))
        if abs(angle - min_angle) <= CLEAR_ANGLE:
            out["clear"] = False
        if not angle >= min_angle:
            continue
        out["hypotheses"] += 1
        if _near(e, max_error):
            out["clear"] = False
        n, cost, inlier = _msac(e, max_error)
        scored.append((n, cost, inlier))
        if best is None or n > best[0] or (n == best[0] and cost < best[1]):
            best = (n, cost, h, X, inlier)
    if best is None or best[0] < min_views:
        out.update(status=NO_CONSENSUS, step=3)
        return out
    for n, cost, inlier in scored:
        if n == best[0] and not np.array_equal(inlier, best[4]) and abs(cost - best[1]) <= CLEAR_REL * abs(best[1]):
            out["clear"] = False
    S = np.nonzero(best[4])[0]
    if np.all(c[S] == c[S[0]]):
        out.update(status=NO_CONSENSUS, step=4)
        return out
    rows = S[::-1] if reverse else S
    v = _null_vector(to.dlt_rows(Pall[c[rows]][None], q[rows][None])[0])
    if v is None:
        out.update(status=DEGENERATE, step=4)
        return out
    X = v[:3] / v[3]
    if refine_steps > 0:
        Xr, steps = to.refine(X[None], R[rows][None], t[rows][None], K, q[rows][None], refine_steps)
        X, out["steps"] = Xr[0], int(steps[0])
    e, _ = _errors(R, t, K, X, q)
    if _near(e, max_error):
        out["clear"] = False
    with np.errstate(invalid="ignore"):
        inlier = e <= max_error
    F = np.nonzero(inlier)[0]
    if len(F) < min_views or np.all(c[F] == c[F[0]]):
        out.update(status=NO_CONSENSUS, step=5)
        return out
    d = to.rays(R[F][None], t[F][None], X[None])[0]
    G = d @ d.T
    iu = np.triu_indices(len(F), 1)
    angle = _angle(float(np.min(G[iu])))
    if abs(angle - min_angle) <= CLEAR_ANGLE:
        out["clear"] = False
    out.update(status=SMALL_ANGLE if angle < min_angle else OK, step=5, X=X, e=e, inlier=inlier, angle=angle)
    return out


def triangulate(K, poses, cam, pt, uv, num_points, max_error, min_views=2, min_angle=0.0, refine_steps=0, max_hypotheses=64,
                reverse=False):
    """-> dict(points (P, 3), status (P,) uint8, obs_error (M,), inlier (M,) uint8, angle (P,) radians, clear (P,) bool, step
    (P,) the step of the definition that set each status, info
    dict(status, points_ok, max_refine_steps_taken, inlier_observations, hypotheses, reserved)).  min_angle in radians,
    max_error in px^2, finite and >= 0."""
    if not (np.isfinite(max_error) and max_error >= 0.0):
        raise ValueError("max_error must be finite and >= 0")
    if isinstance(max_hypotheses, bool) or not 1 <= max_hypotheses <= MAX_HYPOTHESES:
        raise ValueError("max_hypotheses must be in 1 .. 1024")
    if min_views < 2 or refine_steps < 0 or not (np.isfinite(min_angle) and min_angle >= 0.0):
        raise ValueError("min_views >= 2, refine_steps >= 0 and a finite min_angle >= 0")
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    Pn, M = int(num_points), len(cam)
    points = np.full((Pn, 3), np.nan)
    status = np.zeros(Pn, dtype=np.uint8)
    obs_error = np.full(M, np.nan)
    inlier = np.zeros(M, dtype=np.uint8)
    angle = np.full(Pn, np.nan)
    clear = np.ones(Pn, dtype=bool)
    step = np.zeros(Pn, dtype=np.int64)
    info = dict(status=0, points_ok=0, max_refine_steps_taken=0, inlier_observations=0, hypotheses=0, reserved=0)
    out = dict(points=points, status=status, obs_error=obs_error, inlier=inlier, angle=angle, clear=clear, step=step, info=info)
    if M and (cam.min() < 0 or cam.max() >= len(poses) or pt.min() < 0 or pt.max() >= Pn):
        status[:] = BAD_INDEX
        info["status"] = 1
        return out
    order = np.lexsort((np.arange(M), pt))          # point-major, each run in observation order
    counts = np.bincount(pt, minlength=Pn)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    Rall = poses[:, :9].reshape(-1, 3, 3)
    tall = poses[:, 9:]
    Pall = np.einsum("ij,cjk->cik", K, np.concatenate([Rall, tall[:, :, None]], axis=2))
    for p in range(Pn):
        obs = order[starts[p]:starts[p] + counts[p]]
        r = triangulate_point(K, Pall, Rall, tall, cam[obs], uv[obs], min_views, min_angle, max_error, refine_steps,
                              max_hypotheses, reverse)
        status[p], clear[p], step[p] = r["status"], r["clear"], r["step"]
        info["hypotheses"] += r["hypotheses"]
        info["max_refine_steps_taken"] = max(info["max_refine_steps_taken"], r["steps"])
        if r["status"] in (OK, SMALL_ANGLE):
            points[p], angle[p] = r["X"], r["angle"]
            obs_error[obs], inlier[obs] = r["e"], r["inlier"]
        if r["status"] == OK:
            info["inlier_observations"] += int(r["inlier"].sum())
    info["points_ok"] = int(np.count_nonzero(status == OK))
    return out


def plain_threshold_inliers(K, poses, cam, pt, uv, num_points, max_error, second_attempt=False):
    """What thresholding the plain N-view DLT's errors calls the inliers (M,) bool; ``second_attempt`` drops the observations
    above the threshold and triangulates the rest once more (the repair of apps/sfm_multi_view.py)."""
    cam, pt, uv = np.asarray(cam), np.asarray(pt), np.asarray(uv, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = to.triangulate(K, poses, cam, pt, uv, num_points)["obs_error"] <= max_error
    if second_attempt and keep.any():
        again = to.triangulate(K, poses, cam[keep], pt[keep], uv[keep], num_points)["obs_error"]
        inner = np.zeros(len(cam), dtype=bool)
        with np.errstate(invalid="ignore"):
            inner[np.nonzero(keep)[0]] = again <= max_error
        keep = inner
    return keep
