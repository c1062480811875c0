"""Irregular observation graphs for bundle adjustment and track triangulation: the geometry of
``synthetic.bundle_problem`` (points x, y in [-1, 1], z in [4, 6], in front of every camera; camera 0 = [I | 0]) with each
point's camera set drawn directly, so that the graph's structure can be chosen:

- track lengths: ``singles`` points seen once, ``pairs`` seen twice, ``full`` seen by ``full_length`` cameras (default:
  every camera that is not sparse), ``unobserved`` points seen by none, and every other point seen by a uniform
  ``mid[0] .. mid[1]`` cameras (capped at the cameras available);
- ``duplicates`` repeated (camera, point) pairs, each with its own pixel noise, on distinct observations of points seen
  by at least two distinct cameras and never of a sparse camera;
- ``one_camera`` points seen twice by one camera (a single observation and its duplicate): moving points (two
  observations) whose V_p has rank 2;
- ``sparse`` = {camera: n}: that camera sees exactly n points, drawn among the points seen by at least two other cameras;
- ``order`` of the observations: "random", "camera-major" (by camera, then point), "point-major" (by point, then camera)
  or "reversed" (camera-major backwards).  Ties (a duplicate and its original) keep the order they were drawn in.

Point kinds are laid out in index order (unobserved, singles, one-camera, pairs, full, the rest) and then shuffled, so no
kind sits in one index range.  Memory and time are O(observations): C = 70 000 cameras or P = 4.2 M points are cheap.
Returns the dict of ``synthetic.bundle_problem``."""
import numpy as np

from structure_from_motion_amd import synthetic

ORDERS = ("random", "camera-major", "point-major", "reversed")


def _distinct_cameras(rng, pool, n, k):
    """(n, k) int64: each row k distinct entries of ``pool``."""
    pool = np.asarray(pool, dtype=np.int64)
    if k == 0 or n == 0:
        return np.zeros((n, k), dtype=np.int64)
    if k == len(pool):
        return np.broadcast_to(pool, (n, k)).copy()
    if len(pool) <= 64 or 4 * k > len(pool):   # a random key per (row, camera) and the k smallest
        out = np.empty((n, k), dtype=np.int64)
        for s in range(0, n, 1 << 18):   # row chunks keep the (rows, pool) keys small
            e = min(n, s + (1 << 18))
            out[s:e] = pool[np.argsort(rng.random((e - s, len(pool))), axis=1)[:, :k]]
        return out
    idx = rng.integers(0, len(pool), (n, k))
    while True:   # redraw the rows that repeat a camera (rare here: k << len(pool))
        srt = np.sort(idx, axis=1)
        bad = np.nonzero(np.any(srt[:, 1:] == srt[:, :-1], axis=1))[0]
        if len(bad) == 0:
            return pool[idx]
        idx[bad] = rng.integers(0, len(pool), (len(bad), k))


def irregular_problem(cameras, points, seed=0, singles=0, pairs=0, full=0, full_length=None, unobserved=0, mid=(3, 6),
                      duplicates=0, one_camera=0, sparse=None, order="random", noise_px=0.5, rotation_noise=0.003,
                      translation_noise=0.01, point_noise=0.01, K=synthetic.BENCH_K):
    assert order in ORDERS, order
    sparse = dict(sparse or {})
    C, P = int(cameras), int(points)
    rest = P - (unobserved + singles + one_camera + pairs + full)
    assert rest >= 0, "more points of given kinds than points"
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-1.0, 1.0, P), rng.uniform(-1.0, 1.0, P), rng.uniform(4.0, 6.0, P)])
    poses = np.zeros((C, 12))
    poses[0, :9] = np.eye(3).reshape(9)
    if C > 1:
        ax, ay = rng.uniform(-5.0, 5.0, C - 1), rng.uniform(-10.0, 10.0, C - 1)
        for c in range(1, C):
            poses[c, :9] = synthetic.rotation_xy(ax[c - 1], ay[c - 1]).reshape(9)
        poses[1:, 9:] = np.column_stack([rng.uniform(-0.5, 0.5, C - 1), rng.uniform(-0.2, 0.2, C - 1),
                                         rng.uniform(-0.2, 0.2, C - 1)])
    pool = np.setdiff1d(np.arange(C), np.array(sorted(sparse), dtype=np.int64))
    flen = len(pool) if full_length is None else int(full_length)
    lo, hi = min(mid[0], len(pool)), min(mid[1], len(pool))
    # point kinds in index order, then a shuffle of the point indices
    kind_len = np.concatenate([np.zeros(unobserved, dtype=np.int64), np.ones(singles + one_camera, dtype=np.int64),
                               np.full(pairs, 2, dtype=np.int64), np.full(full, flen, dtype=np.int64),
                               rng.integers(lo, hi + 1, rest)])
    one_cam = np.zeros(P, dtype=bool)
    one_cam[unobserved + singles:unobserved + singles + one_camera] = True
    perm = rng.permutation(P)
    length = np.empty(P, dtype=np.int64)
    length[perm] = kind_len
    one_cam_pt = np.zeros(P, dtype=bool)
    one_cam_pt[perm] = one_cam
    cams, pts = [], []
    for k in np.unique(length):
        if k == 0:
            continue
        who = np.nonzero(length == k)[0]
        cams.append(_distinct_cameras(rng, pool, len(who), int(k)).reshape(-1))
        pts.append(np.repeat(who, k))
    cam = np.concatenate(cams) if cams else np.zeros(0, dtype=np.int64)
    pt = np.concatenate(pts) if pts else np.zeros(0, dtype=np.int64)
    # sparse cameras: each on n points seen by at least two distinct (non-sparse) cameras
    multi = np.nonzero(length >= 2)[0]
    for c, n in sorted(sparse.items()):
        assert n <= len(multi), "a sparse camera asks for more points than have two observations"
        cam = np.concatenate([cam, np.full(n, c, dtype=np.int64)])
        pt = np.concatenate([pt, rng.choice(multi, n, replace=False)])
    # duplicates: distinct observations of multi-camera points by non-sparse cameras, plus one per one-camera point
    eligible = np.nonzero((length[pt] >= 2) & np.isin(cam, pool))[0]
    assert duplicates <= len(eligible), "more duplicates than eligible observations"
    dup = np.concatenate([rng.choice(eligible, duplicates, replace=False), np.nonzero(one_cam_pt[pt])[0]])
    cam = np.concatenate([cam, cam[dup]])
    pt = np.concatenate([pt, pt[dup]])
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X[pt]) + poses[cam, 9:]
    uvw = xc @ K.T
    pixels = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (len(cam), 2))
    # the order of the observations (the same draws in every order: one seed is one graph)
    o = rng.permutation(len(cam))
    if order == "point-major":
        o = np.lexsort((cam, pt))
    elif order != "random":
        o = np.lexsort((pt, cam))
        if order == "reversed":
            o = o[::-1]
    cam, pt, pixels = cam[o], pt[o], pixels[o]
    start = poses.copy()
    for c in range(1, C):
        start[c, :9] = (synthetic._small_rotation(rng, rotation_noise) @ poses[c, :9].reshape(3, 3)).reshape(9)
    if C > 1:
        start[1:, 9:] += rng.normal(0.0, translation_noise, (C - 1, 3))
    return dict(K=K, poses=start, points=X + rng.normal(0.0, point_noise, X.shape), camera_indices=cam.astype(np.int32),
                point_indices=pt.astype(np.int32), pixels=pixels, poses_true=poses, points_true=X)


def mixed(cameras, points, seed, order="random", full=True, sparse_camera=None, sparse_count=10, **kw):
    """The mixed graph of the parity tests: 8 % singles, 2 % unobserved, 20 % pairs, a few full-length tracks (when
    ``full``), 2 % duplicates and one free camera (the last by default) with ``sparse_count`` observations."""
    c = cameras - 1 if sparse_camera is None else sparse_camera
    args = dict(singles=points * 8 // 100, unobserved=points // 50, pairs=points // 5, full=4 if full else 0,
                sparse={c: sparse_count})
    args.update(kw)
    pr = irregular_problem(cameras, points, seed, order=order, **args)
    if "duplicates" not in kw:   # 2 % of the observations, drawn again with the count known
        args["duplicates"] = len(pr["camera_indices"]) // 50
        pr = irregular_problem(cameras, points, seed, order=order, **args)
    return pr


def corrupt_long_tracks(problem, fraction, spread_px, seed, min_cameras=3):
    """The problem with ``int(fraction * M)`` gross errors placed where a parity input can bear them -> (new dict, (M,) bool
    mask).  That many distinct points are picked among those seen by at least ``min_cameras`` distinct cameras, and one
    observation of each is shifted by uniform +-``spread_px`` in u and in v.  A point that owns a corrupted observation and
    has only one other view is barely held, and the reference's own result then depends on the summation order (DESIGN.md
    §6n): ``synthetic.corrupt_observations`` draws per observation and cannot avoid that on an irregular graph.

    The choice is made on the observations sorted by (point, camera, u, v), so it does not depend on the order of the
    observation arrays: the four ``order``s of one seed carry the same multiset of (camera, point, pixel)."""
    cam = np.asarray(problem["camera_indices"], dtype=np.int64)
    pt = np.asarray(problem["point_indices"], dtype=np.int64)
    uv = np.asarray(problem["pixels"], dtype=np.float64)
    M, P = len(cam), len(problem["points"])
    canon = np.lexsort((uv[:, 1], uv[:, 0], cam, pt))   # position in the canonical order -> observation
    first = np.searchsorted(pt[canon], np.arange(P + 1))   # canonical range of every point
    pairs = np.unique(np.column_stack([pt, cam]), axis=0)
    distinct = np.bincount(pairs[:, 0], minlength=P)
    eligible = np.nonzero(distinct >= min_cameras)[0]
    n = int(fraction * M)
    assert n <= len(eligible), f"{n} points wanted, {len(eligible)} seen by at least {min_cameras} cameras"
    rng = np.random.default_rng(seed)
    picked = np.sort(rng.choice(eligible, n, replace=False))
    which = first[picked] + rng.integers(0, first[picked + 1] - first[picked])   # one observation of each, canonical
    shift = rng.uniform(-spread_px, spread_px, (n, 2))
    pixels = uv.copy()
    pixels[canon[which]] += shift
    mask = np.zeros(M, dtype=bool)
    mask[canon[which]] = True
    return dict(problem, pixels=pixels), mask
