"""Deterministic synthetic two-view correspondence sets (bench / demo inputs).

Host-side input generation only — nothing here is on the timed path.
"""
from __future__ import annotations

import numpy as np

BENCH_K = np.array([[1520.4, 0.0, 302.32], [0.0, 1525.9, 246.87], [0.0, 0.0, 1.0]])


def rotation_xy(deg_x: float, deg_y: float) -> np.ndarray:
    """Intrinsic rotation about X then Y (``Rotation.from_euler("XY", ...)``): Rx @ Ry."""
    ax, ay = np.radians(deg_x), np.radians(deg_y)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return rx @ ry


def two_view_scene(n: int, seed: int = 6, outlier_fraction: float = 0.3, noise_px: float = 0.5,
                   K: np.ndarray = BENCH_K):
    """Points uniform in x,y in [-1,1], z in [4,6]; camera 1 = [I|0]; camera 2 = euler XY (-5, -10) deg,
    t = (0.5, 0.05, 0.1); Gaussian pixel noise on every projection; a fraction of image-2 points replaced
    by uniform random pixels.  Returns (pix_a (n,2), pix_b (n,2), K, R, t, is_outlier)."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, 3))
    X[:, 0] = rng.uniform(-1.0, 1.0, n)
    X[:, 1] = rng.uniform(-1.0, 1.0, n)
    X[:, 2] = rng.uniform(4.0, 6.0, n)
    R = rotation_xy(-5.0, -10.0)
    t = np.array([0.5, 0.05, 0.1])

    def project(Xc):
        uvw = Xc @ K.T
        return uvw[:, :2] / uvw[:, 2:3]

    pa = project(X) + rng.normal(0.0, noise_px, (n, 2))
    pb = project(X @ R.T + t) + rng.normal(0.0, noise_px, (n, 2))
    is_out = rng.random(n) < outlier_fraction
    width, height = 2.0 * K[0, 2], 2.0 * K[1, 2]
    rand_px = np.column_stack([rng.uniform(0, width, n), rng.uniform(0, height, n)])
    pb = np.where(is_out[:, None], rand_px, pb)
    return pa, pb, K, R, t, is_out


def _small_rotation(rng, sigma: float) -> np.ndarray:
    """exp([w]x) for w ~ N(0, sigma^2 I) (Rodrigues)."""
    w = rng.normal(0.0, sigma, 3)
    th = float(np.linalg.norm(w))
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * W + (1.0 - np.cos(th)) / th**2 * (W @ W)


def bundle_problem(cameras: int, points: int, per_point: int = 4, seed: int = 0, noise_px: float = 0.5,
                   rotation_noise: float = 0.003, translation_noise: float = 0.01, point_noise: float = 0.01,
                   K: np.ndarray = BENCH_K):
    """A bundle-adjustment input: points uniform in x, y in [-1, 1], z in [4, 6]; camera 0 = [I | 0], the others rotated by
    up to 5 / 10 degrees about X / Y and shifted by up to 0.5 in x, 0.2 in y and z.  Each point is seen by
    min(per_point, cameras) distinct cameras, with Gaussian pixel noise; the observations come in random order.  The start
    perturbs every camera but camera 0 (rotation and translation) and every point.  Returns dict(K, poses (C, 12), points
    (P, 3), camera_indices, point_indices (M,), pixels (M, 2), poses_true, points_true)."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-1.0, 1.0, points), rng.uniform(-1.0, 1.0, points), rng.uniform(4.0, 6.0, points)])
    poses = np.zeros((cameras, 12))
    poses[0, :9] = np.eye(3).reshape(9)
    for c in range(1, cameras):
        poses[c, :9] = rotation_xy(rng.uniform(-5.0, 5.0), rng.uniform(-10.0, 10.0)).reshape(9)
        poses[c, 9:] = [rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)]
    k = min(per_point, cameras)
    cam = np.argsort(rng.random((points, cameras)), axis=1)[:, :k].reshape(-1)
    pt = np.repeat(np.arange(points), k)
    order = rng.permutation(len(cam))
    cam, pt = cam[order], pt[order]
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X[pt]) + poses[cam, 9:]
    uvw = xc @ K.T
    pixels = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (len(cam), 2))
    start = poses.copy()
    for c in range(1, cameras):
        start[c, :9] = (_small_rotation(rng, rotation_noise) @ poses[c, :9].reshape(3, 3)).reshape(9)
        start[c, 9:] += rng.normal(0.0, translation_noise, 3)
    return dict(K=K, poses=start, points=X + rng.normal(0.0, point_noise, X.shape), camera_indices=cam.astype(np.int32),
                point_indices=pt.astype(np.int32), pixels=pixels, poses_true=poses, points_true=X)


def sequence_bundle_problem(cameras: int, points: int, track_length: int = 4, seed: int = 0, noise_px: float = 0.5,
                            spacing: float = 0.2, rotation_noise: float = 0.003, translation_noise: float = 0.01,
                            point_noise: float = 0.01, K: np.ndarray = BENCH_K):
    """A bundle-adjustment input shaped like a video sequence: camera i has its centre at (i * spacing, 0, 0) and is
    rotated by up to 1 degree about X and Y (camera 0 = [I | 0]).  Each point is seen by a contiguous window of
    ``min(track_length, cameras)`` neighbouring cameras (the window's first camera uniform), so camera visibility is
    banded: cameras share points only with neighbours less than ``track_length`` apart.  A point lies in x within 0.55 of
    every centre of its window, y in [-0.5, 0.5] and z in [4, 6]; pixels carry Gaussian noise and the observations come in
    random order.  The start perturbs every camera but camera 0 (its rotation about its own centre, and its translation)
    and every point as ``bundle_problem`` does.  Memory is O(observations).  Returns the dict of ``bundle_problem``."""
    rng = np.random.default_rng(seed)
    L = min(track_length, cameras)
    poses = np.zeros((cameras, 12))
    poses[0, :9] = np.eye(3).reshape(9)
    for c in range(1, cameras):
        R = rotation_xy(rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0))
        poses[c, :9] = R.reshape(9)
        poses[c, 9:] = -R @ np.array([c * spacing, 0.0, 0.0])
    first = rng.integers(0, cameras - L + 1, points)
    lo = (first + L - 1) * spacing - 0.55
    hi = first * spacing + 0.55
    X = np.column_stack([rng.uniform(lo, hi), rng.uniform(-0.5, 0.5, points), rng.uniform(4.0, 6.0, points)])
    cam = (first[:, None] + np.arange(L)[None, :]).reshape(-1)
    pt = np.repeat(np.arange(points), L)
    order = rng.permutation(len(cam))
    cam, pt = cam[order], pt[order]
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X[pt]) + poses[cam, 9:]
    uvw = xc @ K.T
    pixels = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (len(cam), 2))
    start = poses.copy()
    for c in range(1, cameras):   # rotated about the camera's own centre, which then moves by the translation noise
        R = _small_rotation(rng, rotation_noise) @ poses[c, :9].reshape(3, 3)
        start[c, :9] = R.reshape(9)
        start[c, 9:] = -R @ np.array([c * spacing, 0.0, 0.0]) + rng.normal(0.0, translation_noise, 3)
    return dict(K=K, poses=start, points=X + rng.normal(0.0, point_noise, X.shape), camera_indices=cam.astype(np.int32),
                point_indices=pt.astype(np.int32), pixels=pixels, poses_true=poses, points_true=X)


def corrupt_observations(problem, fraction: float, spread_px: float, seed: int):
    """``problem`` (the dict of ``bundle_problem``) with wrong observations: every observation is picked with probability
    ``fraction`` and its pixel shifted by uniform +-``spread_px`` in u and in v.  Returns (a new dict with its own
    ``pixels``, the boolean mask (M,) of the shifted observations)."""
    rng = np.random.default_rng(seed)
    pixels = np.array(problem["pixels"], dtype=np.float64)
    bad = rng.random(len(pixels)) < fraction
    pixels[bad] += rng.uniform(-spread_px, spread_px, (int(bad.sum()), 2))
    return dict(problem, pixels=pixels), bad


def multi_view_scene(views: int = 8, points: int = 2000, seed: int = 21, noise_px: float = 0.5,
                     outlier_fraction: float = 0.2, step_deg: float = 5.0, K: np.ndarray = BENCH_K):
    """An N-view scene for incremental reconstruction: points uniform in x, y in [-1, 1], z in [4, 6]; camera 0 = [I | 0]
    and camera i on an arc about the box centre (0, 0, 5), ``i * step_deg`` degrees about the Y axis, looking at it.  A point
    is observed by every camera in front of which it projects inside the image (2 cx by 2 cy), with Gaussian pixel noise;
    only points observed at least twice are kept, so tracks have lengths 2 to ``views``.  A fraction of the observations
    is replaced by uniform random pixels.  The observations come camera-major, by point inside a camera.  Returns
    dict(K, camera_indices, point_indices (M,) int32, pixels (M, 2), is_outlier (M,) bool, poses_true (V, 12),
    points_true (P, 3))."""
    rng = np.random.default_rng(seed)
    width, height = 2.0 * K[0, 2], 2.0 * K[1, 2]
    poses = np.zeros((views, 12))
    for i in range(views):
        a = np.radians(i * step_deg)
        R = np.array([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
        centre = np.array([-5.0 * np.sin(a), 0.0, 5.0 - 5.0 * np.cos(a)])
        poses[i, :9] = R.reshape(9)
        poses[i, 9:] = -R @ centre
    poses[0] = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    kept = []
    while sum(len(x) for x in kept) < points:
        X = np.column_stack([rng.uniform(-1.0, 1.0, points), rng.uniform(-1.0, 1.0, points), rng.uniform(4.0, 6.0, points)])
        seen = np.zeros((points, views), dtype=bool)
        for i in range(views):
            xc = X @ poses[i, :9].reshape(3, 3).T + poses[i, 9:]
            uvw = xc @ K.T
            uv = uvw[:, :2] / uvw[:, 2:3]
            seen[:, i] = (xc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < width) & (uv[:, 1] >= 0) & (uv[:, 1] < height)
        kept.append(X[seen.sum(axis=1) >= 2])
    X = np.vstack(kept)[:points]
    cams, pts, pixels = [], [], []
    for i in range(views):
        xc = X @ poses[i, :9].reshape(3, 3).T + poses[i, 9:]
        uvw = xc @ K.T
        uv = uvw[:, :2] / uvw[:, 2:3]
        vis = np.nonzero((xc[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < width) & (uv[:, 1] >= 0) & (uv[:, 1] < height))[0]
        cams.append(np.full(len(vis), i))
        pts.append(vis)
        pixels.append(uv[vis] + rng.normal(0.0, noise_px, (len(vis), 2)))
    cam, pt, pix = np.concatenate(cams), np.concatenate(pts), np.vstack(pixels)
    is_out = rng.random(len(cam)) < outlier_fraction
    rand_px = np.column_stack([rng.uniform(0, width, len(cam)), rng.uniform(0, height, len(cam))])
    pix = np.where(is_out[:, None], rand_px, pix)
    return dict(K=K, camera_indices=cam.astype(np.int32), point_indices=pt.astype(np.int32), pixels=pix, is_outlier=is_out,
                poses_true=poses, points_true=X)


def planar_pnp_scene(n: int, seed: int = 0, K: np.ndarray = BENCH_K, outlier_fraction: float = 0.3, noise_px: float = 0.5):
    """A PnP input whose 3-D points all lie on one plane, z = 5 + 0.3 x (x, y uniform in [-1, 1]): a wall, a floor or a
    calibration board, which the six-point DLT cannot register.  The view has a random pose (rotation of 0.05 to 0.4 rad
    about a random axis, t uniform in [-0.5, 0.5]^3), Gaussian pixel noise, and a fraction of pixels replaced by uniform
    random ones.  Returns (pts (n, 5) {X, Y, Z, u, v}, R, t, is_outlier)."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a *= rng.uniform(0.05, 0.4) / np.linalg.norm(a)
    th = float(np.linalg.norm(a))
    k = a / th
    W = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(th) * W + (1.0 - np.cos(th)) * (W @ W)
    t = rng.uniform(-0.5, 0.5, 3)
    x = rng.uniform(-1.0, 1.0, n)
    y = rng.uniform(-1.0, 1.0, n)
    X = np.column_stack([x, y, 5.0 + 0.3 * x])
    uvw = (X @ R.T + t) @ K.T
    uv = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (n, 2))
    is_out = rng.random(n) < outlier_fraction
    rand_px = np.column_stack([rng.uniform(0, 2 * K[0, 2], n), rng.uniform(0, 2 * K[1, 2], n)])
    uv = np.where(is_out[:, None], rand_px, uv)
    return np.column_stack([X, uv]), R, t, is_out


def planar_two_view_scene(n: int, seed: int = 0, outlier_fraction: float = 0.3, noise_px: float = 0.5,
                          K: np.ndarray = BENCH_K):
    """Two views of points on one plane, z = 5 + 0.3 x - 0.2 y (x, y uniform in [-1, 1]), which the eight-point algorithm
    cannot fit and the five-point solver can.  Camera 1 = [I|0]; camera 2 as in ``two_view_scene``; Gaussian pixel noise on
    every projection and a fraction of image-2 points replaced by uniform random pixels.  Returns (pix_a (n,2),
    pix_b (n,2), K, R, t, is_outlier, plane) with plane = (normal, d): normal . X = d for every point."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, n)
    y = rng.uniform(-1.0, 1.0, n)
    X = np.column_stack([x, y, 5.0 + 0.3 * x - 0.2 * y])
    R = rotation_xy(-5.0, -10.0)
    t = np.array([0.5, 0.05, 0.1])

    def project(Xc):
        uvw = Xc @ K.T
        return uvw[:, :2] / uvw[:, 2:3]

    pa = project(X) + rng.normal(0.0, noise_px, (n, 2))
    pb = project(X @ R.T + t) + rng.normal(0.0, noise_px, (n, 2))
    is_out = rng.random(n) < outlier_fraction
    width, height = 2.0 * K[0, 2], 2.0 * K[1, 2]
    rand_px = np.column_stack([rng.uniform(0, width, n), rng.uniform(0, height, n)])
    pb = np.where(is_out[:, None], rand_px, pb)
    normal = np.array([-0.3, 0.2, 1.0])
    return pa, pb, K, R, t, is_out, (normal, 5.0)


def pairwise_matches(scene, window: int = 3, wrong_fraction: float = 0.1, seed: int = 0):
    """Pairwise feature matches of a ``multi_view_scene``, the input of ``build_tracks``.  View v's features are its
    observations in a seeded random order (a local index says nothing about the point); the pairs are (i, j) with
    1 <= j - i <= ``window``; a pair's matches are every point both views observe, in random order, with ``wrong_fraction``
    of them re-paired to a random feature of view j.  The scene's random-pixel outliers stay: they are matched like any other
    observation.  Returns dict(features: list of (n_v, 2) pixels, pairs (Q, 2) int64, matches: list of (n_q, 2) int64 local
    indices, feature_points: list of (n_v,) int64 true point of each feature, wrong: list of (n_q,) bool)."""
    rng = np.random.default_rng(seed)
    cam, pt, uv = scene["camera_indices"], scene["point_indices"], scene["pixels"]
    views = int(cam.max()) + 1 if len(cam) else 0
    P = int(pt.max()) + 1 if len(pt) else 0
    features, points, local = [], [], []
    for v in range(views):
        obs = np.nonzero(cam == v)[0]
        obs = obs[rng.permutation(len(obs))]
        features.append(uv[obs])
        points.append(pt[obs].astype(np.int64))
        where = np.full(P, -1, dtype=np.int64)
        where[pt[obs]] = np.arange(len(obs))
        local.append(where)
    pairs, matches, wrong = [], [], []
    for i in range(views):
        for j in range(i + 1, min(views, i + window + 1)):
            common = np.nonzero((local[i] >= 0) & (local[j] >= 0))[0]
            common = common[rng.permutation(len(common))]
            m = np.column_stack([local[i][common], local[j][common]]).astype(np.int64)
            bad = rng.random(len(m)) < wrong_fraction
            m[bad, 1] = rng.integers(0, len(features[j]), int(bad.sum()))
            pairs.append((i, j))
            matches.append(m.reshape(-1, 2))
            wrong.append(bad & (m[:, 1] != local[j][common]))
    return dict(features=features, pairs=np.array(pairs, dtype=np.int64).reshape(-1, 2), matches=matches,
                feature_points=points, wrong=wrong)


def match_graph(images: int, features: int, neighbours: int, matches_per_pair: int, wrong_fraction: float = 0.0,
                seed: int = 0):
    """A match graph for scale, with no geometry, built vectorised.  Image i sees the latent points i * s .. i * s +
    ``features`` - 1 (mod images * s, s = features // (2 neighbours)), feature k of an image is a seeded permutation of them;
    image i is paired with (i + d) mod images for d = 1 .. ``neighbours``, and each pair matches ``matches_per_pair`` points
    of the two images' overlap (a contiguous run of them at a random start), ``wrong_fraction`` of them re-paired to a
    random feature of the second image.  Returns dict(image_offset (I + 1,), pairs (Q, 2), match_offset (Q + 1,),
    match_index (E, 2), all int32, feature_points (F,) int64 the latent point of each global id)."""
    if not 1 <= neighbours < images:
        raise ValueError("neighbours must be in [1, images)")
    rng = np.random.default_rng(seed)
    step = max(1, features // (2 * neighbours))
    P = max(images * step, features)
    if matches_per_pair > features - neighbours * step:
        raise ValueError("matches_per_pair exceeds the overlap of the farthest neighbours")
    perm = rng.permuted(np.tile(np.arange(features, dtype=np.int64), (images, 1)), axis=1)   # canonical k -> local index
    canon = np.argsort(perm, axis=1)                                                          # local index -> canonical k
    feature_points = ((np.arange(images, dtype=np.int64)[:, None] * step + canon) % P).reshape(-1)
    a_img = np.repeat(np.arange(images, dtype=np.int64), neighbours)
    d = np.tile(np.arange(1, neighbours + 1, dtype=np.int64), images)
    b_img = (a_img + d) % images
    Q = len(a_img)
    overlap = features - d * step
    start = (rng.random(Q) * (overlap - matches_per_pair + 1)).astype(np.int64)
    t = start[:, None] + np.arange(matches_per_pair, dtype=np.int64)[None, :]   # canonical index in image b
    ka, kb = t + d[:, None] * step, t
    la = perm[a_img[:, None], ka]
    lb = perm[b_img[:, None], kb]
    wrong = rng.random(lb.shape) < wrong_fraction
    lb = np.where(wrong, rng.integers(0, features, lb.shape), lb)
    off = np.arange(images + 1, dtype=np.int64) * features
    return dict(image_offset=off.astype(np.int32), pairs=np.column_stack([a_img, b_img]).astype(np.int32),
                match_offset=(np.arange(Q + 1, dtype=np.int64) * matches_per_pair).astype(np.int32),
                match_index=np.column_stack([la.reshape(-1), lb.reshape(-1)]).astype(np.int32), feature_points=feature_points)


def rotated_texture_pair(height: int, width: int, degrees: float, n: int, seed: int, noise: float = 0.01):
    """Two uint8 views of one band-limited random texture, the second rotated by ``degrees`` about the image centre, with
    ``n`` ground-truth feature pairs: the scene the descriptor matchers are compared on.

    The texture is white noise smoothed by a separable Gaussian (sigma 1.5 px) on a square canvas that covers the image at
    every rotation, stretched to 0..255 and quantised.  The first image is the canvas's central ``height`` x ``width``
    crop.  Pixel q of the second image samples the quantised canvas bilinearly at centre + R(degrees) (q - centre), plus
    Gaussian noise of standard deviation ``noise`` * 255, rounded and clipped.  A feature at p in the first image is
    therefore at centre + R(-degrees) (p - centre) in the second.  First-image features are integer pixels; a pair is kept
    only if both ends are at least 20 px from every border.  Pure NumPy, elementwise operations only.

    Returns (image_a, image_b, pairs): pairs float64 [n, 4] = (xa, ya, xb, yb)."""
    if height < 48 or width < 48:
        raise ValueError("rotated_texture_pair: the image must be at least 48 x 48")
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.hypot(height, width))) + 8
    radius, sigma = 5, 1.5
    taps = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
    taps /= taps.sum()
    white = rng.standard_normal((side + 2 * radius, side + 2 * radius))
    rows = sum(taps[k] * white[:, k:k + side] for k in range(2 * radius + 1))
    smooth = sum(taps[k] * rows[k:k + side, :] for k in range(2 * radius + 1))
    lo, hi = smooth.min(), smooth.max()
    canvas = np.floor((smooth - lo) / (hi - lo) * 255.0 + 0.5)
    oy, ox = (side - height) // 2, (side - width) // 2
    image_a = canvas[oy:oy + height, ox:ox + width].astype(np.uint8)

    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    th = np.deg2rad(degrees)
    c, s = np.cos(th), np.sin(th)
    qx, qy = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    sx = cx + c * (qx - cx) - s * (qy - cy) + ox
    sy = cy + s * (qx - cx) + c * (qy - cy) + oy
    x0 = np.clip(np.floor(sx).astype(np.int64), 0, side - 2)
    y0 = np.clip(np.floor(sy).astype(np.int64), 0, side - 2)
    fx, fy = sx - x0, sy - y0
    value = ((1 - fy) * ((1 - fx) * canvas[y0, x0] + fx * canvas[y0, x0 + 1])
             + fy * ((1 - fx) * canvas[y0 + 1, x0] + fx * canvas[y0 + 1, x0 + 1]))
    value = value + rng.standard_normal(value.shape) * (noise * 255.0)
    image_b = np.clip(np.floor(value + 0.5), 0, 255).astype(np.uint8)

    border = 20
    pairs = np.empty((0, 4))
    while len(pairs) < n:
        xa = rng.integers(border, width - border, 4 * n).astype(np.float64)
        ya = rng.integers(border, height - border, 4 * n).astype(np.float64)
        xb = cx + c * (xa - cx) + s * (ya - cy)
        yb = cy - s * (xa - cx) + c * (ya - cy)
        keep = (xb >= border) & (xb <= width - 1 - border) & (yb >= border) & (yb <= height - 1 - border)
        pairs = np.concatenate([pairs, np.column_stack([xa, ya, xb, yb])[keep]])
    return image_a, image_b, pairs[:n]


def rotated_texture_views(height: int, width: int, degrees, n: int, extra: int, seed: int, noise: float = 0.01):
    """``rotated_texture_pair``'s scene as a collection: one uint8 view of the same kind of canvas per entry of ``degrees``,
    with ``n`` ground-truth features that every view sees and ``extra`` partnerless ones per view — what a graph matcher is
    measured on.

    The canvas and the sampling are ``rotated_texture_pair``'s: pixel q of view v samples the quantised canvas bilinearly
    at centre + R(degrees[v]) (q - centre), plus Gaussian noise of standard deviation ``noise`` * 255, rounded and clipped
    (every view, a view at 0 degrees included, is sampled and noisy).  The latent points are integer pixels of the
    unrotated frame inside the disc about the image centre that stays 20 px from the borders of every view; latent point p
    is at centre + R(-degrees[v]) (p - centre) in view v.  The partnerless features of a view are integer pixels at least
    20 px from its borders.  Each view's features are shuffled, so an index says nothing.

    Returns (images, features, ids): per view a uint8 [height, width] image, a float64 [n + extra, 2] array of (x, y) and an
    int64 [n + extra] array with the latent point of each feature, -1 for a partnerless one."""
    if height < 48 or width < 48:
        raise ValueError("rotated_texture_views: the image must be at least 48 x 48")
    if n < 0 or extra < 0:
        raise ValueError("rotated_texture_views: n and extra must not be negative")
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.hypot(height, width))) + 8
    radius, sigma = 5, 1.5
    taps = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
    taps /= taps.sum()
    white = rng.standard_normal((side + 2 * radius, side + 2 * radius))
    rows = sum(taps[k] * white[:, k:k + side] for k in range(2 * radius + 1))
    smooth = sum(taps[k] * rows[k:k + side, :] for k in range(2 * radius + 1))
    lo, hi = smooth.min(), smooth.max()
    canvas = np.floor((smooth - lo) / (hi - lo) * 255.0 + 0.5)
    oy, ox = (side - height) // 2, (side - width) // 2
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    qx, qy = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    turns = [(np.cos(np.deg2rad(d)), np.sin(np.deg2rad(d))) for d in degrees]
    images = []
    for c, s in turns:
        sx = cx + c * (qx - cx) - s * (qy - cy) + ox
        sy = cy + s * (qx - cx) + c * (qy - cy) + oy
        x0 = np.clip(np.floor(sx).astype(np.int64), 0, side - 2)
        y0 = np.clip(np.floor(sy).astype(np.int64), 0, side - 2)
        fx, fy = sx - x0, sy - y0
        value = ((1 - fy) * ((1 - fx) * canvas[y0, x0] + fx * canvas[y0, x0 + 1])
                 + fy * ((1 - fx) * canvas[y0 + 1, x0] + fx * canvas[y0 + 1, x0 + 1]))
        value = value + rng.standard_normal(value.shape) * (noise * 255.0)
        images.append(np.clip(np.floor(value + 0.5), 0, 255).astype(np.uint8))

    border = 20
    reach = min(cx, cy) - border                       # the disc every rotation keeps inside every view's margin
    latent = np.empty((0, 2))
    while len(latent) < n:
        x = rng.integers(border, width - border, 4 * n).astype(np.float64)
        y = rng.integers(border, height - border, 4 * n).astype(np.float64)
        keep = (x - cx) ** 2 + (y - cy) ** 2 <= reach * reach
        latent = np.concatenate([latent, np.column_stack([x, y])[keep]])
    latent = latent[:n]
    features, ids = [], []
    for c, s in turns:
        seen = np.column_stack([cx + c * (latent[:, 0] - cx) + s * (latent[:, 1] - cy),
                                cy - s * (latent[:, 0] - cx) + c * (latent[:, 1] - cy)])
        alone = np.column_stack([rng.integers(border, width - border, extra), rng.integers(border, height - border, extra)])
        order = rng.permutation(n + extra)
        features.append(np.concatenate([seen, alone.astype(np.float64)])[order])
        ids.append(np.concatenate([np.arange(n, dtype=np.int64), np.full(extra, -1, dtype=np.int64)])[order])
    return images, features, ids


def similarity_texture_views(height: int, width: int, degrees, scales, seed: int, noise: float = 0.01):
    """Views of one multi-scale random texture that differ by a rotation AND a scale about the image centre — two photographs
    of one object taken from different distances — what a multi-scale detector is measured on.

    The canvas is the sum of four unit-variance Gaussian-smoothed white noises (sigma = 1.5, 3, 6 and 12 px: structure at every
    scale a pyramid looks at), stretched to 0 .. 255 and quantised, and large enough for the largest scale at every rotation.
    Pixel q of view v looks at canvas point C + scales[v] R(degrees[v]) (q - c), c the image centre and C the canvas centre: it
    is the mean of k x k bilinear samples spread evenly over the pixel's footprint, k = ceil(scales[v]), plus Gaussian noise of
    standard deviation ``noise`` * 255, rounded and clipped as in ``rotated_texture_views``.

    Returns (images, to_canvas): per view a uint8 [height, width] image and a float64 [2, 3] matrix A with
    canvas (x, y) = A @ (x, y, 1) for a pixel (x, y) of that view."""
    degrees, scales = [float(d) for d in degrees], [float(s) for s in scales]
    if height < 48 or width < 48:
        raise ValueError("similarity_texture_views: the image must be at least 48 x 48")
    if len(degrees) != len(scales) or not all(np.isfinite(s) and s > 0 for s in scales):
        raise ValueError("similarity_texture_views: one positive scale per rotation")
    rng = np.random.default_rng(seed)
    side = int(np.ceil(max(scales, default=1.0) * np.hypot(height, width))) + 8
    smooth = np.zeros((side, side))
    for sigma in (1.5, 3.0, 6.0, 12.0):
        radius = int(np.ceil(3 * sigma))
        taps = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
        taps /= taps.sum()
        white = rng.standard_normal((side + 2 * radius, side + 2 * radius))
        rows = sum(taps[k] * white[:, k:k + side] for k in range(2 * radius + 1))
        band = sum(taps[k] * rows[k:k + side, :] for k in range(2 * radius + 1))
        smooth += band / np.sum(taps * taps)            # the standard deviation of the separable filter's output
    lo, hi = smooth.min(), smooth.max()
    canvas = np.floor((smooth - lo) / (hi - lo) * 255.0 + 0.5)
    C = (side - 1) / 2.0
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    qx, qy = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    images, to_canvas = [], []
    for d, scale in zip(degrees, scales):
        c, s = scale * np.cos(np.deg2rad(d)), scale * np.sin(np.deg2rad(d))
        A = np.array([[c, -s, C - c * cx + s * cy], [s, c, C - s * cx - c * cy]])
        k = int(np.ceil(scale))
        value = np.zeros((height, width))
        for iy in range(k):
            for ix in range(k):
                px, py = qx + ((ix + 0.5) / k - 0.5), qy + ((iy + 0.5) / k - 0.5)
                sx = A[0, 0] * px + A[0, 1] * py + A[0, 2]
                sy = A[1, 0] * px + A[1, 1] * py + A[1, 2]
                x0 = np.clip(np.floor(sx).astype(np.int64), 0, side - 2)
                y0 = np.clip(np.floor(sy).astype(np.int64), 0, side - 2)
                fx, fy = sx - x0, sy - y0
                value += ((1 - fy) * ((1 - fx) * canvas[y0, x0] + fx * canvas[y0, x0 + 1])
                          + fy * ((1 - fx) * canvas[y0 + 1, x0] + fx * canvas[y0 + 1, x0 + 1]))
        value = value / (k * k) + rng.standard_normal(value.shape) * (noise * 255.0)
        images.append(np.clip(np.floor(value + 0.5), 0, 255).astype(np.uint8))
        to_canvas.append(A)
    return images, to_canvas


def repeated_structure_views(views: int, points: int, unique: int, groups: int, extra: int, seed: int, flips: int = 20,
                             noise_px: float = 0.5, step_deg: float = 5.0):
    """Views of a scene with repeated structure, for guided matching: the geometry of
    ``multi_view_scene(views, points, seed, noise_px, 0.0, step_deg)`` with a 32-byte binary descriptor per observation.

    Latent points 0 .. ``unique`` - 1 have a random prototype descriptor of their own; the other ``points - unique`` share
    ``groups`` prototypes (point ``unique + k`` has prototype ``k % groups``): look-alikes at different places, which a
    descriptor-space ratio test cannot tell apart.  Every observation is its point's prototype with 0 .. ``flips`` random bits
    flipped.  Each view also gets ``extra`` partnerless features: uniform random pixels with random descriptors.  The features
    of a view are shuffled.

    Returns dict(pixels: per view float64 (n_v, 2); descriptors: per view (bits uint8 (n_v, 32), valid bool (n_v,), all true);
    ids: per view int64 (n_v,), the latent point or -1 for a partnerless feature; K; poses_true (views, 12))."""
    if not 0 <= unique <= points or groups < 0 or (points > unique and groups < 1) or extra < 0 or not 0 <= flips <= 256:
        raise ValueError("repeated_structure_views: need 0 <= unique <= points, groups >= 1 when points > unique, extra >= 0 "
                         "and 0 <= flips <= 256")
    scene = multi_view_scene(views, points, seed, noise_px, 0.0, step_deg)
    rng = np.random.default_rng([seed, 0x6ad])
    K = scene["K"]
    width, height = 2.0 * K[0, 2], 2.0 * K[1, 2]
    prototypes = rng.integers(0, 256, (unique + groups, 32), dtype=np.uint8)
    prototype_of = np.concatenate([np.arange(unique), unique + np.arange(points - unique) % max(groups, 1)]).astype(np.int64)
    pixels, descriptors, ids = [], [], []
    for v in range(views):
        seen = scene["camera_indices"] == v
        latent = scene["point_indices"][seen].astype(np.int64)
        n = len(latent)
        flip = np.zeros((n, 256), dtype=np.uint8)
        for row, count in zip(flip, rng.integers(0, flips + 1, n)):
            row[rng.choice(256, count, replace=False)] = 1
        bits = prototypes[prototype_of[latent]] ^ np.packbits(flip, axis=1, bitorder="little")
        alone_px = np.column_stack([rng.uniform(0, width, extra), rng.uniform(0, height, extra)])
        alone_bits = rng.integers(0, 256, (extra, 32), dtype=np.uint8)
        order = rng.permutation(n + extra)
        pixels.append(np.ascontiguousarray(np.vstack([scene["pixels"][seen], alone_px])[order]))
        descriptors.append((np.ascontiguousarray(np.vstack([bits, alone_bits])[order]), np.ones(n + extra, dtype=bool)))
        ids.append(np.concatenate([latent, np.full(extra, -1, dtype=np.int64)])[order])
    return dict(pixels=pixels, descriptors=descriptors, ids=ids, K=K, poses_true=scene["poses_true"])


def arc_poses(views: int, step_deg: float = 4.0, distance: float = 5.0) -> np.ndarray:
    """(views, 12) poses, R row-major then t: cameras on an arc about the point (0, 0, distance), ``step_deg`` degrees apart about
    the Y axis and centred on the Z axis, all looking at that point (the arc of ``multi_view_scene``, centred)."""
    poses = np.zeros((views, 12))
    for i in range(views):
        a = np.radians((i - (views - 1) / 2.0) * step_deg)
        R = np.array([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
        centre = np.array([-distance * np.sin(a), 0.0, distance - distance * np.cos(a)])
        poses[i, :9] = R.reshape(9)
        poses[i, 9:] = -R @ centre
    return poses


def plane_views(height: int, width: int, poses, planes, seed: int, K=None, texels_per_unit: float = 24.0, texture_size: int = 128):
    """Grey views of one or more textured planes, with the exact depth of every pixel.

    ``poses``: (V, 12) world to camera, R row-major then t.  ``planes``: a list of ``(origin, u, v, extent)``: the plane through
    ``origin`` spanned by the orthonormal directions ``u`` and ``v``, cut to ``|s| <= extent[0]``, ``|t| <= extent[1]`` in those
    coordinates, or unbounded with ``extent=None``.  ``K``: the camera matrix (default: focal length 1.2 ``width``, principal
    point at the image centre).  Per pixel the ray is intersected with every plane and the nearest hit in front of the camera
    is taken; its grey value is the bilinear lookup of the plane's own random texture (``texture_size`` squared texels, repeated,
    ``texels_per_unit`` texels per world unit), rounded to uint8.  A slanted plane gives a depth ramp; a second, bounded plane in
    front gives occlusions.  Returns dict(images (V, H, W) uint8, depth (V, H, W) camera depth of the hit (NaN: no plane hit, grey
    0), plane (V, H, W) int32 index of the plane hit or -1, K)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    if K is None:
        K = np.array([[1.2 * width, 0.0, (width - 1) / 2.0], [0.0, 1.2 * width, (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    K = np.asarray(K, dtype=np.float64)
    rng = np.random.default_rng(seed)
    textures = [rng.integers(0, 256, size=(texture_size, texture_size)).astype(np.float64) for _ in planes]
    V = len(poses)
    images = np.zeros((V, height, width), dtype=np.uint8)
    depth = np.full((V, height, width), np.nan)
    hit = np.full((V, height, width), -1, dtype=np.int32)
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    rays_cam = np.stack([x, y, np.ones_like(x)], axis=-1) @ np.linalg.inv(K).T   # camera depth 1 along every ray
    for i in range(V):
        R, t = poses[i, :9].reshape(3, 3), poses[i, 9:]
        centre = -R.T @ t
        rays = rays_cam @ R   # world directions: R^T applied to every row
        nearest = np.full((height, width), np.inf)
        grey = np.zeros((height, width))
        for k, ((origin, u, v, extent), texture) in enumerate(zip(planes, textures)):
            origin, u, v = (np.asarray(a, dtype=np.float64) for a in (origin, u, v))
            normal = np.cross(u, v)
            with np.errstate(all="ignore"):
                lam = float(normal @ (origin - centre)) / (rays @ normal)   # the camera depth of the hit, as rays have depth 1
            P = centre + lam[..., None] * rays - origin
            s, tt = P @ u, P @ v
            ok = np.isfinite(lam) & (lam > 0.0) & (lam < nearest)
            if extent is not None:
                ok &= (np.abs(s) <= extent[0]) & (np.abs(tt) <= extent[1])
            a, b = np.where(ok, s, 0.0) * texels_per_unit, np.where(ok, tt, 0.0) * texels_per_unit
            a0, b0 = np.floor(a), np.floor(b)
            fa, fb = a - a0, b - b0
            ia, ib = a0.astype(np.int64) % texture_size, b0.astype(np.int64) % texture_size
            ja, jb = (ia + 1) % texture_size, (ib + 1) % texture_size
            value = (texture[ib, ia] * (1 - fa) + texture[ib, ja] * fa) * (1 - fb) + (texture[jb, ia] * (1 - fa) + texture[jb, ja] * fa) * fb
            grey = np.where(ok, value, grey)
            nearest = np.where(ok, lam, nearest)
            hit[i][ok] = k
        images[i] = np.clip(np.rint(grey), 0, 255).astype(np.uint8)
        depth[i] = np.where(np.isfinite(nearest), nearest, np.nan)
    return dict(images=images, depth=depth, plane=hit, K=K)
