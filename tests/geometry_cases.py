"""A small family of cameras and worlds for the kernels that take a camera matrix K and poses in a world frame (PnP fits,
scoring, mask, refinement; both bundle adjusters; track triangulation).  Imported by tests/test_geometry_cases_host.py,
tests/test_gpu_geometry_cases.py and the finite-difference tests, like bundle_graphs.py.

Cameras: name -> K, all with row 2 = (0, 0, 1).  A problem is made by the existing generators at synthetic.BENCH_K (their
geometry, visibility, observation graph and perturbed start), and its pixels are then projected again from the true
poses and points with the case's K, with Gaussian noise of ``noise_px * PIXEL_UNIT[camera]``: the pixel unit of ``unit``
(normalised coordinates) is 1 / 1520 of the others', so its noise and its thresholds (px^2: ``threshold``) shrink with it.

Worlds: name -> similarity X' = s Q X + T of the world frame.  Poses map by R' = R Q^T, t' = s t - R' T, so that
R' X' + t' = s (R X + t) and every pixel is unchanged.  ``far`` moves the origin 2e4 scene sizes away: the track DLT and
the pose updates about the world origin lose the digits the offset takes, so it is for the one-shot kernels only."""
import numpy as np

import pnp_oracle
from structure_from_motion_amd import synthetic

BENCH_K = synthetic.BENCH_K


def _with(K, **entries):
    K = K.copy()
    for name, value in entries.items():
        K[int(name[1]), int(name[2])] = value
    return K


CAMERAS = {
    "bench": BENCH_K.copy(),
    "skew": _with(BENCH_K, k01=45.0),
    "affine": np.array([[1520.4, 45.0, 302.32], [-20.0, 760.0, 246.87], [0.0, 0.0, 1.0]]),
    "wide8k": np.array([[11000.0, 0.0, 3840.0], [0.0, 11050.0, 2160.0], [0.0, 0.0, 1.0]]),
    "unit": np.eye(3),
}
PIXEL_UNIT = {"bench": 1.0, "skew": 1.0, "affine": 1.0, "wide8k": 1.0, "unit": 1.0 / 1520.0}


def rotation(axis, degrees):
    """exp([a]x) for a = radians(degrees) * axis / |axis| (Rodrigues)."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    a = np.radians(degrees)
    W = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * W + (1.0 - np.cos(a)) * (W @ W)


# name -> (s, Q, T)
WORLDS = {
    "id": (1.0, np.eye(3), np.zeros(3)),
    "turned": (1.0, rotation((1.0, 2.0, 3.0), 170.0), np.array([3.0, -2.0, 1.0])),
    "large": (1e3, rotation((0.0, 1.0, 0.0), 95.0), np.zeros(3)),
    "small": (1e-3, rotation((1.0, 0.0, 0.0), -120.0), np.zeros(3)),
    "far": (1.0, np.eye(3), np.array([1e4, -2e4, 5e3])),
}
ITERATIVE_WORLDS = ("id", "turned", "large", "small")
ALL_WORLDS = ITERATIVE_WORLDS + ("far",)


def threshold(camera, px2):
    """A threshold of px2 squared bench pixels in the camera's own pixel unit."""
    return px2 * PIXEL_UNIT[camera] ** 2


def project(K, poses, points):
    """Pixels of points (m, 3) under poses (m, 12) = {R | t}: K (R X + t) dehomogenised."""
    R = poses[:, :9].reshape(-1, 3, 3)
    uvw = (np.einsum("mij,mj->mi", R, points) + poses[:, 9:]) @ np.asarray(K).T
    return uvw[:, :2] / uvw[:, 2:3]


def _pixels(camera, poses, points, noise_px, outlier, rng):
    """The observations' pixels under the camera: projected, noisy, and uniform in the box of the projections where
    ``outlier`` is set."""
    uv = project(CAMERAS[camera], poses, points)
    lo, hi = uv.min(axis=0), uv.max(axis=0)
    uv = uv + rng.normal(0.0, 1.0, uv.shape) * (noise_px * PIXEL_UNIT[camera])
    random_px = lo + rng.random(uv.shape) * (hi - lo)
    return np.where(np.asarray(outlier, dtype=bool)[:, None], random_px, uv)


def bundle_case(camera, cameras, points, seed, per_point=4, noise_px=0.5):
    """synthetic.bundle_problem's dict (graph, true values and perturbed start) with K and the pixels of ``camera``."""
    pr = synthetic.bundle_problem(cameras, points, per_point=per_point, seed=seed, noise_px=0.0)
    cam, pt = pr["camera_indices"], pr["point_indices"]
    uv = _pixels(camera, pr["poses_true"][cam], pr["points_true"][pt], noise_px, np.zeros(len(cam), bool),
                 np.random.default_rng(1000 + seed))
    return dict(pr, K=CAMERAS[camera].copy(), pixels=uv)


def tracks_case(camera, views, points, seed, noise_px=0.5, outliers=0.0):
    """synthetic.multi_view_scene's tracks (visibility at BENCH_K, lengths 2 .. views) under ``camera``: dict(K, poses,
    cam, pt, uv, P, points_true); the observations in random order."""
    sc = synthetic.multi_view_scene(views, points, seed, noise_px=0.0, outlier_fraction=outliers)
    rng = np.random.default_rng(2000 + seed)
    cam, pt = sc["camera_indices"], sc["point_indices"]
    uv = _pixels(camera, sc["poses_true"][cam], sc["points_true"][pt], noise_px, sc["is_outlier"], rng)
    order = rng.permutation(len(cam))
    return dict(K=CAMERAS[camera].copy(), poses=sc["poses_true"], cam=cam[order], pt=pt[order], uv=uv[order], P=points,
                points_true=sc["points_true"])


def pnp_case(camera, n, seed, outliers=0.3, noise_px=0.5):
    """pnp_oracle.scene's points, pose and outlier set under ``camera``: (pts (n, 5), R, t)."""
    pts, R, t = pnp_oracle.scene(n, seed, BENCH_K, outlier_fraction=outliers, noise_px=0.0)
    pose = np.tile(np.concatenate([R.reshape(9), t]), (n, 1))
    outlier = np.max(np.abs(project(BENCH_K, pose, pts[:, :3]) - pts[:, 3:]), axis=1) > 1e-6
    uv = _pixels(camera, pose, pts[:, :3], noise_px, outlier, np.random.default_rng(3000 + seed))
    return np.column_stack([pts[:, :3], uv]), R, t


# ---- worlds ---------------------------------------------------------------------------------------------------------
def points_to(world, X):
    s, Q, T = WORLDS[world]
    return s * (np.asarray(X) @ Q.T) + T


def points_back(world, X):
    s, Q, T = WORLDS[world]
    return ((np.asarray(X) - T) @ Q) / s


def poses_to(world, poses):
    """poses (..., 12) = {R | t} -> {R Q^T | s t - R Q^T T}."""
    s, Q, T = WORLDS[world]
    poses = np.asarray(poses, dtype=np.float64)
    R = poses[..., :9].reshape(poses.shape[:-1] + (3, 3)) @ Q.T
    t = s * poses[..., 9:] - R @ T
    return np.concatenate([R.reshape(poses.shape[:-1] + (9,)), t], axis=-1)


def poses_back(world, poses):
    """The inverse of poses_to: {R' Q | (t' + R' T) / s}."""
    s, Q, T = WORLDS[world]
    poses = np.asarray(poses, dtype=np.float64)
    Rw = poses[..., :9].reshape(poses.shape[:-1] + (3, 3))
    t = (poses[..., 9:] + Rw @ T) / s
    return np.concatenate([(Rw @ Q).reshape(poses.shape[:-1] + (9,)), t], axis=-1)


def problem_to(world, pr):
    """A bundle_case / tracks_case dict in the world: every pose and point array it holds is mapped, the rest is kept."""
    out = dict(pr)
    for key in ("poses", "poses_true"):
        if key in pr:
            out[key] = poses_to(world, pr[key])
    for key in ("points", "points_true"):
        if key in pr:
            out[key] = points_to(world, pr[key])
    return out


def pnp_to(world, pts, R, t):
    """(pts (n, 5), R, t) of a PnP scene in the world."""
    pose = poses_to(world, np.concatenate([np.asarray(R).reshape(9), np.asarray(t)]))
    return np.column_stack([points_to(world, pts[:, :3]), pts[:, 3:]]), pose[:9].reshape(3, 3), pose[9:]


def pose_back(world, R, t):
    """(R, t) of a result in the world, in the original frame and unit."""
    pose = poses_back(world, np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)]))
    return pose[:9].reshape(3, 3), pose[9:]


def rotation_gap(Ra, Rb):
    """max |Ra - Rb|: resolves what the arc-cosine of a trace cannot (anything below 4e-8 rad)."""
    return float(np.max(np.abs(np.asarray(Ra) - np.asarray(Rb))))
