"""Headless three-view structure from motion on synthetic data: the two-view pipeline on views 1 and 2
(``estimate_essential_mat_with_ransac`` -> ``recover_r_t_from_e`` -> ``triangulate_points``), then view 3 registered against
the triangulated points with ``estimate_pose_pnp_with_ransac``.  Points are projected directly (no images), a fraction of
the view-2 and view-3 observations are replaced by random pixels, and the recovered pose of view 3 is compared with ground
truth in the scale of the two-view reconstruction (|t_2| = 1).  ``--refine K`` refines the view-3 pose on its inliers
(``refine_rounds=K``) and also reports the unrefined pose's errors, from the same RANSAC draw, next to the refined ones.
``--bundle-adjust N`` then adjusts all three cameras (camera 1 fixed) and the triangulated points together, at most N
Levenberg-Marquardt steps, on views 1 and 2 of every triangulated point and view 3 of every PnP inlier, and reports the
errors and the RMS reprojection error before and after.
"""
from __future__ import annotations

import argparse
import json
import random

import numpy as np

from lib.common.feature import Feature
from lib.epipolar.eight_point import create_trivial_matches, recover_r_t_from_e
from lib.epipolar.epipolar_ransac import estimate_essential_mat_with_ransac
from lib.bundle.bundle import bundle_adjust as adjust_bundle
from lib.epipolar.triangulation import triangulate_points
from lib.feature_matching.matching import Match
from lib.pnp.pnp import estimate_pose_pnp_with_ransac
from lib.transforms.transforms import Transform3D
from structure_from_motion_amd import synthetic


def three_view_scene(n: int = 400, seed: int = 11, outlier_fraction: float = 0.3, noise_px: float = 0.0):
    """Points uniform in x, y in [-1, 1], z in [4, 6] (frame of camera 1 = [I | 0]); camera 2 and camera 3 at fixed poses.
    Returns dict of pixel arrays pa, pb, pc (n, 2), K, and the ground-truth poses R2, t2, R3, t3."""
    rng = np.random.default_rng(seed)
    K = synthetic.BENCH_K
    X = np.column_stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(4.0, 6.0, n)])
    R2, t2 = synthetic.rotation_xy(-5.0, -10.0), np.array([0.5, 0.05, 0.1])
    R3, t3 = synthetic.rotation_xy(4.0, 9.0), np.array([-0.45, 0.12, 0.2])

    def project(Xc):
        uvw = Xc @ K.T
        return uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, noise_px, (len(Xc), 2))

    def corrupt(p):
        out = rng.random(n) < outlier_fraction
        rand_px = np.column_stack([rng.uniform(0, 2 * K[0, 2], n), rng.uniform(0, 2 * K[1, 2], n)])
        return np.where(out[:, None], rand_px, p)

    pa = project(X)
    pb = corrupt(project(X @ R2.T + t2))
    pc = corrupt(project(X @ R3.T + t3))
    return dict(pa=pa, pb=pb, pc=pc, K=K, X=X, R2=R2, t2=t2, R3=R3, t3=t3)


def rotation_angle(Ra: np.ndarray, Rb: np.ndarray) -> float:
    """Angle in radians of Ra Rb^T."""
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def run(n: int = 400, seed: int = 11, outlier_fraction: float = 0.3, noise_px: float = 0.0, sed_threshold: float = 1.5e-6,
        reprojection_threshold: float = 4.0, iterations: int = 2000, refine: int = 0, bundle_adjust: int = 0,
        pnp_solver: str = "dlt", e_solver: str = "eight_point") -> dict:
    scene = three_view_scene(n, seed, outlier_fraction, noise_px)
    K = scene["K"]
    features_a = [Feature(float(x), float(y)) for x, y in scene["pa"]]
    features_b = [Feature(float(x), float(y)) for x, y in scene["pb"]]
    features_c = [Feature(float(x), float(y)) for x, y in scene["pc"]]
    random.seed(seed)
    # views 1-2: E, pose, triangulation of the cheirality survivors
    e, inlier_pairs = estimate_essential_mat_with_ransac(
        K, features_a, features_b, create_trivial_matches(n), sed_inlier_threshold=sed_threshold,
        min_num_extra_inliers=10, max_iterations=iterations, solver=e_solver)
    R2, t2, mask = recover_r_t_from_e(e, K, [p[0] for p in inlier_pairs], [p[1] for p in inlier_pairs])
    kept = [inlier_pairs[i] for i in mask]
    points = triangulate_points([p[0] for p in kept], [p[1] for p in kept], K, Transform3D.from_rmat_t(R2, t2))
    # view 3: its features matched to the triangulated points (the observation of the same scene point)
    index_of = {(f.x, f.y): i for i, f in enumerate(features_a)}
    matches = [Match(a_index=k, b_index=index_of[(p[0].x, p[0].y)]) for k, p in enumerate(kept)]
    state = random.getstate()
    R3, t3, inliers = estimate_pose_pnp_with_ransac(K, points, features_c, matches, reprojection_threshold,
                                                    min_num_extra_inliers=10, max_iterations=iterations, solver=pnp_solver)
    scale = np.linalg.norm(scene["t2"])
    unrefined = {}
    if refine > 0:
        unrefined = {
            "pnp_inliers_unrefined": len(inliers),
            "R3_error_rad_unrefined": rotation_angle(R3, scene["R3"]),
            "t3_error_unrefined": float(np.linalg.norm(t3 - scene["t3"] / scale)),
        }
        random.setstate(state)   # the same RANSAC draw, now refined
        R3, t3, inliers = estimate_pose_pnp_with_ransac(K, points, features_c, matches, reprojection_threshold,
                                                        min_num_extra_inliers=10, max_iterations=iterations,
                                                        refine_rounds=refine, solver=pnp_solver)
    adjusted = {}
    if bundle_adjust > 0:
        adjusted = _bundle_adjust(scene, K, points, kept, features_c, matches, R2, t2, R3, t3, reprojection_threshold,
                                  bundle_adjust)
        R2, t2, R3, t3 = adjusted.pop("R2"), adjusted.pop("t2"), adjusted.pop("R3"), adjusted.pop("t3")
    return {
        "points": n,
        "two_view_inliers": len(inlier_pairs),
        "triangulated": len(kept),
        "pnp_inliers": len(inliers),
        "R2_error_rad": rotation_angle(R2, scene["R2"]),
        "R3_error_rad": rotation_angle(R3, scene["R3"]),
        "t3_error": float(np.linalg.norm(t3 - scene["t3"] / scale)),
        "R3": R3.tolist(),
        "t3": t3.tolist(),
        **unrefined,
        **adjusted,
    }


def _bundle_adjust(scene, K, points, kept, features_c, matches, R2, t2, R3, t3, threshold, max_steps) -> dict:
    """Bundle adjustment of the three views and the triangulated points (camera 1 fixed): views 1 and 2 of every point,
    view 3 of every match whose squared reprojection error under (R3, t3) is at most ``threshold`` (the PnP inliers)."""
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    uv_c = np.array([[features_c[m.b_index].x, features_c[m.b_index].y] for m in matches]).reshape(-1, 2)
    xc = X @ R3.T + t3
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.sum(((xc @ K.T)[:, :2] / xc[:, 2:3] - uv_c) ** 2, axis=1)
    inl = np.nonzero((xc[:, 2] > 0) & (e <= threshold))[0]
    pixels = np.vstack([[[p[0].x, p[0].y] for p in kept], [[p[1].x, p[1].y] for p in kept], uv_c[inl]]).reshape(-1, 2)
    cams = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32), np.full(len(inl), 2, np.int32)])
    pts = np.concatenate([np.arange(n), np.arange(n), inl]).astype(np.int32)
    poses = np.array([np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), np.concatenate([R2.reshape(9), t2.reshape(3)]),
                      np.concatenate([R3.reshape(9), t3.reshape(3)])])
    out, _, info = adjust_bundle(K, poses, X, cams, pts, pixels, fixed_cameras=(0,), max_steps=max_steps)
    scale = np.linalg.norm(scene["t2"])
    return {
        "R2_error_rad_before_ba": rotation_angle(R2, scene["R2"]),
        "R3_error_rad_before_ba": rotation_angle(R3, scene["R3"]),
        "t3_error_before_ba": float(np.linalg.norm(t3 - scene["t3"] / scale)),
        "rms_px_before_ba": float(np.sqrt(info.initial_cost / len(cams))),
        "rms_px": float(np.sqrt(info.final_cost / len(cams))),
        "ba_observations": len(cams),
        "ba_status": info.status,
        "ba_steps": info.steps,
        "ba_accepted": info.accepted,
        "R2": out[1, :9].reshape(3, 3), "t2": out[1, 9:], "R3": out[2, :9].reshape(3, 3), "t3": out[2, 9:],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=400)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--noise", type=float, default=0.0, help="pixel noise (standard deviation)")
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--sed-threshold", type=float, default=1.5e-6,
                    help="two-view SED inlier threshold (the default suits noise-free pixels; about 6e-6 for --noise 0.5)")
    ap.add_argument("--reprojection-threshold", type=float, default=4.0, help="PnP inlier threshold in pixels squared")
    ap.add_argument("--refine", type=int, default=0, metavar="K",
                    help="refine the view-3 pose on its inliers, K rounds (0: off); also reports the unrefined errors")
    ap.add_argument("--bundle-adjust", type=int, default=0, metavar="N",
                    help="bundle-adjust the three views and the points, at most N LM steps (0: off); also reports the "
                         "errors before it")
    ap.add_argument("--pnp-solver", choices=("dlt", "p3p"), default="dlt",
                    help="minimal solver of the view-3 PnP: six-point DLT or P3P on four-item samples")
    ap.add_argument("--e-solver", choices=("eight_point", "five_point"), default="eight_point",
                    help="minimal solver of the views-1-2 essential matrix: eight-point, or five-point on six-item samples")
    args = ap.parse_args()
    print(json.dumps(run(args.points, args.seed, args.outliers, args.noise, sed_threshold=args.sed_threshold,
                         reprojection_threshold=args.reprojection_threshold, iterations=args.iterations,
                         refine=args.refine, bundle_adjust=args.bundle_adjust, pnp_solver=args.pnp_solver,
                         e_solver=args.e_solver)))


if __name__ == "__main__":
    main()
