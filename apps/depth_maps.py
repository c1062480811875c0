"""Dense depth maps of a rendered two-plane scene: plane-sweep stereo for every view in one call, the consistency filter across
the maps and the fused point cloud, all on the GPU (``lib.stereo.depth_maps``).

V views on an arc see a slanted textured plane and a smaller plane in front of it, which hides a part of the first from every
view, a different part from each (``synthetic.plane_views``; the exact depth of every pixel is known).  All depth maps are
computed by one ``compute_depth_maps`` call, filtered by one ``filter_depth_maps`` call and compacted by ``point_cloud``.

Printed as JSON, per view: the share of the interior pixels (further than the window radius from the border) whose winning
hypothesis lies within one hypothesis step of the truth, before the filter (of all interior pixels) and after it (of the pixels
it kept), the share it kept, the median relative depth error of the sub-sample depths before and after, and the number of
points of the view in the cloud.

``--smooth P1 P2`` adds the same figures under ``"smoothed"`` for the maps whose cost volume was smoothed along 8 scanline paths
with these penalties before the winners were taken (``compute_depth_maps(..., smoothness=(P1, P2))``).

``--from-model`` takes nothing from the truth but the images and the camera matrix: sparse points of the same scene are observed
with pixel noise, reconstructed by the incremental route of ``apps/merge_reconstructions.py`` (in the gauge of its first view and
seed baseline), and the poses, each view's depth range (``depth_ranges``) and its sources (``select_source_views``) come from
that model.  The truth is brought into the model's scale for the comparison only.  One hypothesis step is a sixth of a pixel
of disparity between neighbouring views here, so the criterion is as tight for the model's poses as for the depth maps: with
``--noise-px 0.3 --sparse-points 1500`` the poses are off by 0.002 rad and the winners by more than a step on a third of the
pixels (profiles/plane_sweep/README.md).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lib.stereo.depth_maps import (compute_depth_maps, depth_hypotheses, depth_ranges, filter_depth_maps, point_cloud,   # noqa: E402
                                   select_source_views)
from structure_from_motion_amd import synthetic   # noqa: E402


def two_plane_scene(views: int, height: int, width: int, seed: int, step_deg: float) -> dict:
    c, s = np.cos(np.radians(25.0)), np.sin(np.radians(25.0))
    planes = [((0.0, 0.0, 5.0), (c, 0.0, s), (0.0, 1.0, 0.0), None),
              ((0.1, 0.0, 3.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.45, 0.5))]
    poses = synthetic.arc_poses(views, step_deg, 5.0)
    scene = synthetic.plane_views(height, width, poses, planes, seed=seed)
    scene["poses"] = poses
    return scene


def sparse_observations(scene, points: int, noise_px: float, seed: int) -> dict:
    """``points`` surface points, drawn as random pixels of random views, observed in every view that sees them unoccluded, with
    Gaussian pixel noise: the observation lists a reconstruction starts from (the layout of ``synthetic.multi_view_scene``)."""
    rng = np.random.default_rng(seed)
    K, poses, depth = scene["K"], scene["poses"], scene["depth"]
    V, H, W = depth.shape
    v, y, x = rng.integers(0, V, points), rng.integers(0, H, points), rng.integers(0, W, points)
    d = depth[v, y, x]
    rays = np.column_stack([x, y, np.ones(points)]) @ np.linalg.inv(K).T * d[:, None]
    R, t = poses[v, :9].reshape(-1, 3, 3), poses[v, 9:]
    X = np.einsum("pji,pj->pi", R, rays - t)
    X = X[np.isfinite(d)]
    cams, pts, pixels = [], [], []
    for i in range(V):
        xc = X @ poses[i, :9].reshape(3, 3).T + poses[i, 9:]
        uv = (xc @ K.T)[:, :2] / xc[:, 2:3]
        xi, yi = np.rint(uv[:, 0]).astype(np.int64), np.rint(uv[:, 1]).astype(np.int64)
        inside = (xc[:, 2] > 0) & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        seen = inside.copy()
        seen[inside] = np.abs(depth[i, yi[inside], xi[inside]] - xc[inside, 2]) < 0.02 * xc[inside, 2]   # not hidden by the front plane
        at = np.nonzero(seen)[0]
        cams.append(np.full(len(at), i))
        pts.append(at)
        pixels.append(uv[at] + rng.normal(0.0, noise_px, (len(at), 2)))
    cam, pt, pix = np.concatenate(cams), np.concatenate(pts), np.vstack(pixels)
    keep = np.bincount(pt, minlength=len(X))[pt] >= 2
    return dict(K=K, camera_indices=cam[keep].astype(np.int32), point_indices=pt[keep].astype(np.int32), pixels=pix[keep],
                poses_true=poses, points_true=X)


def model_of(scene, points: int, noise_px: float, seed: int) -> dict:
    """Poses, depth ranges and sources from a sparse reconstruction of the scene, and the factor from the true scale to its own."""
    from apps.merge_reconstructions import baseline, reconstruct
    from structure_from_motion_amd import device

    random.seed(seed)   # the RANSAC stages of the reconstruction draw from Python's generator
    sparse = sparse_observations(scene, points, noise_px, seed)
    focal = float(scene["K"][0, 0])
    rec = reconstruct(sparse, sed_threshold=(3.0 * max(noise_px, 0.1) / focal) ** 2, reprojection_threshold=(4.0 * max(noise_px, 0.25)) ** 2,
                      iterations=1000, refine_steps=10, ba_steps=20, final_ba_steps=50)
    V = len(scene["poses"])
    if len(rec.registered) < V:
        raise RuntimeError(f"the sparse reconstruction registered {len(rec.registered)} of {V} views")
    use = rec.active & (rec.status[rec.pt] == device.TRACKS_OK)
    near, far = depth_ranges(rec.poses, np.nan_to_num(rec.X), rec.cam[use], rec.pt[use], margin=0.1)
    sources = select_source_views(rec.cam[use], rec.pt[use], V, min(4, V - 1))
    scale = baseline(rec.poses, 0, 1) / baseline(scene["poses"], 0, 1)
    return dict(poses=rec.poses, near=near, far=far, sources=sources, scale=scale, points=int(np.sum(rec.status == device.TRACKS_OK)))


def _median(values) -> float | None:
    return float(np.median(values)) if len(values) else None


def run(views: int = 5, height: int = 120, width: int = 160, depths: int = 64, radius: int = 3, top_k: int = 2, seed: int = 2,
        step_deg: float = 4.0, max_pixel_error: float = 1.0, max_relative_depth_error: float = 0.02, min_consistent: int = 2,
        from_model: bool = False, sparse_points: int = 3000, noise_px: float = 0.1, smooth=None) -> dict:
    if views < 3:
        raise ValueError(f"need at least 3 views, got {views!r}")
    scene = two_plane_scene(views, height, width, seed, step_deg)
    truth = scene["depth"]
    report = {"views": views, "height": height, "width": width, "depths": depths, "radius": radius, "top_k": top_k,
              "from_model": bool(from_model)}
    if from_model:
        model = model_of(scene, sparse_points, noise_px, seed)
        poses, near, far, sources = model["poses"], model["near"], model["far"], model["sources"]
        truth = truth * model["scale"]
        report["model"] = {"points": model["points"], "scale": model["scale"]}
    else:
        poses = scene["poses"]
        near = np.full(views, np.nanmin(truth) / 1.05)
        far = np.full(views, np.nanmax(truth) * 1.05)
        sources = np.array([sorted((u for u in range(views) if u != v), key=lambda u, v=v: (abs(u - v), u))[:4] for v in range(views)],
                           dtype=np.int32)
    z = np.stack([depth_hypotheses(near[v], far[v], depths) for v in range(views)])
    inner = np.zeros((height, width), dtype=bool)
    inner[radius:height - radius, radius:width - radius] = True
    filter_args = (max_pixel_error, max_relative_depth_error, min_consistent)
    report.update(_figures(scene, poses, z, sources, radius, top_k, None, filter_args, truth, inner))
    if smooth is not None:
        report["smoothed"] = {"p1": float(smooth[0]), "p2": float(smooth[1]),
                              **_figures(scene, poses, z, sources, radius, top_k, tuple(smooth), filter_args, truth, inner)}
    return report


def _figures(scene, poses, z, sources, radius, top_k, smoothness, filter_args, truth, inner) -> dict:
    """The depth maps with or without smoothing, the filter and the cloud: the figures of the module docstring."""
    views = len(z)
    maps = compute_depth_maps(scene["images"], scene["K"], poses, z, sources=sources, radius=radius, top_k=top_k, smoothness=smoothness)
    kept = filter_depth_maps(maps, scene["K"], poses, sources, *filter_args)
    points, grey, view = point_cloud(kept)
    report = {"per_view": []}
    for v in range(views):
        with np.errstate(all="ignore"):
            want = np.abs(1.0 / truth[v][..., None] - 1.0 / z[v]).argmin(axis=-1)
        right = (maps.index[v] >= 0) & np.isfinite(truth[v]) & (np.abs(maps.index[v] - want) <= 1)
        stays = np.isfinite(kept.depth[v]) & inner
        with np.errstate(all="ignore"):
            error = np.abs(maps.depth[v] - truth[v]) / truth[v]
        report["per_view"].append({
            "view": v,
            "within_one_before": float((right & inner).sum() / inner.sum()),
            "within_one_after": float((right & stays).sum() / max(int(stays.sum()), 1)),
            "kept": float(stays.sum() / inner.sum()),
            "median_relative_error_before": _median(error[inner & np.isfinite(error)]),
            "median_relative_error_after": _median(error[stays & np.isfinite(error)]),
            "cloud_points": int(np.sum(view == v)),
        })
    report["cloud_points"] = int(len(points))
    report["mean_grey"] = float(grey.mean()) if len(grey) else None
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--height", type=int, default=120)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--depths", type=int, default=64)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--step-deg", type=float, default=4.0)
    ap.add_argument("--max-pixel-error", type=float, default=1.0)
    ap.add_argument("--max-relative-depth-error", type=float, default=0.02)
    ap.add_argument("--min-consistent", type=int, default=2)
    ap.add_argument("--from-model", action="store_true", help="poses, depth ranges and sources from a sparse reconstruction")
    ap.add_argument("--sparse-points", type=int, default=3000)
    ap.add_argument("--noise-px", type=float, default=0.1, help="pixel noise of the sparse observations")
    ap.add_argument("--smooth", type=float, nargs=2, metavar=("P1", "P2"), default=None,
                    help="also report the maps of the cost volume smoothed with these penalties")
    a = ap.parse_args()
    print(json.dumps(run(a.views, a.height, a.width, a.depths, a.radius, a.top_k, a.seed, a.step_deg, a.max_pixel_error,
                         a.max_relative_depth_error, a.min_consistent, a.from_model, a.sparse_points, a.noise_px, a.smooth)))


if __name__ == "__main__":
    main()
