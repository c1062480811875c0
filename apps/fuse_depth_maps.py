"""A surface from posed images: the two-plane scene of ``apps/depth_maps.py`` through plane-sweep stereo, the consistency filter
and the fusion of all depth maps into a TSDF volume whose zero level set is extracted as a triangle mesh, all on the GPU
(``lib.stereo.depth_maps``, ``lib.stereo.fusion``).

V views on an arc see a slanted textured plane and a smaller plane in front of it.  The depth maps of all views are computed by
one ``compute_depth_maps`` call and filtered by one ``filter_depth_maps`` call; the volume is laid around the kept points
(``volume_bounds``) with voxels of ``--pixels`` pixel footprints at the median depth (``suggest_voxel_size``), every map is
averaged into it (``TsdfVolume.integrate``) and the mesh taken over the cells that at least ``--min-count`` views saw.

Printed as JSON: the number of triangles and of welded points, the share of the volume's cells that are valid, the mean and the
largest distance of the mesh's points to the nearest of the two true planes, in voxels, and the share of the triangles whose
normal faces the middle camera.  ``--ply PATH`` writes the welded mesh with its grey values.

``--smooth P1 P2`` adds the same figures under ``"smoothed"`` for the surface fused from the depth maps whose cost volume was
smoothed with these penalties (``compute_depth_maps(..., smoothness=(P1, P2))``).

``--from-model`` takes the poses, depth ranges and sources from a sparse reconstruction, as in ``apps/depth_maps.py``; the mesh
is brought back from the model's gauge into the scene's for the comparison only."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apps.depth_maps import model_of, two_plane_scene   # noqa: E402
from lib.stereo.depth_maps import compute_depth_maps, depth_hypotheses, filter_depth_maps   # noqa: E402
from lib.stereo.fusion import TsdfVolume, save_ply, suggest_voxel_size, volume_bounds   # noqa: E402

SLANT = (np.cos(np.radians(25.0)), 0.0, np.sin(np.radians(25.0)))


def distance_to_planes(points: np.ndarray) -> np.ndarray:
    """The distance of every point to the nearest of the scene's two planes: the unbounded slanted one through (0, 0, 5) and the
    rectangle |x - 0.1| <= 0.45, |y| <= 0.5 at z = 3.6."""
    normal = np.cross(SLANT, (0.0, 1.0, 0.0))
    slanted = np.abs((points - np.array([0.0, 0.0, 5.0])) @ normal)
    off = np.stack([np.maximum(np.abs(points[:, 0] - 0.1) - 0.45, 0.0), np.maximum(np.abs(points[:, 1]) - 0.5, 0.0), points[:, 2] - 3.6], axis=1)
    return np.minimum(slanted, np.linalg.norm(off, axis=1))


def run(views: int = 5, height: int = 120, width: int = 160, depths: int = 64, radius: int = 3, top_k: int = 2, seed: int = 2,
        step_deg: float = 4.0, max_pixel_error: float = 1.0, max_relative_depth_error: float = 0.02, min_consistent: int = 2,
        pixels: float = 2.0, truncation_voxels: float = 4.0, min_count: int = 2, from_model: bool = False, sparse_points: int = 3000,
        noise_px: float = 0.1, ply: str | None = None, smooth=None) -> dict:
    if views < 3:
        raise ValueError(f"need at least 3 views, got {views!r}")
    scene = two_plane_scene(views, height, width, seed, step_deg)
    truth = scene["depth"]
    scale = 1.0
    report = {"views": views, "height": height, "width": width, "depths": depths, "from_model": bool(from_model)}
    if from_model:
        model = model_of(scene, sparse_points, noise_px, seed)
        poses, near, far, sources, scale = model["poses"], model["near"], model["far"], model["sources"], model["scale"]
        report["model"] = {"points": model["points"], "scale": scale}
    else:
        poses = scene["poses"]
        near = np.full(views, np.nanmin(truth) / 1.05)
        far = np.full(views, np.nanmax(truth) * 1.05)
        sources = np.array([sorted((u for u in range(views) if u != v), key=lambda u, v=v: (abs(u - v), u))[:4] for v in range(views)],
                           dtype=np.int32)
    z = np.stack([depth_hypotheses(near[v], far[v], depths) for v in range(views)])
    filter_args = (max_pixel_error, max_relative_depth_error, min_consistent)
    fusion_args = (pixels, truncation_voxels, min_count)
    report.update(_surface(scene, poses, z, sources, radius, top_k, None, filter_args, fusion_args, scale, ply))
    if smooth is not None:
        report["smoothed"] = {"p1": float(smooth[0]), "p2": float(smooth[1]),
                              **_surface(scene, poses, z, sources, radius, top_k, tuple(smooth), filter_args, fusion_args, scale, None)}
    return report


def _surface(scene, poses, z, sources, radius, top_k, smoothness, filter_args, fusion_args, scale, ply) -> dict:
    """The depth maps with or without smoothing, the filter, the fusion and the mesh: the figures of the module docstring."""
    views = len(z)
    pixels, truncation_voxels, min_count = fusion_args
    maps = compute_depth_maps(scene["images"], scene["K"], poses, z, sources=sources, radius=radius, top_k=top_k, smoothness=smoothness)
    kept = filter_depth_maps(maps, scene["K"], poses, sources, *filter_args)
    voxel = suggest_voxel_size(kept, scene["K"], pixels)
    truncation = truncation_voxels * voxel
    low, high = volume_bounds(kept, truncation)
    dims = np.maximum(np.ceil((high - low) / voxel).astype(np.int64), 2)
    volume = TsdfVolume(low, voxel, dims, truncation, with_grey=True)
    volume.integrate(kept.depth, scene["K"], poses, images=scene["images"])
    mesh = volume.extract_mesh(min_count)
    if ply:
        save_ply(ply, mesh)
    points, faces, _ = mesh.weld()
    count = volume.to_host()[1] >= min_count
    cells = (count[:-1, :-1, :-1] & count[:-1, :-1, 1:] & count[:-1, 1:, :-1] & count[:-1, 1:, 1:] &
             count[1:, :-1, :-1] & count[1:, :-1, 1:] & count[1:, 1:, :-1] & count[1:, 1:, 1:])
    # into the scene's gauge: through the first camera, whose frame the two gauges share up to the scale
    first, first_true = poses[0], scene["poses"][0]

    def to_scene(X):
        camera = (X @ first[:9].reshape(3, 3).T + first[9:]) / scale
        return (camera - first_true[9:]) @ first_true[:9].reshape(3, 3)

    where = to_scene(points) if len(points) else np.zeros((0, 3))
    distance = distance_to_planes(where) / (voxel / scale)
    middle = scene["poses"][views // 2]
    centre = -middle[:9].reshape(3, 3).T @ middle[9:]
    corners = to_scene(mesh.vertices.reshape(-1, 3)).reshape(-1, 3, 3)
    normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    facing = np.einsum("ij,ij->i", normal, centre - corners.mean(axis=1)) > 0
    return {"voxel_size": voxel, "dims": [int(d) for d in dims], "triangles": int(len(faces)), "points": int(len(points)),
            "valid_cells": float(cells.mean()),
            "mean_distance_voxels": float(distance.mean()) if len(distance) else None,
            "max_distance_voxels": float(distance.max()) if len(distance) else None,
            "normals_facing_cameras": float(facing.mean()) if len(facing) else None}


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
    ap.add_argument("--pixels", type=float, default=2.0, help="voxel size in pixel footprints at the median depth")
    ap.add_argument("--truncation-voxels", type=float, default=4.0)
    ap.add_argument("--min-count", type=int, default=2, help="views that must have seen every corner of a cell")
    ap.add_argument("--from-model", action="store_true", help="poses, depth ranges and sources from a sparse reconstruction")
    ap.add_argument("--sparse-points", type=int, default=3000)
    ap.add_argument("--noise-px", type=float, default=0.1, help="pixel noise of the sparse observations")
    ap.add_argument("--ply", default=None, help="write the welded mesh to this PLY file")
    ap.add_argument("--smooth", type=float, nargs=2, metavar=("P1", "P2"), default=None,
                    help="also report the surface of the depth maps smoothed with these penalties")
    a = ap.parse_args()
    print(json.dumps(run(a.views, a.height, a.width, a.depths, a.radius, a.top_k, a.seed, a.step_deg, a.max_pixel_error,
                         a.max_relative_depth_error, a.min_consistent, a.pixels, a.truncation_voxels, a.min_count, a.from_model,
                         a.sparse_points, a.noise_px, a.ply, a.smooth)))


if __name__ == "__main__":
    main()
