"""Sub-pixel refinement of the tracks of a collection of views that differ by a rotation and a scale.

Views of one texture (``synthetic.similarity_texture_views``) go through the chain: multi-scale keypoints
(``detect_and_describe``), all pairs matched at once (``match_image_pairs`` over ``all_pairs``), every pair verified
(``verify_pairs``), the verified matches linked into tracks (``build_tracks``) and the tracks' observations refined
(``refine_track_observations``).  Every view's pixels map to the canvas by a known similarity, so the distance of an observation
from its track's reference on the canvas measures how well the two look at one surface point.

    python apps/refine_tracks.py --degrees 0 17 45 133 --scales 1 1.25 1.5 2

Prints, per view, the median and the 90th percentile of that distance in canvas pixels before and after the refinement, and
the number of observations per status.  Printed as JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from structure_from_motion_amd import synthetic  # noqa: E402


def canvas_points(xy, to_canvas):
    """Pixels (n, 2) of a view -> canvas coordinates (n, 2)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return xy @ to_canvas[:, :2].T + to_canvas[:, 2]


def reference_distances(pixels, camera_indices, reference, to_canvas):
    """(M,) canvas distance of every observation from its track's reference; NaN for the references themselves."""
    canvas = np.zeros((len(pixels), 2))
    for v, A in enumerate(to_canvas):
        mine = camera_indices == v
        canvas[mine] = canvas_points(pixels[mine], A)
    target = np.where(reference >= 0, reference, 0)
    distance = np.linalg.norm(canvas - canvas[target], axis=1)
    return np.where(reference >= 0, distance, np.nan)


def run(degrees=(0.0, 17.0, 45.0, 133.0), scales=(1.0, 1.25, 1.5, 2.0), height: int = 240, width: int = 320, features: int = 1000,
        threshold: int = 20, seed: int = 7, noise: float = 0.01, levels: int = 8, inlier_threshold: float = 1e-5,
        iterations: int = 500, radius: int = 7, max_iterations: int = 10, min_correlation: float = 0.8, details: bool = False):
    """The JSON record; with ``details`` also (images, keypoints, ``TrackBuildResult``, ``TrackRefinement``)."""
    from lib.epipolar.view_graph import verify_pairs
    from lib.feature_matching.graph_matching import all_pairs, match_image_pairs
    from lib.feature_matching.keypoints import detect_and_describe
    from lib.multiview.track_refinement import refine_track_observations
    from lib.multiview.tracks import build_tracks
    from structure_from_motion_amd.multiview.track_refinement import STATUS_NAMES

    images, to_canvas = synthetic.similarity_texture_views(height, width, degrees, scales, seed, noise)
    pairs = all_pairs(len(images))
    # rotation and scale about the principal point: a pure camera rotation with a change of focal length, a homography
    K = np.array([[float(width), 0.0, (width - 1) / 2.0], [0.0, float(width), (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    keypoints = detect_and_describe(images, num_features=features, levels=levels, threshold=threshold)
    matched = match_image_pairs([k.descriptors for k in keypoints], pairs)
    graph = verify_pairs(K, [k.xy for k in keypoints], pairs, matched.matches, inlier_threshold, min_extra_fraction=0.4,
                         max_iterations=iterations, seed=seed)
    tracks = build_tracks([k.xy for k in keypoints], pairs, graph.inlier_matches)
    refined = refine_track_observations(images, keypoints, tracks, radius=radius, max_iterations=max_iterations,
                                        min_correlation=min_correlation, levels=levels)
    before = reference_distances(tracks.pixels, tracks.camera_indices, refined.reference, to_canvas)
    after = reference_distances(refined.pixels, tracks.camera_indices, refined.reference, to_canvas)
    out = dict(height=height, width=width, degrees=[float(d) for d in degrees], scales=[float(s) for s in scales], features=features,
               seed=seed, noise=noise, levels=levels, radius=radius, max_iterations=max_iterations, min_correlation=min_correlation,
               tracks=int(tracks.info.tracks), observations=int(len(tracks.camera_indices)), views=[])
    for v in range(len(images)):
        mine = (tracks.camera_indices == v) & (refined.reference >= 0)
        entry = dict(view=v, observations=int(np.count_nonzero(mine)))
        if entry["observations"]:
            entry.update(median_before=float(np.median(before[mine])), p90_before=float(np.percentile(before[mine], 90)),
                         median_after=float(np.median(after[mine])), p90_after=float(np.percentile(after[mine], 90)))
        out["views"].append(entry)
    counts = np.bincount(refined.status, minlength=len(STATUS_NAMES))
    out["status"] = {name: int(count) for name, count in zip(STATUS_NAMES, counts)}
    moved = refined.status == 0
    out["mean_iterations"] = float(refined.iterations[refined.reference >= 0].mean()) if np.any(refined.reference >= 0) else 0.0
    out["refined_share"] = float(np.count_nonzero(moved) / max(1, np.count_nonzero(refined.reference >= 0)))
    if details:
        return out, (images, keypoints, tracks, refined)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--degrees", type=float, nargs="+", default=[0.0, 17.0, 45.0, 133.0])
    ap.add_argument("--scales", type=float, nargs="+", default=[1.0, 1.25, 1.5, 2.0])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--threshold", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--max-iterations", type=int, default=10)
    ap.add_argument("--min-correlation", type=float, default=0.8)
    args = ap.parse_args()
    print(json.dumps(run(args.degrees, args.scales, args.height, args.width, args.features, args.threshold, args.seed, args.noise,
                         args.levels, radius=args.radius, max_iterations=args.max_iterations,
                         min_correlation=args.min_correlation), indent=1))
