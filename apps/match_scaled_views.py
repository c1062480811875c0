"""Views of one object from different distances, matched with single-scale and with multi-scale keypoints: per image pair the
matches kept and how many of them are right, for ``levels=1`` and for ``levels=8``.

Every stage is one device call over the whole collection: keypoints and descriptors (``detect_and_describe``), all pairs
matched at once (``match_image_pairs`` over ``all_pairs``) and every pair verified (``verify_pairs``).  The scene is
``synthetic.similarity_texture_views``: one multi-scale random texture seen rotated and scaled about the image centre.  A
match is right iff its two ends lie within 3 x the larger of their footprints of each other on the canvas; the footprint of a
keypoint is scale of its view x 1.25^level canvas pixels.  Printed as JSON.

    python apps/match_scaled_views.py --scales 1 1.5 2 --degrees 0 45 133
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


def count_right(matches, xy_a, level_a, scale_a, to_canvas_a, xy_b, level_b, scale_b, to_canvas_b) -> int:
    """How many of ``matches`` ((n, 2) indices into the two keypoint lists) join two keypoints of one canvas point."""
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    a, b = matches[:, 0], matches[:, 1]
    apart = np.linalg.norm(canvas_points(xy_a, to_canvas_a)[a] - canvas_points(xy_b, to_canvas_b)[b], axis=1)
    footprint = np.maximum(scale_a * 1.25 ** np.asarray(level_a, dtype=np.float64)[a],
                           scale_b * 1.25 ** np.asarray(level_b, dtype=np.float64)[b])
    return int(np.count_nonzero(apart <= 3.0 * footprint))


def run(degrees=(0.0, 45.0, 133.0), scales=(1.0, 1.5, 2.0), height: int = 480, width: int = 640, features: int = 1000,
        threshold: int = 20, seed: int = 7, noise: float = 0.01, levels=(1, 8), inlier_threshold: float = 1e-5,
        iterations: int = 500, images=None, to_canvas=None):
    """The JSON record.  ``images`` / ``to_canvas``: views made before (the generator's output for the other arguments)."""
    from lib.epipolar.view_graph import verify_pairs
    from lib.feature_matching.graph_matching import all_pairs, match_image_pairs
    from lib.feature_matching.keypoints import detect_and_describe

    if images is None:
        images, to_canvas = synthetic.similarity_texture_views(height, width, degrees, scales, seed, noise)
    pairs = all_pairs(len(images))
    # rotation and scale about the principal point: a pure camera rotation with a change of focal length, a homography
    K = np.array([[float(width), 0.0, (width - 1) / 2.0], [0.0, float(width), (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    out = dict(height=height, width=width, degrees=[float(d) for d in degrees], scales=[float(s) for s in scales],
               features=features, threshold=threshold, seed=seed, noise=noise, runs=[])
    for count in levels:
        keypoints = detect_and_describe(images, num_features=features, levels=count, threshold=threshold)
        matched = match_image_pairs([k.descriptors for k in keypoints], pairs)
        graph = verify_pairs(K, [k.xy for k in keypoints], pairs, matched.matches, inlier_threshold, min_extra_fraction=0.4,
                             max_iterations=iterations, seed=seed)
        record = dict(levels=int(count), keypoints=[int(len(k.xy)) for k in keypoints], pairs=[])
        for q, (i, j) in enumerate(pairs.tolist()):
            right = count_right(matched.matches[q], keypoints[i].xy, keypoints[i].level, scales[i], to_canvas[i],
                                keypoints[j].xy, keypoints[j].level, scales[j], to_canvas[j])
            kind = graph.kind[q]
            inliers = int(graph.homography_count[q] if kind == "homography" else graph.essential_count[q] if kind == "essential" else 0)
            record["pairs"].append(dict(images=[i, j], kept=int(len(matched.matches[q])), right=right, kind=kind, inliers=inliers))
        out["runs"].append(record)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--degrees", type=float, nargs="+", default=[0.0, 45.0, 133.0])
    ap.add_argument("--scales", type=float, nargs="+", default=[1.0, 1.5, 2.0])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--threshold", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    print(json.dumps(run(args.degrees, args.scales, args.height, args.width, args.features, args.threshold, args.seed, args.noise,
                         tuple(args.levels)), indent=1))
