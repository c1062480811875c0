"""From the images of a collection to verified tracks, every stage one device call over the whole match graph: BRIEF
descriptors per view (``compute_brief``), all pairs matched at once (``match_image_pairs`` over ``all_pairs``), every pair
verified (``verify_pairs``) and the verified matches linked into tracks (``build_tracks``).

The scene is ``synthetic.rotated_texture_views``: views of one band-limited random texture rotated about the image centre,
with features every view sees and partnerless ones per view.  Printed as JSON: per pair the matches kept, their precision
and recall against the ground truth, the kind of two-view model and its inlier count (an in-plane rotation is a
homography), and overall the share of the built tracks that hold one latent point.

``--guided`` adds the second matching pass after the verification (``guided_match_pairs``: each pair's search repeated among the
partners its verified model admits), verifies its result and builds the tracks on that; kept, precision and recall are then
printed per pair before and after.  ``--scene repeated`` runs the chain on ``synthetic.repeated_structure_views`` — views on an
arc around a box of points, part of which look alike — whose pairs are essential matrices, instead of the texture views.

    python apps/match_image_collection.py --degrees 0 17 45 90
    python apps/match_image_collection.py --scene repeated --guided
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lib.epipolar.view_graph import verify_pairs
from lib.feature_matching.brief import compute_brief
from lib.feature_matching.graph_matching import all_pairs, match_image_pairs
from lib.feature_matching.guided_matching import guided_match_pairs
from lib.multiview.tracks import build_tracks
from structure_from_motion_amd import synthetic


def precision_recall(matches, ids_a, ids_b, common: int):
    """(precision, recall) of one pair's matches: a match is right when both ends are the same latent point."""
    right = int(np.count_nonzero((ids_a[matches[:, 0]] >= 0) & (ids_a[matches[:, 0]] == ids_b[matches[:, 1]])))
    return (right / len(matches) if len(matches) else 0.0), (right / common if common else 0.0)


def run(degrees=(0.0, 17.0, 45.0, 90.0), height: int = 240, width: int = 320, features: int = 200, extra: int = 60,
        seed: int = 7, noise: float = 0.01, max_distance: int = 64, ratio=0.8, cross_check: bool = True,
        inlier_threshold: float = 1e-5, iterations: int = 500, details: bool = False, scene: str = "texture",
        guided: bool = False, views: int = 4, unique: int | None = None, groups: int = 30):
    """The JSON record; with ``details`` also (descriptors per view, ``PairMatches``, ``ViewGraph``, ``TrackBuildResult``) —
    with ``guided`` or ``scene="repeated"`` followed by (the guided ``PairMatches`` or None, the pixels per view, K, the
    ``ViewGraph`` of the first pass), and the graph and the tracks before them are then those of the last pass."""
    if scene not in ("texture", "repeated"):
        raise ValueError(f"scene must be 'texture' or 'repeated', got {scene!r}")
    repeated = scene == "repeated"
    if repeated:
        unique = features * 5 // 8 if unique is None else unique
        sc = synthetic.repeated_structure_views(views, features, unique, groups, extra, seed)
        descriptors, feats, ids, K = sc["descriptors"], sc["pixels"], sc["ids"], sc["K"]
    else:
        images, feats, ids = synthetic.rotated_texture_views(height, width, degrees, features, extra, seed, noise)
        descriptors = [compute_brief(image, f) for image, f in zip(images, feats)]
        # the rotation is about the principal point: a pure camera rotation
        K = np.array([[float(width), 0.0, (width - 1) / 2.0], [0.0, float(width), (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    pairs = all_pairs(len(feats))
    matched = match_image_pairs(descriptors, pairs, max_distance=max_distance, ratio=ratio, cross_check=cross_check)
    pose = dict(relative_pose=True, refine_pose_rounds=2) if repeated and guided else {}
    graph = verify_pairs(K, feats, pairs, matched.matches, inlier_threshold, min_extra_fraction=0.4, max_iterations=iterations,
                         seed=seed, **pose)
    second, first_graph = None, graph
    if guided:
        second = guided_match_pairs(descriptors, feats, K, graph, inlier_threshold, use_pose=bool(pose),
                                    max_distance=max_distance, ratio=ratio, cross_check=cross_check)
        graph = verify_pairs(K, feats, pairs, second.matches, inlier_threshold, min_extra_fraction=0.4,
                                                 max_iterations=iterations, seed=seed, **pose)
    tracks = build_tracks(feats, pairs, graph.inlier_matches)
    truth = np.concatenate(ids)[tracks.feature_indices]
    lo = np.full(tracks.info.tracks, np.iinfo(np.int64).max)
    hi = np.full(tracks.info.tracks, -1)
    np.minimum.at(lo, tracks.point_indices, truth)
    np.maximum.at(hi, tracks.point_indices, truth)
    out = dict(height=height, width=width, degrees=[float(d) for d in degrees], features=features, extra=extra, seed=seed,
               noise=noise, max_distance=max_distance, ratio=ratio, cross_check=cross_check, pairs=[],
               tracks=int(tracks.info.tracks),
               pure_track_share=float(np.mean((lo == hi) & (lo >= 0))) if tracks.info.tracks else float("nan"))
    if repeated:
        for name in ("height", "width", "degrees", "noise"):
            del out[name]
        out.update(scene=scene, views=views, unique=unique, groups=groups)
    if guided:
        out["guided"] = True

    def model_entry(g, q):
        model = g.kind[q]
        inliers = int(g.homography_count[q] if model == "homography" else g.essential_count[q] if model == "essential" else 0)
        return dict(kind=model, inliers=inliers, homography_count=int(g.homography_count[q]),
                    essential_count=int(g.essential_count[q]))

    for q, (i, j) in enumerate(pairs.tolist()):
        common = len(np.intersect1d(ids[i][ids[i] >= 0], ids[j][ids[j] >= 0])) if repeated else features
        precision, recall = precision_recall(matched.matches[q], ids[i], ids[j], common)
        entry = dict(images=[i, j], kept=int(len(matched.matches[q])), precision=precision, recall=recall,
                     **model_entry(first_graph, q))
        if repeated:
            entry["common"] = common
        if guided:
            precision, recall = precision_recall(second.matches[q], ids[i], ids[j], common)
            entry["guided"] = dict(kept=int(len(second.matches[q])), precision=precision, recall=recall, **model_entry(graph, q))
        out["pairs"].append(entry)
    if not details:
        return out
    if guided or repeated:
        return out, (descriptors, matched, graph, tracks, second, feats, K, first_graph)
    return out, (descriptors, matched, graph, tracks)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--degrees", type=float, nargs="+", default=[0.0, 17.0, 45.0, 90.0])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--features", type=int, default=200)
    ap.add_argument("--extra", type=int, default=60)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--max-distance", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.8, help="Lowe's ratio; 0 or less switches the test off")
    ap.add_argument("--no-cross-check", action="store_true")
    ap.add_argument("--guided", action="store_true", help="add the guided second pass after the verification")
    ap.add_argument("--scene", choices=["texture", "repeated"], default="texture")
    ap.add_argument("--views", type=int, default=4, help="views of --scene repeated")
    ap.add_argument("--unique", type=int, default=None, help="points of --scene repeated with a descriptor of their own")
    ap.add_argument("--groups", type=int, default=30, help="look-alike groups of --scene repeated")
    ap.add_argument("--inlier-threshold", type=float, default=None)
    args = ap.parse_args()
    threshold = args.inlier_threshold if args.inlier_threshold is not None else (6e-6 if args.scene == "repeated" else 1e-5)
    print(json.dumps(run(args.degrees, args.height, args.width, args.features, args.extra, args.seed, args.noise,
                         args.max_distance, args.ratio if args.ratio > 0 else None, not args.no_cross_check,
                         inlier_threshold=threshold, scene=args.scene, guided=args.guided, views=args.views,
                         unique=args.unique, groups=args.groups), indent=1))
