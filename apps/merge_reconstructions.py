"""Merge two reconstructions of overlapping view ranges with a RANSAC similarity alignment on the GPU.

From one synthetic N-view scene, two overlapping ranges of views are reconstructed independently, each by the incremental
route of ``apps/sfm_multi_view.py`` (seed pair, PnP chain, bundle adjustment): each gets the gauge of its own seed pair — its
first view at the identity, its seed baseline as the unit.  The tracks that stand in both are the 3-D / 3-D pairs from which
``estimate_similarity_with_ransac`` aligns B onto A; B's poses and points are carried over, united with A's, and one final
bundle adjustment runs over everything.

Printed as JSON: the common tracks and the inliers among them, the recovered scale against the ratio of the two true seed
baselines, the alignment RMS, and the per-view pose errors of the merged model against the truth (in A's gauge: relative to A's
first view, in units of A's true seed baseline) before and after the final adjustment, next to those of the two halves on their
own.  ``--corrupt FRACTION`` displaces that share of B's common points before the alignment and prints the plain least-squares
``fit_similarity`` over all pairs next to the RANSAC result: what the robust estimate buys.

``--parts K`` with K > 2 reconstructs K overlapping view ranges along the arc instead, aligns every pair of parts that share at
least 30 standing tracks in ONE ``align_models`` call, puts the parts into the frame of the first with
``merge_frames`` and runs one final adjustment over the union (the iterative solver above 64 cameras, as
``apps/sfm_multi_view.py`` chooses it).  Each pair's threshold is ``--align-threshold`` in the unit of its side B, that part's own
seed baseline, and ``--corrupt`` displaces that share of every pair's side-A points.  Printed then: per pair the common tracks,
the inliers, the displaced points among them and the scale error against the ratio of the two true seed baselines; the
disagreement of every pair with the frames (the loops); the worst pose error of the merged model before and after the
adjustment, next to each part's own.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apps.sfm_multi_view import MIN_PNP_INLIERS, Reconstruction, _errors, _pose, rotation_angle   # noqa: E402
from lib.bundle.bundle import bundle_adjust   # noqa: E402
from lib.common.feature import Feature   # noqa: E402
from lib.epipolar.eight_point import create_trivial_matches, recover_r_t_from_e   # noqa: E402
from lib.epipolar.epipolar_ransac import estimate_essential_mat_with_ransac   # noqa: E402
from lib.feature_matching.matching import Match   # noqa: E402
from lib.multiview.alignment import (align_models, apply_similarity, estimate_similarity_with_ransac,   # noqa: E402
                                     fit_similarity, inconsistent_alignments, merge_frames, transform_poses)
from lib.pnp.pnp import estimate_pose_pnp_with_ransac   # noqa: E402
from structure_from_motion_amd import device, synthetic   # noqa: E402

MIN_COMMON_TRACKS = 30   # a pair of parts is aligned when it shares at least this many standing tracks
DENSE_MAX_VIEWS = 64     # the dense bundle adjuster's camera limit (apps/sfm_multi_view.py)


def sub_scene(scene, first: int, last: int) -> dict:
    """The observations of views first .. last - 1 with the cameras re-indexed from 0; the tracks keep their indices."""
    cam = scene["camera_indices"]
    keep = (cam >= first) & (cam < last)
    return dict(K=scene["K"], camera_indices=(cam[keep] - first).astype(np.int32), point_indices=scene["point_indices"][keep],
                pixels=scene["pixels"][keep], poses_true=scene["poses_true"][first:last])


def reconstruct(scene, sed_threshold: float, reprojection_threshold: float, iterations: int, refine_steps: int, ba_steps: int,
                final_ba_steps: int) -> Reconstruction:
    """The incremental route of apps/sfm_multi_view.py on the scene's views: seed on views 0 and 1, then the view with the most
    observations of standing points by PnP, triangulation and bundle adjustment, to the last view."""
    K = scene["K"]
    rec = Reconstruction(scene, reprojection_threshold, refine_steps, min_angle_deg=1.0)
    cam, pt, uv = rec.cam, rec.pt, rec.uv
    in0, in1 = np.full(rec.P, -1), np.full(rec.P, -1)
    in0[pt[cam == 0]] = np.nonzero(cam == 0)[0]
    in1[pt[cam == 1]] = np.nonzero(cam == 1)[0]
    both = np.nonzero((in0 >= 0) & (in1 >= 0))[0]
    fa = [Feature(float(x), float(y)) for x, y in uv[in0[both]]]
    fb = [Feature(float(x), float(y)) for x, y in uv[in1[both]]]
    e, pairs = estimate_essential_mat_with_ransac(K, fa, fb, create_trivial_matches(len(both)), sed_inlier_threshold=sed_threshold,
                                                  min_num_extra_inliers=int(0.4 * len(both)), max_iterations=iterations)
    R1, t1, _ = recover_r_t_from_e(e, K, [p[0] for p in pairs], [p[1] for p in pairs])
    index_of = {(f.x, f.y): k for k, f in enumerate(fa)}
    kept = both[sorted(index_of[(p[0].x, p[0].y)] for p in pairs)]
    rec.poses[0], rec.poses[1] = _pose(np.eye(3), np.zeros(3)), _pose(R1, t1)
    rec.registered = [0, 1]
    rec.start(np.nonzero(np.isin(pt, kept) & (cam <= 1))[0], final_ba_steps)
    while len(rec.registered) < rec.views:
        use = rec.active & (rec.status[pt] == device.TRACKS_OK)
        counts = np.bincount(cam[use], minlength=rec.views)
        counts[rec.registered] = -1
        v = int(np.argmax(counts))
        obs = np.nonzero(use & (cam == v))[0]
        if len(obs) < MIN_PNP_INLIERS:
            break
        try:
            R, t, inliers = estimate_pose_pnp_with_ransac(K, [rec.X[p] for p in pt[obs]], [Feature(float(x), float(y)) for x, y in uv[obs]],
                                                          [Match(a_index=i, b_index=i) for i in range(len(obs))],
                                                          reprojection_threshold, min_num_extra_inliers=10,
                                                          max_iterations=iterations, refine_rounds=2)
        except ValueError:
            break
        if len(inliers) < MIN_PNP_INLIERS:
            break
        rec.poses[v] = _pose(R, t)
        rec.registered.append(v)
        rec.triangulate(rec.pending())
        rec.adjust(ba_steps)
    rec.adjust(final_ba_steps)
    return rec


def true_poses_in_gauge(poses_true, origin: int, unit: float):
    """The true poses relative to view `origin`, translations in units of `unit`."""
    Ra, ta = poses_true[origin, :9].reshape(3, 3), poses_true[origin, 9:]
    Rv = np.einsum("vij,kj->vik", poses_true[:, :9].reshape(-1, 3, 3), Ra)   # R_v Ra^T
    return np.hstack([Rv.reshape(-1, 9), (poses_true[:, 9:] - Rv @ ta) / unit])


def pose_errors(poses, truth, views) -> dict:
    return {int(v): {"rotation_rad": rotation_angle(poses[v, :9].reshape(3, 3), truth[v, :9].reshape(3, 3)),
                     "translation": float(np.linalg.norm(poses[v, 9:] - truth[v, 9:]))} for v in views}


def baseline(poses_true, a: int, b: int) -> float:
    centre = lambda v: -poses_true[v, :9].reshape(3, 3).T @ poses_true[v, 9:]   # noqa: E731
    return float(np.linalg.norm(centre(a) - centre(b)))


def summary(errors: dict) -> dict:
    return {"max_rotation_rad": max(e["rotation_rad"] for e in errors.values()),
            "max_translation": max(e["translation"] for e in errors.values())}


def run(views: int = 12, overlap: int = 4, points: int = 2000, seed: int = 21, noise_px: float = 0.5, outlier_fraction: float = 0.2,
        corrupt: float = 0.0, align_threshold: float = 0.05, align_iterations: int = 1000, sed_threshold: float = 6e-6,
        reprojection_threshold: float = 16.0, iterations: int = 2000, refine_steps: int = 10, ba_steps: int = 20,
        final_ba_steps: int = 50, step_deg: float = 5.0, parts: int = 2) -> dict:
    if not 0.0 <= corrupt < 1.0:
        raise ValueError(f"corrupt must be a fraction in [0, 1), got {corrupt!r}")
    if isinstance(parts, bool) or not isinstance(parts, (int, np.integer)) or parts < 2:
        raise ValueError(f"parts must be an integer >= 2, got {parts!r}")
    if parts > 2:
        return run_parts(parts, views, overlap, points, seed, noise_px, outlier_fraction, corrupt, align_threshold, align_iterations,
                         (sed_threshold, reprojection_threshold, iterations, refine_steps, ba_steps, final_ba_steps), step_deg)
    if not (4 <= views <= 64 and 2 <= overlap <= views - 2 and (views + overlap) // 2 >= 3):
        raise ValueError(f"need 4 <= views <= 64 and 2 <= overlap <= views - 2, got views={views}, overlap={overlap}")
    if not (np.isfinite(align_threshold) and align_threshold > 0.0):
        raise ValueError(f"align_threshold must be a positive length in A's units, got {align_threshold!r}")
    scene = synthetic.multi_view_scene(views, points, seed, noise_px, outlier_fraction, step_deg=step_deg)
    last_a = (views + overlap) // 2      # A: views 0 .. last_a - 1;  B: views first_b .. views - 1
    first_b = last_a - overlap
    random.seed(seed)
    options = (sed_threshold, reprojection_threshold, iterations, refine_steps, ba_steps, final_ba_steps)
    rec_a = reconstruct(sub_scene(scene, 0, last_a), *options)
    rec_b = reconstruct(sub_scene(scene, first_b, views), *options)
    truth = scene["poses_true"]
    unit_a, unit_b = baseline(truth, 0, 1), baseline(truth, first_b, first_b + 1)
    truth_a = true_poses_in_gauge(truth, 0, unit_a)
    truth_b = true_poses_in_gauge(truth, first_b, unit_b)

    # the tracks that stand in both halves: B's point -> A's point
    P = min(rec_a.P, rec_b.P)
    common = np.nonzero((rec_a.status[:P] == device.TRACKS_OK) & (rec_b.status[:P] == device.TRACKS_OK))[0]
    from_b, onto_a = rec_b.X[common].copy(), rec_a.X[common]
    rng = np.random.default_rng(seed + 1)
    displaced = rng.permutation(len(common))[:int(round(corrupt * len(common)))]
    extent = float(np.max(np.abs(from_b - np.median(from_b, axis=0))))
    from_b[displaced] += rng.uniform(-1.0, 1.0, size=(len(displaced), 3)) * extent
    threshold = align_threshold ** 2
    sim = estimate_similarity_with_ransac(from_b, onto_a, threshold, iterations=align_iterations,
                                          min_num_extra_inliers=max(3, len(common) // 4), seed=seed)
    if sim is None:
        raise ValueError(f"no similarity aligns {len(common)} common tracks within {align_threshold}")
    plain = fit_similarity(from_b, onto_a)
    residual = apply_similarity(sim, from_b[sim.inliers]) - onto_a[sim.inliers]

    # B in A's frame; a view of the overlap keeps A's pose, a track that stands in A keeps A's point
    poses = np.full((views, 12), np.nan)
    poses_b = transform_poses(sim, rec_b.poses)
    poses[first_b + np.array(rec_b.registered)] = poses_b[rec_b.registered]
    poses[rec_a.registered] = rec_a.poses[rec_a.registered]
    registered = np.nonzero(~np.isnan(poses).any(axis=1))[0]
    total = int(scene["point_indices"].max()) + 1
    X = np.full((total, 3), np.nan)
    ok_b = np.nonzero(rec_b.status == device.TRACKS_OK)[0]
    X[ok_b] = apply_similarity(sim, rec_b.X[ok_b])
    ok_a = np.nonzero(rec_a.status == device.TRACKS_OK)[0]
    X[ok_a] = rec_a.X[ok_a]
    before = pose_errors(poses, truth_a, registered)
    plain_poses = transform_poses(plain, rec_b.poses)
    only_b = [int(v) for v in first_b + np.array(rec_b.registered) if v >= last_a]
    plain_errors = pose_errors(np.vstack([np.full((first_b, 12), np.nan), plain_poses]), truth_a, only_b)

    # one final bundle adjustment of the union on the observations that fit it
    cam, pt, uv = scene["camera_indices"], scene["point_indices"], scene["pixels"]
    standing = np.nonzero(~np.isnan(X).any(axis=1))[0]
    cam_slot, pt_slot = np.full(views, -1), np.full(total, -1)
    cam_slot[registered] = np.arange(len(registered))
    pt_slot[standing] = np.arange(len(standing))
    use = np.nonzero((cam_slot[cam] >= 0) & (pt_slot[pt] >= 0))[0]
    use = use[_errors(scene["K"], poses, X, cam[use], pt[use], uv[use]) <= reprojection_threshold]
    adjusted, _, info = bundle_adjust(scene["K"], poses[registered], X[standing], cam_slot[cam[use]], pt_slot[pt[use]], uv[use],
                                      fixed_cameras=(0,), max_steps=final_ba_steps)
    after_poses = poses.copy()
    after_poses[registered] = adjusted
    after = pose_errors(after_poses, truth_a, registered)
    half_a = pose_errors(rec_a.poses, truth_a, rec_a.registered)
    half_b = pose_errors(rec_b.poses, truth_b[first_b:], rec_b.registered)   # B's views count from its own first
    return {
        "views": views,
        "range_a": [0, last_a],
        "range_b": [first_b, views],
        "views_registered": {"a": len(rec_a.registered), "b": len(rec_b.registered), "merged": int(len(registered))},
        "common_tracks": int(len(common)),
        "corrupted": int(len(displaced)),
        "alignment": {
            "inliers": int(len(sim.inliers)),
            "corrupted_among_inliers": int(np.count_nonzero(np.isin(sim.inliers, displaced))),
            "refined": bool(sim.refined),
            "scale": sim.scale,
            "true_baseline_ratio": unit_b / unit_a,
            "scale_error": abs(sim.scale / (unit_b / unit_a) - 1.0),
            "rms": float(np.sqrt(np.mean(np.sum(residual * residual, axis=1)))),
        },
        "fit_similarity_all_pairs": {"scale": plain.scale, "scale_error": abs(plain.scale / (unit_b / unit_a) - 1.0),
                                     "rms": plain.error, "pose_errors_of_b_only_views": summary(plain_errors) if plain_errors else None},
        "halves": {"a": summary(half_a), "b": summary(half_b)},
        "merged_before_adjustment": {"worst": summary(before), "per_view": before},
        "merged_after_adjustment": {"worst": summary(after), "per_view": after, "ba_status": info.status, "ba_observations": int(len(use)),
                                    "rms_px": float(np.sqrt(info.final_cost / len(use))) if len(use) else float("nan")},
    }


def part_ranges(views: int, overlap: int, parts: int):
    """K view ranges [first, last) of equal length along the arc, consecutive ones sharing `overlap` views, the last ending at
    the last view."""
    length = -(-(views + (parts - 1) * overlap) // parts)
    firsts = [min(k * (length - overlap), views - length) for k in range(parts)]
    return [(first, first + length) for first in firsts]


def run_parts(parts: int, views: int, overlap: int, points: int, seed: int, noise_px: float, outlier_fraction: float, corrupt: float,
              align_threshold: float, align_iterations: int, options, step_deg: float) -> dict:
    if not (np.isfinite(align_threshold) and align_threshold > 0.0):
        raise ValueError(f"align_threshold must be a positive length in a part's units, got {align_threshold!r}")
    if overlap < 2 or views < parts * 3:
        raise ValueError(f"need overlap >= 2 and at least {parts * 3} views for {parts} parts, got views={views}, overlap={overlap}")
    ranges = part_ranges(views, overlap, parts)
    length = ranges[0][1] - ranges[0][0]
    if not (overlap + 1 <= length <= DENSE_MAX_VIEWS) or any(a[0] >= b[0] for a, b in zip(ranges, ranges[1:])):
        raise ValueError(f"{parts} parts of {views} views with {overlap} in common are ranges of {length} views: need "
                         f"{overlap + 1} to {DENSE_MAX_VIEWS}, each starting behind the one before")
    scene = synthetic.multi_view_scene(views, points, seed, noise_px, outlier_fraction, step_deg=step_deg)
    random.seed(seed)
    recs = [reconstruct(sub_scene(scene, first, last), *options) for first, last in ranges]
    truth = scene["poses_true"]
    units = [baseline(truth, first, first + 1) for first, _ in ranges]
    total = int(scene["point_indices"].max()) + 1
    standing = [np.nonzero(rec.status == device.TRACKS_OK)[0] for rec in recs]

    # every pair of parts that shares enough standing tracks; side A of pair q is a copy of part i's common points, so that
    # --corrupt can displace a share of them pair by pair: model parts + q of the call
    clouds, ids = [rec.X[ok] for rec, ok in zip(recs, standing)], list(standing)
    pairs, displaced = [], []
    rng = np.random.default_rng(seed + 1)
    for i in range(parts):
        for j in range(i + 1, parts):
            common = np.intersect1d(standing[i], standing[j])
            if len(common) < MIN_COMMON_TRACKS:
                continue
            side_a = recs[i].X[common].copy()
            moved = np.sort(rng.permutation(len(common))[:int(round(corrupt * len(common)))])
            extent = float(np.max(np.abs(side_a - np.median(side_a, axis=0))))
            side_a[moved] += rng.uniform(-1.0, 1.0, size=(len(moved), 3)) * extent
            clouds.append(side_a), ids.append(common), displaced.append(common[moved])
            pairs.append((i, j))
    if not pairs:
        raise ValueError(f"no two parts share {MIN_COMMON_TRACKS} standing tracks")
    call_pairs = np.array([[parts + q, j] for q, (_, j) in enumerate(pairs)])
    found = align_models(clouds, ids, call_pairs, align_threshold ** 2, iterations=align_iterations, min_num_extra_inliers=3,
                         min_extra_fraction=0.25, seed=seed)
    pair_arr = np.array(pairs)
    frames = merge_frames(parts, pair_arr, found, root=0, min_inliers=MIN_COMMON_TRACKS // 2)
    per_pair = []
    for q, (i, j) in enumerate(pairs):
        ratio = units[i] / units[j]   # part i's unit in part j's
        per_pair.append({
            "parts": [i, j], "status": found.status[q], "common_tracks": int(found.common_count[q]),
            "inliers": int(found.inlier_count[q]), "corrupted": int(len(displaced[q])),
            "corrupted_among_inliers": int(np.count_nonzero(np.isin(found.inliers[q], displaced[q]))),
            "scale": float(found.scale[q]), "true_baseline_ratio": ratio, "scale_error": abs(float(found.scale[q]) / ratio - 1.0),
            "in_tree": bool(q in frames.tree_pairs.tolist()),
            "disagreement": {"rotation_deg": float(frames.rotation_deg[q]), "log_scale": float(frames.log_scale[q]),
                             "distance": float(frames.distance[q])}})

    # the union in the frame of part 0: a view or a track that stands in several parts keeps the earliest part's
    poses, X = np.full((views, 12), np.nan), np.full((total, 3), np.nan)
    for k in reversed(range(parts)):
        if not frames.reached[k]:
            continue
        G = frames.frame(k)
        moved = transform_poses(G, recs[k].poses)
        poses[ranges[k][0] + np.array(recs[k].registered)] = moved[recs[k].registered]
        X[standing[k]] = apply_similarity(G, recs[k].X[standing[k]])
    registered = np.nonzero(~np.isnan(poses).any(axis=1))[0]
    truth_0 = true_poses_in_gauge(truth, 0, units[0])
    before = pose_errors(poses, truth_0, registered)
    cam, pt, uv = scene["camera_indices"], scene["point_indices"], scene["pixels"]
    kept = np.nonzero(~np.isnan(X).any(axis=1))[0]
    cam_slot, pt_slot = np.full(views, -1), np.full(total, -1)
    cam_slot[registered] = np.arange(len(registered))
    pt_slot[kept] = np.arange(len(kept))
    use = np.nonzero((cam_slot[cam] >= 0) & (pt_slot[pt] >= 0))[0]
    use = use[_errors(scene["K"], poses, X, cam[use], pt[use], uv[use]) <= options[1]]
    solver = "iterative" if len(registered) > DENSE_MAX_VIEWS else "dense"
    adjusted, _, info = bundle_adjust(scene["K"], poses[registered], X[kept], cam_slot[cam[use]], pt_slot[pt[use]], uv[use],
                                      fixed_cameras=(0,), max_steps=options[5], linear_solver=solver)
    after_poses = poses.copy()
    after_poses[registered] = adjusted
    after = pose_errors(after_poses, truth_0, registered)
    own = [summary(pose_errors(rec.poses, true_poses_in_gauge(truth, first, unit)[first:], rec.registered))
           for rec, (first, _), unit in zip(recs, ranges, units)]
    return {
        "views": views, "parts": parts, "ranges": [list(r) for r in ranges],
        "views_registered": {"parts": [len(rec.registered) for rec in recs], "merged": int(len(registered))},
        "parts_merged": int(np.count_nonzero(frames.reached)), "pairs": per_pair,
        "tree_pairs": [int(q) for q in frames.tree_pairs], "corrupt": corrupt,
        "inconsistent_pairs": [int(q) for q in inconsistent_alignments(frames, 1.0, 0.02)],
        "parts_own": own,
        "merged_before_adjustment": {"worst": summary(before)},
        "merged_after_adjustment": {"worst": summary(after), "ba_status": info.status, "ba_solver": solver,
                                    "ba_observations": int(len(use)),
                                    "rms_px": float(np.sqrt(info.final_cost / len(use))) if len(use) else float("nan")},
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=12, help="views of the scene (4 to 64)")
    ap.add_argument("--overlap", type=int, default=4, help="views that both halves reconstruct")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--noise", type=float, default=0.5, help="pixel noise (standard deviation)")
    ap.add_argument("--outliers", type=float, default=0.2, help="fraction of observations replaced by random pixels")
    ap.add_argument("--corrupt", type=float, default=0.0, metavar="FRACTION",
                    help="displace this share of B's common points before the alignment")
    ap.add_argument("--align-threshold", type=float, default=0.05,
                    help="inlier distance of the alignment, in units of A's seed baseline")
    ap.add_argument("--align-iterations", type=int, default=1000, help="RANSAC hypotheses of the alignment")
    ap.add_argument("--parts", type=int, default=2, metavar="K",
                    help="reconstruct K overlapping view ranges and align every pair of them in one call (default 2: two halves)")
    args = ap.parse_args()
    try:
        out = run(args.views, args.overlap, args.points, args.seed, args.noise, args.outliers, corrupt=args.corrupt,
                  align_threshold=args.align_threshold, align_iterations=args.align_iterations, parts=args.parts)
    except ValueError as e:
        ap.error(str(e))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
