"""Timing of the pair-pose refinement behind ``sfm_verify_pairs`` and ``sfm_pair_poses`` (profiles/pair_refine/README.md):
device events around ``ViewGraphWorkspace.run`` + ``poses`` and around one ``refine_pair_poses`` call on the pose table they
left, at 1 and at 2 rounds, for PAIRS pairs of MATCHES matches each (two-view scenes of ``synthetic.two_view_scene``,
0.5 px noise, 30 % outliers, one seed per pair), the median of ROUNDS timed calls after WARMUP warm-ups; then the pairwise pose
errors against the truth before and after, and the app with and without ``--refine-pairs``.

    python tools/pair_refine_timing.py [--pairs 496] [--matches 2000] [--iterations 256] [--app]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from structure_from_motion_amd import device, synthetic  # noqa: E402
from tools.view_graph_timing import RMS, ROUNDS, SEED, WARMUP, timed  # noqa: E402

THR = 6e-6


def _angle(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def errors(table, R_true, t_true):
    ok = table["status"] == device.POSE_OK
    rot = [_angle((np.trace(R_true.T @ R) - 1.0) / 2.0) for R in table["R"][ok]]
    direction = [_angle(t @ t_true / np.linalg.norm(t_true)) for t in table["t"][ok]]
    return dict(pairs=int(ok.sum()), rotation_median_deg=float(np.median(rot)), rotation_max_deg=float(np.max(rot)),
                direction_median_deg=float(np.median(direction)), direction_max_deg=float(np.max(direction)))


def measure(pairs, matches, iterations):
    scenes = [synthetic.two_view_scene(matches, seed=1000 + q, outlier_fraction=0.3) for q in range(pairs)]
    K, R_true, t_true = scenes[0][2], scenes[0][3], scenes[0][4]
    pix = device.to_device(np.stack([np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])]))
    corr = device.normalize_correspondences(pix[0], pix[1], K)
    offset_t = device.to_device(np.arange(pairs + 1, dtype=np.int64) * matches, torch.int64)
    gate_t = device.to_device(np.full(pairs, float(matches // 15)))
    ws = device.ViewGraphWorkspace(pairs, pairs * matches, iterations)

    def verify_and_poses():
        ws.run(corr, offset_t, gate_t, THR, RMS, 0.8, SEED)
        ws.poses(50.0)

    verify_and_poses()
    start = ws.pose.clone()
    results = {}

    def refine(rounds):
        results[rounds] = device.refine_pair_poses(corr, offset_t, start, THR, RMS, rounds=rounds, max_steps=20)

    for _ in range(WARMUP):
        verify_and_poses()
        refine(1)
        refine(2)
    torch.cuda.synchronize()
    tv, t1, t2 = [], [], []
    for _ in range(ROUNDS):
        tv.append(timed(verify_and_poses))
        t1.append(timed(lambda: refine(1)))
        t2.append(timed(lambda: refine(2)))
    out = dict(pairs=pairs, matches=matches, iterations=iterations, verify_and_poses_us=float(np.median(tv)),
               refine_1_round_us=float(np.median(t1)), refine_2_rounds_us=float(np.median(t2)),
               verify_and_poses_min_us=float(min(tv)), refine_1_round_min_us=float(min(t1)), refine_2_rounds_min_us=float(min(t2)))
    out["before"] = errors(start.cpu().numpy().reshape(-1).view(device.POSE_DTYPE), R_true, t_true)
    for rounds in (1, 2):
        pose, _, info = results[rounds]
        info = device.read_pair_refine_info(info)
        out[f"after_{rounds}"] = dict(errors(pose.cpu().numpy().reshape(-1).view(device.POSE_DTYPE), R_true, t_true),
                                      rounds_kept=int(info["accepted"].sum()), lm_steps=int(info["lm_steps"].sum()),
                                      lm_steps_max=int(info["lm_steps"].max()))
    return out


def app_routes():
    from apps import sfm_multi_view as app

    keep = ("pair_refinement", "views_registered", "rms_px", "points_ok", "global_rotations", "global_positions")
    out = {}
    for rounds in (0, 2):
        r = app.run(views=8, tracks="matches", verify="batched", rotations="global", positions="global", refine_pairs=rounds)
        out[f"refine_pairs_{rounds}"] = {k: r[k] for k in keep if k in r}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=496)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=256)
    ap.add_argument("--app", action="store_true", help="also run apps/sfm_multi_view.py with --refine-pairs 0 and 2")
    args = ap.parse_args()
    device.require_gpu()
    print(json.dumps(measure(args.pairs, args.matches, args.iterations)), flush=True)
    if args.app:
        print(json.dumps(app_routes()), flush=True)


if __name__ == "__main__":
    main()
