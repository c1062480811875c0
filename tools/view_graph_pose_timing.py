"""Timing of the pose call behind ``sfm_verify_pairs`` (profiles/view_graph/README.md): device events around one
``ViewGraphWorkspace.run`` (seven launches), one ``poses`` (three launches) and both in a row, at the graph shapes of
tools/view_graph_timing.py, the median of ROUNDS rounds after WARMUP warm-ups; then the statuses and median angles of the
pairs, and the app by either seed route.

    python tools/view_graph_pose_timing.py [--iterations 2000] [--app]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from structure_from_motion_amd import device  # noqa: E402
from tools.view_graph_timing import RMS, ROUNDS, SEED, THR, WARMUP, graph_arrays, timed  # noqa: E402


def measure(views, step_deg, iterations):
    _, corr, offset, counts = graph_arrays(views, step_deg)
    Q = len(counts)
    ws = device.ViewGraphWorkspace(Q, int(offset[-1]), iterations)
    offset_t, gate_t = device.to_device(offset, torch.int64), device.to_device(np.floor(0.4 * counts))

    def verify():
        ws.run(corr, offset_t, gate_t, THR, RMS, 0.8, SEED)

    def poses():
        ws.poses(50.0)

    def both():
        verify()
        poses()

    for _ in range(WARMUP):
        both()
    torch.cuda.synchronize()
    tv, tp, tb = [], [], []
    for _ in range(ROUNDS):
        tv.append(timed(verify))
        tp.append(timed(poses))
        tb.append(timed(both))
    out = ws.outcome()
    ok = out.pose_status == device.POSE_OK
    return dict(views=views, pairs=Q, items=int(offset[-1]), iterations=iterations, verify_us=float(np.median(tv)),
                poses_us=float(np.median(tp)), both_us=float(np.median(tb)), verify_min_us=float(min(tv)),
                poses_min_us=float(min(tp)), both_min_us=float(min(tb)), poses_ok=int(ok.sum()),
                median_angle_deg_range=[float(np.degrees(out.pose_median_angle[ok]).min()),
                                        float(np.degrees(out.pose_median_angle[ok]).max())] if ok.any() else None)


def app_routes():
    from apps import sfm_multi_view as app

    keep = ("seed_pair", "median_angle_deg", "views_registered", "registration_order", "rotation_error_rad", "translation_error",
            "rms_px", "points_ok")
    out = {}
    for route in ("first", "auto"):
        r = app.run(views=8, tracks="matches", verify="batched", seed_pair=route)
        out[route] = {k: r[k] for k in keep if k in r}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--app", action="store_true", help="also run apps/sfm_multi_view.py by either seed route")
    args = ap.parse_args()
    device.require_gpu()
    for views, step in ((8, 5.0), (96, 3.75)):
        print(json.dumps(measure(views, step, args.iterations)), flush=True)
    if args.app:
        print(json.dumps(app_routes()), flush=True)


if __name__ == "__main__":
    main()
