"""Timing of the outlier-robust triangulation of tracks (``sfm_triangulate_tracks_robust``) next to the plain call
(``sfm_triangulate_tracks``) on the same inputs: milliseconds per call at the sizes of tools/bench_tracks.py (16 x 100 000 x 4
and 64 x 1 000 000 x 5, cameras x points x observations per point), the mixed lengths 2 .. 8 and one size with 64-long tracks,
with ``refine_steps`` 0 and 10, one JSON line per size and setting.

The scenes are those of tools/bench_tracks.py with ``--shifted`` (0.15) of the pixels moved by up to +-100 px.  Per size: the
two calls alternate, ``--steps`` times each after ``--warmup`` each, timed by HIP events around the whole call (set-up
included); the medians and the minima are reported.  The robust call takes the caller's workspace and outputs, so nothing is
allocated inside the timed window.

``--profile DIR`` instead re-runs this script (one size per run, under ``timeout``) below ``rocprofv3 --kernel-trace --stats``
and prints the per-kernel split of its stats file."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_tracks  # noqa: E402

SIZES = "16x100000x4,64x1000000x5,16x100000x2-8,64x20000x64"
MAX_ERROR = 9.0


def time_size(size: str, refine_steps: int, steps: int, warmup: int, shifted: float, max_hypotheses: int) -> dict:
    import torch

    from structure_from_motion_amd import device

    device.require_gpu()
    cameras, points, lo, hi = bench_tracks.parse(size)
    pr = bench_tracks.problem(cameras, points, lo, hi)
    rng = np.random.default_rng(1)
    bad = rng.random(len(pr["pixels"])) < shifted
    pr["pixels"][bad] += rng.uniform(-100.0, 100.0, (int(bad.sum()), 2))
    inputs = (device.to_device(pr["poses"]), device.to_device(pr["cam"], dtype=torch.int32),
              device.to_device(pr["pt"], dtype=torch.int32), device.to_device(pr["pixels"]), points, pr["K"])
    min_angle = float(np.radians(1.0))
    out, ws = device.triangulate_tracks_robust(*inputs, MAX_ERROR, 2, min_angle, refine_steps, max_hypotheses)

    def robust():
        return device.triangulate_tracks_robust(*inputs, MAX_ERROR, 2, min_angle, refine_steps, max_hypotheses, out=out,
                                                workspace=ws)[0]

    def plain():
        return device.triangulate_tracks(*inputs, 2, min_angle, MAX_ERROR, refine_steps)

    for _ in range(warmup):
        plain(), robust()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"plain": [], "robust": []}
    for _ in range(steps):
        for name, call in (("plain", plain), ("robust", robust)):
            start.record()
            result = call()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end))
            if name == "plain":
                plain_info = device.read_tracks_info(result[4])
    info = device.read_robust_tracks_info(out[5])
    median = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    return {"size": size, "cameras": cameras, "points": points, "observations": int(len(pr["cam"])), "shifted": shifted,
            "refine_steps": refine_steps, "max_hypotheses": max_hypotheses, "calls": steps,
            "plain_ms": median(times["plain"]), "plain_min_ms": min(times["plain"]),
            "robust_ms": median(times["robust"]), "robust_min_ms": min(times["robust"]),
            "plain_points_ok": plain_info.points_ok, "robust_points_ok": info.points_ok,
            "inlier_observations": info.inlier_observations, "hypotheses": info.hypotheses,
            "max_refine_steps_taken": info.max_refine_steps_taken, "status": info.status}


def profile(out_dir: str, size: str, refine_steps: int, steps: int, warmup: int, limit: int, shifted: float,
            max_hypotheses: int) -> dict:
    run_dir = os.path.join(out_dir, f"{size}_r{refine_steps}")
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir,
           "-o", "robust_tracks", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--refine-steps",
           str(refine_steps), "--steps", str(steps), "--warmup", str(warmup), "--shifted", str(shifted), "--max-hypotheses",
           str(max_hypotheses)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "tracks" in row["Name"] or "robust" in row["Name"] or "order_" in row["Name"]:
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"size": size, "refine_steps": refine_steps, "kernels": split, "timing": proc.stdout.strip().splitlines()[-1:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="CxPxL or CxPxL-H, comma-separated")
    ap.add_argument("--refine-steps", default="0,10", help="comma-separated refine_steps settings")
    ap.add_argument("--steps", type=int, default=10, help="timed calls of each entry point per size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shifted", type=float, default=0.15, help="share of the pixels moved by up to +-100 px")
    ap.add_argument("--max-hypotheses", type=int, default=64)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        for refine in (int(v) for v in args.refine_steps.split(",")):
            if args.profile:
                print(json.dumps(profile(args.profile, size, refine, args.steps, args.warmup, args.limit, args.shifted,
                                         args.max_hypotheses)), flush=True)
            else:
                print(json.dumps(time_size(size, refine, args.steps, args.warmup, args.shifted, args.max_hypotheses)), flush=True)


if __name__ == "__main__":
    main()
