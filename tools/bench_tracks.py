"""Timing of the triangulation of multi-view tracks (``sfm_triangulate_tracks``): milliseconds per call at 16 x 100 000 x 4
and 64 x 1 000 000 x 5 (cameras x points x observations per point), with ``refine_steps`` 0 and 10, one JSON line per size
and setting.

Per size: the median of ``--steps`` calls after ``--warmup`` calls, by HIP events around the whole call (set-up included).
The cameras are those of ``synthetic.bundle_problem``; point p is seen by ``per_point`` consecutive cameras from a random
first one, with 0.5 px noise, and the observations come in random order.  A size written ``CxPxL-H`` gives each point a
track length drawn uniformly from L to H instead (the cost of unequal track lengths inside a wave).  Sizes:
``--sizes 16x100000x4,64x1000000x5``.

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

SIZES = "16x100000x4,64x1000000x5"


def problem(cameras: int, points: int, lo: int, hi: int, seed: int = 0) -> dict:
    from structure_from_motion_amd import synthetic

    rng = np.random.default_rng(seed)
    poses = synthetic.bundle_problem(cameras, 1, per_point=1, seed=cameras)["poses_true"]
    X = np.column_stack([rng.uniform(-1.0, 1.0, points), rng.uniform(-1.0, 1.0, points), rng.uniform(4.0, 6.0, points)])
    length = rng.integers(lo, hi + 1, points) if hi > lo else np.full(points, lo)
    pt = np.repeat(np.arange(points), length)
    first = np.repeat(rng.integers(0, cameras, points), length)
    offset = np.arange(len(pt)) - np.repeat(np.cumsum(length) - length, length)
    cam = (first + offset) % cameras
    order = rng.permutation(len(pt))
    cam, pt = cam[order], pt[order]
    R = poses[cam, :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, X[pt]) + poses[cam, 9:]
    uvw = xc @ synthetic.BENCH_K.T
    pixels = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, 0.5, (len(pt), 2))
    return dict(poses=poses, cam=cam.astype(np.int32), pt=pt.astype(np.int32), pixels=pixels, K=synthetic.BENCH_K)


def parse(size: str):
    c, p, lengths = size.split("x")
    lo, _, hi = lengths.partition("-")
    return int(c), int(p), int(lo), int(hi or lo)


def time_size(size: str, refine_steps: int, steps: int, warmup: int) -> dict:
    import torch

    from structure_from_motion_amd import device

    device.require_gpu()
    cameras, points, lo, hi = parse(size)
    pr = problem(cameras, points, lo, hi)
    args = (device.to_device(pr["poses"]), device.to_device(pr["cam"], dtype=torch.int32),
            device.to_device(pr["pt"], dtype=torch.int32), device.to_device(pr["pixels"]), points, pr["K"], 2,
            float(np.radians(1.0)), 16.0, refine_steps)
    for _ in range(warmup):
        device.triangulate_tracks(*args)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        start.record()
        out = device.triangulate_tracks(*args)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    info = device.read_tracks_info(out[4])
    return {"size": size, "cameras": cameras, "points": points, "observations": int(len(pr["cam"])),
            "refine_steps": refine_steps, "calls": steps, "call_ms": sorted(times)[len(times) // 2], "min_ms": min(times),
            "points_ok": info.points_ok, "max_refine_steps_taken": info.max_refine_steps_taken, "status": info.status}


def profile(out_dir: str, size: str, refine_steps: int, steps: int, warmup: int, limit: int) -> dict:
    run_dir = os.path.join(out_dir, f"{size}_r{refine_steps}")
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir,
           "-o", "tracks", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--refine-steps", str(refine_steps),
           "--steps", str(steps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "tracks" in row["Name"] or "order_" in row["Name"]:
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"size": size, "refine_steps": refine_steps, "kernels": split, "timing": proc.stdout.strip().splitlines()[-1:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="CxPxL or CxPxL-H, comma-separated")
    ap.add_argument("--refine-steps", default="0,10", help="comma-separated refine_steps settings")
    ap.add_argument("--steps", type=int, default=10, help="timed calls per size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        for refine in (int(v) for v in args.refine_steps.split(",")):
            if args.profile:
                print(json.dumps(profile(args.profile, size, refine, args.steps, args.warmup, args.limit)), flush=True)
            else:
                print(json.dumps(time_size(size, refine, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
