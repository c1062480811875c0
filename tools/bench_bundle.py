"""Bundle adjustment timing (``sfm_bundle_adjust``): milliseconds per call and per LM trial step at 3 x 5 000, 16 x 100 000
and 64 x 500 000 (cameras x points, 5 observations per point), one JSON line per size.

Per size: the median of ``--steps`` calls after ``--warmup`` calls, by HIP events around the whole call (``max_steps``
LM steps, set-up included), and the same for ``max_steps = 0`` (set-up, first linearisation and the starting cost only).
Per step = (call - set-up) / trial steps.  Sizes: ``--sizes 3x5000,16x100000,64x500000``.

``--profile DIR`` instead re-runs this script (one size per run, under ``timeout``) below ``rocprofv3 --kernel-trace --stats``
and prints the per-kernel split of its stats file."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = "3x5000,16x100000,64x500000"


def time_size(cameras: int, points: int, per_point: int, max_steps: int, steps: int, warmup: int) -> dict:
    import torch

    from structure_from_motion_amd import device, synthetic

    device.require_gpu()
    pr = synthetic.bundle_problem(cameras, points, per_point=per_point, seed=cameras)
    args = (device.to_device(pr["poses"]), device.to_device(pr["points"]),
            device.to_device(pr["camera_indices"], dtype=torch.int32), device.to_device(pr["point_indices"], dtype=torch.int32),
            device.to_device(pr["pixels"]), pr["K"], (0,))

    def median(limit):
        for _ in range(warmup):
            device.bundle_adjust(*args, max_steps=limit)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(steps):
            start.record()
            out = device.bundle_adjust(*args, max_steps=limit)
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return sorted(times)[len(times) // 2], min(times), device.read_bundle_info(out[2])

    setup_ms, _, _ = median(0)
    call_ms, min_ms, info = median(max_steps)
    trial_steps = max(info.steps, 1)
    return {"cameras": cameras, "points": points, "observations": int(len(pr["pixels"])), "max_steps": max_steps,
            "calls": steps, "call_ms": call_ms, "min_ms": min_ms, "setup_ms": setup_ms,
            "ms_per_step": (call_ms - setup_ms) / trial_steps, "steps": info.steps, "accepted": info.accepted,
            "initial_cost": info.initial_cost, "final_cost": info.final_cost, "status": info.status}


def profile(out_dir: str, size: str, per_point: int, max_steps: int, steps: int, warmup: int, limit: int) -> dict:
    run_dir = os.path.join(out_dir, size)
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir,
           "-o", "bundle", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--per-point", str(per_point),
           "--max-steps", str(max_steps), "--steps", str(steps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "bundle" in row["Name"]:
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"size": size, "kernels": split, "timing": proc.stdout.strip().splitlines()[-2:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--per-point", type=int, default=5, help="observations per point")
    ap.add_argument("--max-steps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5, help="timed calls per size")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        if args.profile:
            print(json.dumps(profile(args.profile, size, args.per_point, args.max_steps, args.steps, args.warmup, args.limit)),
                  flush=True)
        else:
            cameras, points = (int(v) for v in size.split("x"))
            print(json.dumps(time_size(cameras, points, args.per_point, args.max_steps, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
