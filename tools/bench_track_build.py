"""Timing of tracks from pairwise matches (``sfm_build_tracks``): milliseconds per call at 100 x 8 000 and 1 000 x 8 000
features (images x features per image), each image matched to its 10 next neighbours with 2 000 matches per pair, one
JSON line per size.

Per size: the median of ``--steps`` calls after ``--warmup`` calls, by HIP events around the whole call (the workspace
allocation included).  The graph is ``synthetic.match_graph`` with 1 % wrong matches.  A size is written
``IxFxNxM`` (images x features per image x neighbours x matches per pair); ``--sizes 100x8000x10x2000,1000x8000x10x2000``.
``--oracle`` also times the plain-Python oracle of tests/track_build_oracle.py on the host (slow: use it at the small size).

``--profile DIR`` instead re-runs this script (one size per run, under ``timeout``) below ``rocprofv3 --kernel-trace --stats``
and prints the per-kernel split of its stats file."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = "100x8000x10x2000,1000x8000x10x2000"
WRONG = 0.01


def parse(size: str):
    return tuple(int(v) for v in size.split("x"))


def time_size(size: str, steps: int, warmup: int, oracle: bool) -> dict:
    import torch

    from structure_from_motion_amd import device, synthetic

    dev = device.require_gpu()
    images, features, neighbours, per_pair = parse(size)
    g = synthetic.match_graph(images, features, neighbours, per_pair, wrong_fraction=WRONG, seed=0)
    args = [torch.as_tensor(g[k], device=dev) for k in ("image_offset", "pairs", "match_offset", "match_index")]
    F = images * features
    for _ in range(warmup):
        device.build_tracks(*args, F)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        start.record()
        out = device.build_tracks(*args, F)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    info = device.read_track_build_info(out[6])
    rec = {"size": size, "images": images, "features": F, "pairs": int(len(g["pairs"])), "matches": int(len(g["match_index"])),
           "wrong_fraction": WRONG, "calls": steps, "call_ms": sorted(times)[len(times) // 2], "min_ms": min(times),
           "status": info.status, "components": info.components, "tracks": info.tracks, "observations": info.observations,
           "conflicts": info.conflicts, "unmatched": info.unmatched}
    if oracle:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import track_build_oracle as tbo

        t0 = time.perf_counter()
        ref = tbo.build_tracks(g["image_offset"], g["pairs"], g["match_offset"], g["match_index"])
        rec["oracle_s"] = time.perf_counter() - t0
        got = [t.cpu().numpy().astype(np.int64) for t in out[:6]]
        rec["oracle_equal"] = all(np.array_equal(a, ref[k].astype(np.int64)) for a, k in
                                  zip(got, ("component", "track", "status", "camera_index", "point_index", "feature_index")))
    return rec


def profile(out_dir: str, size: str, steps: int, warmup: int, limit: int) -> dict:
    run_dir = os.path.join(out_dir, size)
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir,
           "-o", "track_build", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--steps", str(steps),
           "--warmup", str(warmup)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "build_" in row["Name"] or "order_" in row["Name"]:
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"size": size, "kernels": split, "timing": proc.stdout.strip().splitlines()[-1:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="IxFxNxM, comma-separated")
    ap.add_argument("--steps", type=int, default=10, help="timed calls per size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle", action="store_true", help="also time the plain-Python oracle (host)")
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        if args.profile:
            print(json.dumps(profile(args.profile, size, args.steps, args.warmup, args.limit)), flush=True)
        else:
            print(json.dumps(time_size(size, args.steps, args.warmup, args.oracle)), flush=True)


if __name__ == "__main__":
    main()
