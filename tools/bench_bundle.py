"""Bundle adjustment timing (``sfm_bundle_adjust``): milliseconds per call and per LM trial step at 3 x 5 000, 16 x 100 000
and 64 x 500 000 (cameras x points, 5 observations per point), one JSON line per size.

Per size: the median of ``--steps`` calls after ``--warmup`` calls, by HIP events around the whole call (``max_steps``
LM steps, set-up included), and the same for ``max_steps = 0`` (set-up, first linearisation and the starting cost only).
Per step = (call - set-up) / trial steps.  Sizes: ``--sizes 3x5000,16x100000,64x500000``.

``--corrupt FRACTION`` shifts that fraction of the pixels by up to +-``--corrupt-spread`` (200) px
(``synthetic.corrupt_observations``, seed = cameras + 100).  ``--loss huber|cauchy`` with ``--loss-scale`` pixels times the
robust call and, in the same process on the same data, the squared one beside it (``squared_call_ms``,
``squared_ms_per_step``).  Without these options the run and its JSON are what they were.

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


def time_size(cameras: int, points: int, per_point: int, max_steps: int, steps: int, warmup: int, loss: str = "squared",
              loss_scale: float = 2.0, corrupt: float = 0.0, spread: float = 200.0) -> dict:
    import torch

    from structure_from_motion_amd import device, synthetic

    device.require_gpu()
    pr = synthetic.bundle_problem(cameras, points, per_point=per_point, seed=cameras)
    if corrupt > 0.0:
        pr, _ = synthetic.corrupt_observations(pr, corrupt, spread, seed=cameras + 100)
    args = (device.to_device(pr["poses"]), device.to_device(pr["points"]),
            device.to_device(pr["camera_indices"], dtype=torch.int32), device.to_device(pr["point_indices"], dtype=torch.int32),
            device.to_device(pr["pixels"]), pr["K"], (0,))

    def median(limit, **kw):
        for _ in range(warmup):
            device.bundle_adjust(*args, max_steps=limit, **kw)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(steps):
            start.record()
            out = device.bundle_adjust(*args, max_steps=limit, **kw)
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return sorted(times)[len(times) // 2], min(times), device.read_bundle_info(out[2])

    robust = {} if loss == "squared" else dict(loss=loss, loss_scale=loss_scale)
    setup_ms, _, _ = median(0, **robust)
    call_ms, min_ms, info = median(max_steps, **robust)
    trial_steps = max(info.steps, 1)
    out = {"cameras": cameras, "points": points, "observations": int(len(pr["pixels"])), "max_steps": max_steps,
           "calls": steps, "call_ms": call_ms, "min_ms": min_ms, "setup_ms": setup_ms,
           "ms_per_step": (call_ms - setup_ms) / trial_steps, "steps": info.steps, "accepted": info.accepted,
           "initial_cost": info.initial_cost, "final_cost": info.final_cost, "status": info.status}
    if corrupt > 0.0:
        out.update(corrupt=corrupt, corrupt_spread=spread)
    if robust:   # the squared call beside it, same process, same data
        sq_setup, _, _ = median(0)
        sq_call, _, sq = median(max_steps)
        out.update(loss=loss, loss_scale=loss_scale, squared_call_ms=sq_call, squared_setup_ms=sq_setup,
                   squared_ms_per_step=(sq_call - sq_setup) / max(sq.steps, 1), squared_steps=sq.steps,
                   squared_accepted=sq.accepted)
    return out


def profile(out_dir: str, size: str, per_point: int, max_steps: int, steps: int, warmup: int, limit: int, passed=()) -> dict:
    run_dir = os.path.join(out_dir, size)
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir,
           "-o", "bundle", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--per-point", str(per_point),
           "--max-steps", str(max_steps), "--steps", str(steps), "--warmup", str(warmup), *passed]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "bundle" in row["Name"] or "sfmlm::" in row["Name"]:
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
    ap.add_argument("--loss", choices=("squared", "huber", "cauchy"), default="squared")
    ap.add_argument("--loss-scale", type=float, default=2.0, help="scale of a huber or cauchy loss in pixels")
    ap.add_argument("--corrupt", type=float, default=0.0, metavar="FRACTION", help="fraction of the pixels shifted")
    ap.add_argument("--corrupt-spread", type=float, default=200.0, help="the largest shift in pixels")
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    passed = ["--loss", args.loss, "--loss-scale", str(args.loss_scale), "--corrupt", str(args.corrupt), "--corrupt-spread",
              str(args.corrupt_spread)]
    for size in args.sizes.split(","):
        if args.profile:
            print(json.dumps(profile(args.profile, size, args.per_point, args.max_steps, args.steps, args.warmup, args.limit,
                                     passed)),
                  flush=True)
        else:
            cameras, points = (int(v) for v in size.split("x"))
            print(json.dumps(time_size(cameras, points, args.per_point, args.max_steps, args.steps, args.warmup, args.loss,
                                       args.loss_scale, args.corrupt, args.corrupt_spread)), flush=True)


if __name__ == "__main__":
    main()
