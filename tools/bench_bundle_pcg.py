"""Timing of bundle adjustment with the iterative Schur solver (``sfm_bundle_adjust_pcg``): milliseconds per call, per LM
trial step and per CG iteration, CG iterations per step, and the final cost relative to the dense solver where that one
runs (at most 64 cameras).  One JSON line per size.

Sizes ``CxP`` (cameras x points): 64 x 500 000 is ``bench_bundle.py``'s random problem (5 observations per point, the
same seed), for an A/B on one box; the others are ``synthetic.sequence_bundle_problem`` (banded visibility, 4
observations per point).  Per size: the median of ``--steps`` calls after ``--warmup`` calls, by HIP events around the
whole call, and the same for ``max_steps = 0`` (set-up, first linearisation and starting cost).  Per step = (call -
set-up) / trial steps; per CG iteration = (call - set-up) / CG iterations, an upper bound (it includes the steps'
linearisation, preconditioner and trial).

``--corrupt FRACTION`` shifts that fraction of the pixels by up to +-``--corrupt-spread`` (200) px
(``synthetic.corrupt_observations``, seed = cameras + 100).  ``--loss huber|cauchy`` with ``--loss-scale`` pixels times the
robust call and, in the same process on the same data, the squared one beside it (``squared_*``); the dense comparison
is then left out.  Without these options the run and its JSON are what they were.

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

SIZES = "64x500000,256x500000,1024x1000000,4096x2000000"


def problem(cameras: int, points: int):
    from structure_from_motion_amd import synthetic

    if cameras == 64 and points == 500000:   # bench_bundle.py's problem
        return synthetic.bundle_problem(cameras, points, per_point=5, seed=cameras)
    return synthetic.sequence_bundle_problem(cameras, points, track_length=4, seed=cameras)


def time_size(cameras: int, points: int, max_steps: int, max_cg: int, tol: float, steps: int, warmup: int,
              loss: str = "squared", loss_scale: float = 2.0, corrupt: float = 0.0, spread: float = 200.0) -> dict:
    import torch

    from structure_from_motion_amd import device

    device.require_gpu()
    pr = problem(cameras, points)
    if corrupt > 0.0:
        from structure_from_motion_amd import synthetic

        pr, _ = synthetic.corrupt_observations(pr, corrupt, spread, seed=cameras + 100)
    args = (device.to_device(pr["poses"]), device.to_device(pr["points"]),
            device.to_device(pr["camera_indices"], dtype=torch.int32), device.to_device(pr["point_indices"], dtype=torch.int32),
            device.to_device(pr["pixels"]), pr["K"], (0,))

    def median(fn, read, limit):
        for _ in range(warmup):
            fn(*args, max_steps=limit)
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(steps):
            start.record()
            out = fn(*args, max_steps=limit)
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return sorted(times)[len(times) // 2], read(out[2])

    robust = {} if loss == "squared" else dict(loss=loss, loss_scale=loss_scale)

    def squared(*a, max_steps):
        return device.bundle_adjust_pcg(*a, max_steps=max_steps, max_cg_iterations=max_cg, cg_tolerance=tol)

    def pcg(*a, max_steps):
        return device.bundle_adjust_pcg(*a, max_steps=max_steps, max_cg_iterations=max_cg, cg_tolerance=tol, **robust)

    setup_ms, _ = median(pcg, device.read_bundle_pcg_info, 0)
    call_ms, info = median(pcg, device.read_bundle_pcg_info, max_steps)
    out = {"cameras": cameras, "points": points, "observations": int(len(pr["pixels"])), "max_steps": max_steps,
           "max_cg_iterations": max_cg, "cg_tolerance": tol, "calls": steps, "call_ms": call_ms, "setup_ms": setup_ms,
           "ms_per_step": (call_ms - setup_ms) / max(info.steps, 1),
           "ms_per_cg_iteration": (call_ms - setup_ms) / max(info.cg_iterations, 1), "steps": info.steps,
           "accepted": info.accepted, "cg_iterations": info.cg_iterations, "cg_per_step": info.cg_iterations / max(info.steps, 1),
           "cg_max": info.cg_max, "initial_cost": info.initial_cost, "final_cost": info.final_cost, "status": info.status}
    if corrupt > 0.0:
        out.update(corrupt=corrupt, corrupt_spread=spread)
    if robust:   # the squared call beside it, same process, same data
        sq_setup, _ = median(squared, device.read_bundle_pcg_info, 0)
        sq_call, sq = median(squared, device.read_bundle_pcg_info, max_steps)
        out.update(loss=loss, loss_scale=loss_scale, squared_call_ms=sq_call, squared_setup_ms=sq_setup,
                   squared_ms_per_step=(sq_call - sq_setup) / max(sq.steps, 1),
                   squared_ms_per_cg_iteration=(sq_call - sq_setup) / max(sq.cg_iterations, 1), squared_steps=sq.steps,
                   squared_accepted=sq.accepted, squared_cg_iterations=sq.cg_iterations)
    elif cameras <= 64:
        dense_ms, dinfo = median(device.bundle_adjust, device.read_bundle_info, max_steps)
        out.update(dense_call_ms=dense_ms, dense_final_cost=dinfo.final_cost,
                   final_cost_over_dense=info.final_cost / dinfo.final_cost)
    return out


def profile(out_dir: str, size: str, args) -> dict:
    run_dir = os.path.join(out_dir, size)
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
           run_dir, "-o", "bundle_pcg", "--", sys.executable, os.path.abspath(__file__), "--sizes", size, "--max-steps",
           str(args.max_steps), "--max-cg", str(args.max_cg), "--tol", str(args.tol), "--steps", str(args.steps), "--warmup",
           str(args.warmup), "--loss", args.loss, "--loss-scale", str(args.loss_scale), "--corrupt", str(args.corrupt),
           "--corrupt-spread", str(args.corrupt_spread)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if "pcg_" in row["Name"] or "order_" in row["Name"] or "sfmlm::" in row["Name"]:
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"size": size, "kernels": split, "timing": proc.stdout.strip().splitlines()[-2:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--max-steps", type=int, default=10)
    ap.add_argument("--max-cg", type=int, default=100, help="max_cg_iterations")
    ap.add_argument("--tol", type=float, default=0.1, help="cg_tolerance")
    ap.add_argument("--steps", type=int, default=3, help="timed calls per size")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loss", choices=("squared", "huber", "cauchy"), default="squared")
    ap.add_argument("--loss-scale", type=float, default=2.0, help="scale of a huber or cauchy loss in pixels")
    ap.add_argument("--corrupt", type=float, default=0.0, metavar="FRACTION", help="fraction of the pixels shifted")
    ap.add_argument("--corrupt-spread", type=float, default=200.0, help="the largest shift in pixels")
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=600, help="seconds per profiled run")
    args = ap.parse_args()
    for size in args.sizes.split(","):
        if args.profile:
            print(json.dumps(profile(args.profile, size, args)), flush=True)
        else:
            cameras, points = (int(v) for v in size.split("x"))
            print(json.dumps(time_size(cameras, points, args.max_steps, args.max_cg, args.tol, args.steps, args.warmup, args.loss,
                                       args.loss_scale, args.corrupt, args.corrupt_spread)),
                  flush=True)


if __name__ == "__main__":
    main()
