"""PnP pass throughput: milliseconds per whole pass (fit, score, select, mask: ``sfm_pnp_ransac_pass``) and evaluations per
second (points x hypotheses / time) at 50 000 x 100 000 and 5 000 x 10 000, one JSON line per size.

``--profile DIR`` instead re-runs this script (one size per run, under ``timeout``) below ``rocprofv3 --kernel-trace --stats``
and prints the per-kernel split of its stats file.  Sizes: ``--sizes 50000x100000,5000x10000``.

``--refine`` instead times the refinement of the winner (``sfm_pnp_refine``, one round, at most 20 LM steps) at 5 000 and
50 000 points for one view and a batch of 64 views: HIP events around the call, median of ``--steps`` calls, one JSON line
per size (``--refine-sizes 5000x1,5000x64,50000x1,50000x64``, points x views).

``--solver p3p`` times the P3P pass (four-item samples) instead of the DLT's, in every mode but ``--refine``.  ``--fit``
times the fit kernel alone (``sfm_pnp_fit`` / ``sfm_p3p_fit`` on a Philox table) at each size.  ``--confidence`` prints,
for both solvers and 30 / 50 / 70 % outliers, the hypotheses H that give a clean sample with 99 % probability
(H = ceil(log(0.01) / log(1 - w^s)), w the inlier ratio, s = 6 for the DLT, 4 for P3P: three solve points and the one that
picks the solution) and the measured pass time at that H for the first of ``--sizes``."""
import math
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SIZES = "50000x100000,5000x10000"
REFINE_SIZES = "5000x1,5000x64,50000x1,50000x64"


def time_pass(n: int, h: int, steps: int, warmup: int, solver: str = "dlt") -> dict:
    import torch

    import pnp_oracle as orc
    from structure_from_motion_amd import device, synthetic
    from structure_from_motion_amd._native import AGG_RMS

    dev = device.require_gpu()
    K = synthetic.BENCH_K
    pts = device.to_device(orc.scene(n, seed=6, K=K, noise_px=0.02)[0]).reshape(1, n, 5)
    ws = device.PnPWorkspace(1, n, h, dev)
    for s in range(warmup):
        ws.run(pts, K, 4.0, 10, AGG_RMS, philox=(100 + s, 0, 1), solver=solver)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for s in range(steps):
        start.record()
        ws.run(pts, K, 4.0, 10, AGG_RMS, philox=(1000 + s, 0, 1), solver=solver)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    best = ws.outcome(0)
    ms = sorted(times)[len(times) // 2]
    return {"solver": solver, "n": n, "h": h, "steps": steps, "median_ms": ms, "min_ms": min(times), "evals_per_s": n * h / (ms * 1e-3),
            "best_h": best.best_h, "extra_inliers": best.extra_inliers}


def time_fit(n: int, h: int, steps: int, warmup: int, solver: str = "dlt") -> dict:
    import torch

    import pnp_oracle as orc
    from structure_from_motion_amd import device, synthetic

    K = synthetic.BENCH_K
    pts = device.to_device(orc.scene(n, seed=6, K=K, noise_px=0.02)[0]).reshape(1, n, 5)
    S = device.sample_philox(3, 0, h, n)
    fit = device.p3p_fit if solver == "p3p" else device.pnp_fit
    model, flags = fit(pts, S, K)
    for _ in range(warmup):
        fit(pts, S, K, model, flags)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        start.record()
        fit(pts, S, K, model, flags)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    ms = sorted(times)[len(times) // 2]
    nan = int(torch.isnan(model[0, :, 0]).sum())
    return {"solver": solver, "fit_only": True, "n": n, "h": h, "steps": steps, "median_ms": ms, "min_ms": min(times),
            "no_solution": nan, "flagged": int(flags.ne(0).sum())}


def hypotheses_for(confidence: float, inlier_ratio: float, sample: int) -> int:
    """Hypotheses for a clean sample with the given probability: ceil(log(1 - p) / log(1 - w^s))."""
    return int(math.ceil(math.log(1.0 - confidence) / math.log(1.0 - inlier_ratio**sample)))


def time_refine(n: int, batch: int, steps: int, warmup: int, rounds: int = 1, max_steps: int = 20) -> dict:
    import numpy as np
    import torch

    import pnp_oracle as orc
    from structure_from_motion_amd import device, synthetic
    from structure_from_motion_amd._native import AGG_RMS

    dev = device.require_gpu()
    K = synthetic.BENCH_K
    views = np.stack([orc.scene(n, seed=40 + b, K=K, outlier_fraction=0.3, noise_px=0.5)[0] for b in range(batch)])
    pts = device.to_device(views).reshape(batch, n, 5)
    ws = device.PnPWorkspace(batch, n, 256, dev)
    ws.run(pts, K, 4.0, 10, AGG_RMS, philox=(7, 0, 1000))
    best_h = ws.result[:, 1].clamp(min=0)
    model = ws.model[torch.arange(batch, device=dev), best_h].contiguous()
    err = ws.result[:, 2].contiguous().view(torch.float64)
    call = lambda: device.pnp_refine(pts, model, ws.mask, err, K, 4.0, AGG_RMS, rounds, max_steps)  # noqa: E731
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(steps):
        start.record()
        out = call()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    info = device.read_pnp_refine_info(out[2])
    ms = sorted(times)[len(times) // 2]
    return {"n": n, "views": batch, "rounds": rounds, "max_steps": max_steps, "steps": steps, "median_ms": ms,
            "min_ms": min(times), "us_per_view": ms * 1e3 / batch,
            "lm_steps_mean": float(np.mean([r.lm_steps for r in info])),
            "accepted": sum(r.accepted > 0 for r in info), "inliers_mean": float(np.mean([r.count for r in info]))}


def profile(out_dir: str, n: int, h: int, steps: int, warmup: int, limit: int, solver: str = "dlt") -> dict:
    run_dir = os.path.join(out_dir, f"{solver}_{n}x{h}")
    os.makedirs(run_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", run_dir, "-o", "pnp", "--",
           sys.executable, os.path.abspath(__file__), "--sizes", f"{n}x{h}", "--steps", str(steps), "--warmup", str(warmup), "--solver", solver]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                if any(key in row["Name"] for key in ("pnp", "p3p", "select_")):   # the pass's kernels, selection included
                    name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                    split[name] = {
                        "calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "percent": float(row["Percentage"])}
    return {"solver": solver, "n": n, "h": h, "kernels": split}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=300, help="seconds per profiled run")
    ap.add_argument("--refine", action="store_true", help="time the refinement of the winner instead of the pass")
    ap.add_argument("--refine-sizes", default=REFINE_SIZES)
    ap.add_argument("--solver", choices=("dlt", "p3p"), default="dlt", help="minimal solver of the timed pass")
    ap.add_argument("--fit", action="store_true", help="time the fit kernel alone")
    ap.add_argument("--confidence", action="store_true",
                    help="hypotheses and pass time to a clean sample with 99 %% probability, both solvers")
    args = ap.parse_args()
    if args.confidence:
        n = int(args.sizes.split(",")[0].split("x")[0])
        for outliers in (0.3, 0.5, 0.7):
            for solver, sample in (("dlt", 6), ("p3p", 4)):
                h = hypotheses_for(0.99, 1.0 - outliers, sample)
                rec = time_pass(n, h, args.steps, args.warmup, solver)
                print(json.dumps(dict(rec, outliers=outliers, confidence=0.99)), flush=True)
        return
    if args.refine:
        for size in args.refine_sizes.split(","):
            n, batch = (int(v) for v in size.split("x"))
            print(json.dumps(time_refine(n, batch, args.steps, args.warmup)), flush=True)
        return
    for size in args.sizes.split(","):
        n, h = (int(v) for v in size.split("x"))
        if args.profile:
            print(json.dumps(profile(args.profile, n, h, args.steps, args.warmup, args.limit, args.solver)), flush=True)
        elif args.fit:
            print(json.dumps(time_fit(n, h, args.steps, args.warmup, args.solver)), flush=True)
        else:
            print(json.dumps(time_pass(n, h, args.steps, args.warmup, args.solver)), flush=True)


if __name__ == "__main__":
    main()
