"""Timing of the ragged absolute-pose call (``sfm_register_views``) next to the loop of per-view calls it
replaces: 64 views of 200 to 5 000 items each over one model, 2 000 P3P hypotheses per view, two refinement rounds.  One JSON
line with

* ``ragged_device_ms``: ``RegisterViewsWorkspace.run`` on device-resident inputs, HIP events around the call;
* ``single_device_ms``: the sum over the views of ``PnPWorkspace(1, n_v, h).run(solver="p3p")`` + ``.refine`` on the same
  items, HIP events around each view's two calls (the workspaces allocated before);
* ``ragged_host_ms``: ``register_views`` from host arrays (sort, upload, gather, the call, the read-back), wall clock;
* ``loop_host_ms``: the loop of ``estimate_pose_pnp_with_ransac(..., solver="p3p", refine_rounds=2)`` calls from the
  Python lists it takes (built before the clock starts), wall clock, with ``SFM_SAMPLER=philox`` so that both sample on the
  device;

and their ratios.  Every figure is the median of ``--steps`` timed repetitions after ``--warmup`` (the minimum beside it).

``--profile DIR`` instead re-runs this script (the device timings only, under ``timeout``) below ``rocprofv3 --kernel-trace
--stats`` and prints the per-kernel split of its stats file."""
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

THR, GATE, ROUNDS, MAX_STEPS = 16.0, 10, 2, 20


def problem(views: int, lo: int, hi: int, seed: int):
    """(K, points (P, 3), view_indices, point_indices, pixels) in ``register_views``'s layout: every view a rotation of 0.05 to
    0.4 rad about a random axis and t uniform in [-0.5, 0.5]^3, 0.5 px of noise, 30 % of its pixels replaced."""
    from structure_from_motion_amd import synthetic

    K = synthetic.BENCH_K
    rng = np.random.default_rng(seed)
    points = np.column_stack([rng.uniform(-1, 1, hi), rng.uniform(-1, 1, hi), rng.uniform(4, 6, hi)])
    view, index, pixels = [], [], []
    for v, n in enumerate(rng.integers(lo, hi + 1, views)):
        a = rng.normal(size=3)
        a *= rng.uniform(0.05, 0.4) / np.linalg.norm(a)
        th = float(np.linalg.norm(a))
        k = a / th
        W = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R = np.eye(3) + np.sin(th) * W + (1.0 - np.cos(th)) * (W @ W)
        t = rng.uniform(-0.5, 0.5, 3)
        idx = rng.permutation(hi)[:n]
        uvw = (points[idx] @ R.T + t) @ K.T
        uv = uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, 0.5, (n, 2))
        out = rng.random(n) < 0.3
        uv[out] = np.column_stack([rng.uniform(0, 2 * K[0, 2], n), rng.uniform(0, 2 * K[1, 2], n)])[out]
        view.append(np.full(n, v, dtype=np.int64)), index.append(idx.astype(np.int64)), pixels.append(uv)
    return K, points, np.concatenate(view), np.concatenate(index), np.concatenate(pixels)


def _stats(values):
    return sorted(values)[len(values) // 2], min(values)


def time_all(views: int, lo: int, hi: int, h: int, steps: int, warmup: int, seed: int, device_only: bool) -> dict:
    import torch

    from structure_from_motion_amd import device
    from structure_from_motion_amd.pnp.registration import ragged_order, register_views

    dev = device.require_gpu()
    K, points, view, index, pixels = problem(views, lo, hi, seed)
    order, offset = ragged_order(view, views)
    pts = np.ascontiguousarray(np.column_stack([points[index[order]], pixels[order]]))
    counts = np.diff(offset)
    pts_t, offset_t = device.to_device(pts), device.to_device(offset, torch.int64)
    gate_t = device.to_device(np.full(views, float(GATE)))
    ws = device.RegisterViewsWorkspace(views, len(pts), h, dev)
    singles = [(device.PnPWorkspace(1, int(n), h, dev), pts_t[offset[v]:offset[v + 1]].reshape(1, int(n), 5))
               for v, n in enumerate(counts)]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def ragged():
        start.record()
        ws.run(pts_t, offset_t, gate_t, K, THR, 3, seed, 1, 0, ROUNDS, MAX_STEPS)
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    def single():
        total = 0.0
        for v, (one, items) in enumerate(singles):
            start.record()
            one.run(items, K, THR, GATE, 3, philox=(seed + v, 0, 1), solver="p3p")
            one.refine(items, K, THR, 3, rounds=ROUNDS, max_steps=MAX_STEPS)
            end.record()
            end.synchronize()
            total += start.elapsed_time(end)
        return total

    for _ in range(warmup):
        ragged(), single()
    t_ragged, t_single = [], []
    for _ in range(steps):
        t_ragged.append(ragged()), t_single.append(single())
    status = device.read_register_status(ws.status)
    info = device.read_pnp_refine_info(ws.info)
    out = {"views": views, "items": int(len(pts)), "items_per_view": [int(counts.min()), int(counts.max())], "hypotheses": h,
           "refine_rounds": ROUNDS, "calls": steps,
           "ragged_device_ms": _stats(t_ragged)[0], "ragged_device_min_ms": _stats(t_ragged)[1],
           "single_device_ms": _stats(t_single)[0], "single_device_min_ms": _stats(t_single)[1],
           "views_ok": int(np.count_nonzero(status == device.REGISTER_OK)), "rounds_kept": int(sum(r.accepted for r in info)),
           "lm_steps": int(sum(r.lm_steps for r in info))}
    out["device_ratio_single_over_ragged"] = out["single_device_ms"] / out["ragged_device_ms"]
    if device_only:
        return out

    from structure_from_motion_amd.common.feature import Feature
    from structure_from_motion_amd.feature_matching.matching import Match
    from structure_from_motion_amd.pnp.pnp import estimate_pose_pnp_with_ransac

    def host_ragged():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        register_views(K, points, view, index, pixels, THR, num_views=views, min_num_extra_inliers=GATE, max_iterations=h,
                       refine_rounds=ROUNDS, refine_max_steps=MAX_STEPS, seed=seed)
        return (time.perf_counter() - t0) * 1e3

    t0 = time.perf_counter()
    lists = []
    for v in range(views):
        obs = order[offset[v]:offset[v + 1]]
        lists.append(([points[p] for p in index[obs]], [Feature(float(x), float(y)) for x, y in pixels[obs]],
                      [Match(a_index=i, b_index=i) for i in range(len(obs))]))
    out["loop_list_building_ms"] = (time.perf_counter() - t0) * 1e3

    def host_loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for X, features, matches in lists:
            estimate_pose_pnp_with_ransac(K, X, features, matches, THR, min_num_extra_inliers=GATE, max_iterations=h,
                                          refine_rounds=ROUNDS, solver="p3p")
        return (time.perf_counter() - t0) * 1e3

    os.environ["SFM_SAMPLER"] = "philox"
    os.environ["SFM_SEED"] = str(seed)
    os.environ["SFM_DEGENERATE"] = "skip"   # a collinear sample is skipped, as the ragged call skips it
    for _ in range(warmup):
        host_ragged(), host_loop()
    h_ragged, h_loop = [], []
    for _ in range(steps):
        h_ragged.append(host_ragged()), h_loop.append(host_loop())
    out.update(ragged_host_ms=_stats(h_ragged)[0], ragged_host_min_ms=_stats(h_ragged)[1], loop_host_ms=_stats(h_loop)[0],
               loop_host_min_ms=_stats(h_loop)[1])
    out["host_ratio_loop_over_ragged"] = out["loop_host_ms"] / out["ragged_host_ms"]
    return out


def profile(out_dir: str, args) -> dict:
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
           "-o", "register_views", "--", sys.executable, os.path.abspath(__file__), "--device-only", "--views", str(args.views),
           "--min-items", str(args.min_items), "--max-items", str(args.max_items), "--hypotheses", str(args.hypotheses), "--steps",
           str(args.steps), "--warmup", str(args.warmup), "--seed", str(args.seed)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise SystemExit(f"profiled run failed ({proc.returncode}):\n{proc.stderr[-2000:]}")
    stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    split = {}
    if stats:
        with open(stats[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                if any(key in name for key in ("register_", "ragged_", "pnp", "p3p", "select", "mask_kernel")):
                    split[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                   "total_ms": float(row["TotalDurationNs"]) / 1e6, "percent": float(row["Percentage"])}
    return {"kernels": split, "timing": proc.stdout.strip().splitlines()[-1:]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--min-items", type=int, default=200)
    ap.add_argument("--max-items", type=int, default=5000)
    ap.add_argument("--hypotheses", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=9, help="timed repetitions of each figure")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device-only", action="store_true", help="the two device timings only")
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the profiled run")
    args = ap.parse_args()
    if args.profile:
        print(json.dumps(profile(args.profile, args)), flush=True)
    else:
        print(json.dumps(time_all(args.views, args.min_items, args.max_items, args.hypotheses, args.steps, args.warmup, args.seed,
                                  args.device_only)), flush=True)


if __name__ == "__main__":
    main()
