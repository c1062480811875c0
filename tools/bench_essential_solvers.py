"""Eight-point against five-point essential-matrix RANSAC on one GPU (results in profiles/five_point/README.md).

Reports, as one JSON object:
  fit_ms_per_100k   the fit launch alone over 100 000 hypotheses (5 000 correspondences), both solvers;
  pass_ms           a whole pass (fit, scoring, selection, mask) over 5 000 correspondences at the 99 %-confidence
                    hypothesis counts of each solver at 50 % and 70 % outliers (8 items: 1 177 / 70 188, 6 items: 293 / 6 315);
  to_pose           wall time of estimate_essential_mat_with_ransac (Philox sampler) at those counts on a 5 000-match scene
                    with 50 % / 70 % outliers, and the rotation error of the pose it leads to.

    python tools/bench_essential_solvers.py [--repeats 20]
"""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from structure_from_motion_amd import device, synthetic  # noqa: E402
from structure_from_motion_amd._native import AGG_RMS  # noqa: E402
from structure_from_motion_amd.common.feature import Feature  # noqa: E402
from structure_from_motion_amd.epipolar import epipolar_ransac as er  # noqa: E402
from structure_from_motion_amd.epipolar.eight_point import recover_r_t_from_e  # noqa: E402
from structure_from_motion_amd.feature_matching.matching import Match  # noqa: E402

SAMPLE = {"eight_point": 8, "five_point": 6}


def hypotheses(solver, outliers, confidence=0.99):
    return math.ceil(math.log(1.0 - confidence) / math.log(1.0 - (1.0 - outliers) ** SAMPLE[solver]))


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats):
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


def scene_corr(n, outliers, seed):
    pa, pb, K, R, t, is_out = synthetic.two_view_scene(n, seed=seed, outlier_fraction=outliers, noise_px=0.5)
    corr = device.normalize_correspondences(device.to_device(pa), device.to_device(pb), K)
    return pa, pb, K, R, corr


def rotation_error(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    device.require_gpu()
    out = {"fit_ms_per_100k": {}, "pass_ms": {}, "to_pose": {}}
    n = 5000
    *_, corr = scene_corr(n, 0.5, 1)
    c = corr.reshape(1, n, 4)
    S = device.sample_philox(3, 0, 100_000, n)
    E = torch.empty((1, 100_000, 9), dtype=torch.float64, device=c.device)
    flags = torch.empty((1, 100_000), dtype=torch.int32, device=c.device)
    out["fit_ms_per_100k"]["eight_point"] = timed(lambda: device.fit_eight_point(c, S, E, flags), args.repeats)
    out["fit_ms_per_100k"]["five_point"] = timed(lambda: device.five_point_fit(c, S, E, flags), args.repeats)
    for outliers in (0.5, 0.7):
        for solver in ("eight_point", "five_point"):
            h = hypotheses(solver, outliers)
            ws = device.RansacWorkspace(1, n, h)
            kw = {} if solver == "eight_point" else {"solver": solver}
            ms = timed(lambda: ws.run(c, 2e-5, 10, AGG_RMS, philox=(5, 0, 1), **kw), args.repeats)
            out["pass_ms"][f"{solver}@{int(outliers * 100)}%_H={h}"] = ms
    os.environ["SFM_SAMPLER"] = "philox"
    for outliers in (0.5, 0.7):
        pa, pb, K, R, corr = scene_corr(n, outliers, 2)
        fa = [Feature(float(x), float(y)) for x, y in pa]
        fb = [Feature(float(x), float(y)) for x, y in pb]
        matches = [Match(a_index=i, b_index=i) for i in range(n)]
        for solver in ("eight_point", "five_point"):
            h = hypotheses(solver, outliers)
            walls, errs = [], []
            for rep in range(5):
                os.environ["SFM_SEED"] = str(100 + rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    e, inl = er.estimate_essential_mat_with_ransac(K, fa, fb, matches, 2e-5, min_num_extra_inliers=int(0.3 * n * (1 - outliers)),
                                                                   max_iterations=h, solver=solver)
                    R2, _, _ = recover_r_t_from_e(e, K, [p[0] for p in inl], [p[1] for p in inl])
                    errs.append(rotation_error(R2, R))
                except ValueError:
                    errs.append(float("nan"))
                walls.append((time.perf_counter() - t0) * 1e3)
            out["to_pose"][f"{solver}@{int(outliers * 100)}%_H={h}"] = {
                "wall_ms_median": float(np.median(walls)), "rotation_error_rad_median": float(np.nanmedian(errs)),
                "rotation_error_rad_max": float(np.nanmax(errs)), "runs_without_model": int(np.isnan(errs).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
