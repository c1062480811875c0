"""Timing of the sub-pixel track refinement: ``sfm_refine_observations`` at radius 7 for 10^5 and 10^6
observations on the pyramids of four 1920 x 1080 views, device time by HIP events around the C call (the table upload is
inside), the median of ``--reps`` calls after two warm-ups.  One JSON line per size, with the mean number of Gauss-Newton solves
of the observations that are no references and the count per status.

The views show one band-limited texture under small rotations; a track is one texture point seen in all four views on a random
pyramid level each, its first observation the reference; warp0 is the true map between the two planes turned by up to 6 degrees,
as an orientation bin would leave it.

    python tools/bench_track_refine.py [--reps 10] [--observations 100000 1000000]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from structure_from_motion_amd import device  # noqa: E402
from structure_from_motion_amd.feature_matching import keypoints as kp  # noqa: E402
from structure_from_motion_amd.multiview.track_refinement import STATUS_NAMES  # noqa: E402

HEIGHT, WIDTH, VIEWS, LEVELS, RADIUS = 1080, 1920, 4, 8, 7
DEGREES = (0.0, 7.0, -11.0, 16.0)
WAVES = ((0.061, 0.023, 0.3, 1.0), (-0.034, 0.071, 1.1, 0.9), (0.093, -0.047, 2.0, 0.7), (0.017, 0.102, 0.7, 0.8),
         (0.128, 0.064, 2.6, 0.5), (-0.081, -0.119, 1.7, 0.5), (0.142, -0.012, 0.2, 0.4), (0.032, 0.033, 2.9, 1.1))


def rotation(degrees):
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def view_map(degrees):
    """[2, 3]: pixel -> canvas, a rotation about the image centre."""
    R, centre = rotation(degrees), np.array([(WIDTH - 1) / 2.0, (HEIGHT - 1) / 2.0])
    return np.column_stack([R, centre - R @ centre])


def render(A):
    x, y = np.meshgrid(np.arange(WIDTH, dtype=np.float64), np.arange(HEIGHT, dtype=np.float64))
    X, Y = A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2]
    total = sum(w[3] * np.sin(2.0 * np.pi * (w[0] * X + w[1] * Y) + w[2]) for w in WAVES)
    return np.clip(np.floor(127.5 + 127.5 * total / sum(w[3] for w in WAVES) + 0.5), 0, 255).astype(np.uint8)


def observations(M, rows, maps, rng):
    """plane, x, y, reference int32 [M] and warp0 float64 [M, 4]: tracks of VIEWS observations."""
    tracks = (M + VIEWS - 1) // VIEWS
    points = np.column_stack([rng.uniform(0.3 * WIDTH, 0.7 * WIDTH, tracks), rng.uniform(0.3 * HEIGHT, 0.7 * HEIGHT, tracks)])
    plane_of = {(r[0], r[1]): p for p, r in enumerate(rows)}
    level = rng.integers(0, 4, (tracks, VIEWS))
    plane, xy, linear = np.zeros((tracks, VIEWS), np.int32), np.zeros((tracks, VIEWS, 2)), np.zeros((tracks, VIEWS, 2, 2))
    for v in range(VIEWS):
        for l in range(4):
            mine = level[:, v] == l
            s = 1.25 ** l
            L = maps[v][:, :2] * s                       # level pixel -> canvas
            offset = maps[v][:, :2] @ np.array([0.5 * s - 0.5, 0.5 * s - 0.5]) + maps[v][:, 2]
            xy[mine, v] = np.rint(np.linalg.solve(L, (points[mine] - offset).T).T)
            linear[mine, v] = L
            plane[mine, v] = plane_of[(v, l)]
    turn = np.deg2rad(rng.uniform(-6.0, 6.0, (tracks, VIEWS)))
    c, s = np.cos(turn), np.sin(turn)
    off = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)
    warp = np.linalg.inv(linear) @ linear[:, :1] @ off     # reference offsets -> the observation's
    warp[:, 0] = np.eye(2)
    first = np.repeat(np.arange(tracks) * VIEWS, VIEWS).reshape(tracks, VIEWS)
    reference = np.where(np.arange(VIEWS)[None, :] == 0, -1, first)
    flat = lambda a, *shape: np.ascontiguousarray(a.reshape(tracks * VIEWS, *shape)[:M])  # noqa: E731
    return (flat(plane), flat(xy[..., 0]).astype(np.int32), flat(xy[..., 1]).astype(np.int32), flat(reference).astype(np.int32),
            flat(warp, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--observations", type=int, nargs="+", default=[100_000, 1_000_000])
    args = ap.parse_args()
    dev = device.require_gpu()
    maps = [view_map(d) for d in DEGREES]
    images = [render(A) for A in maps]
    layout = kp.plan([im.shape for im in images], 1, LEVELS)
    pool = torch.empty((layout.pool_bytes,), dtype=torch.uint8, device=dev)
    host = np.concatenate([im.reshape(-1) for im in images])
    pool[:host.size].copy_(torch.as_tensor(host))
    table = device.keypoint_plane_table(layout.rows)
    workspace = device.build_pyramid(table, len(layout.rows), VIEWS, pool)
    rng = np.random.default_rng(0)
    for M in args.observations:
        plane, x, y, reference, warp0 = (torch.as_tensor(a).to(dev) for a in observations(M, layout.rows, maps, rng))
        xy, warp = torch.empty((M, 2), dtype=torch.float64, device=dev), torch.empty((M, 4), dtype=torch.float64, device=dev)
        correlation = torch.empty((M,), dtype=torch.float64, device=dev)
        iterations, status = torch.empty((M,), dtype=torch.int32, device=dev), torch.empty((M,), dtype=torch.int32, device=dev)

        def call():
            device.refine_observations(table, len(layout.rows), VIEWS, pool, plane, x, y, reference, warp0, RADIUS, 10, 1e-3, 3.0,
                                       0.8, xy, warp, correlation, iterations, status, workspace)
        times = []
        for rep in range(args.reps + 2):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times.append(start.elapsed_time(stop))
        moving = (reference >= 0).cpu().numpy()
        solves, codes = iterations.cpu().numpy(), status.cpu().numpy()
        counts = np.bincount(codes, minlength=len(STATUS_NAMES))
        ms = float(np.median(times))
        print(json.dumps(dict(observations=M, aligned=int(moving.sum()), radius=RADIUS, planes=len(layout.rows),
                              pool_mb=layout.pool_bytes / 1e6, ms=ms, ms_min=float(min(times)), ms_max=float(max(times)),
                              ns_per_aligned_observation=1e6 * ms / max(1, int(moving.sum())),
                              mean_solves=float(solves[moving].mean()), total_solves=int(solves.sum()),
                              ns_per_solve=1e6 * ms / max(1, int(solves.sum())),
                              status={n: int(c) for n, c in zip(STATUS_NAMES, counts)})), flush=True)


if __name__ == "__main__":
    main()
