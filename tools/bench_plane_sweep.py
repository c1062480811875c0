"""Timing of the plane sweep and of the consistency filter (``sfm_plane_sweep``, ``sfm_filter_depth_maps``) for
profiles/plane_sweep/README.md: nine rendered views of 640 x 480, D = 128 hypotheses, S = 4 sources, radius 3.  One JSON line with

* ``sweep_ms``: for R = 1 and R = 8 references, ``PlaneSweepWorkspace.run`` on device-resident inputs, HIP events around the call
  (both launches), without and with the cost volume;
* ``filter_ms``: ``device.filter_depth_maps`` over the nine depth maps of a sweep, HIP events around the call;
* ``floor_ms``: the least time the fp64 pipe needs for the sweep's window sums alone, the five operations per window pixel,
  source and depth (b added, b b and a b multiplied and added) at 16 fp64 lanes per SIMD and clock, 4 SIMDs, 256 CUs, 2.4 GHz;

every time the median of ``--steps`` timed repetitions after ``--warmup`` (the minimum beside it)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP64_LANE_OPS_PER_SECOND = 256 * 4 * 16 * 2.4e9


def floor_ms(refs, height, width, depths, sources, radius):
    return refs * height * width * depths * sources * 5 * (2 * radius + 1) ** 2 / FP64_LANE_OPS_PER_SECOND * 1e3


def _stats(values):
    return {"median": sorted(values)[len(values) // 2], "min": min(values)}


def time_all(height, width, views, depths, sources, radius, steps, warmup, seed):
    import torch

    from structure_from_motion_amd import device, synthetic
    from structure_from_motion_amd.stereo.depth_maps import depth_hypotheses

    dev = device.require_gpu()
    c, s = np.cos(np.radians(25.0)), np.sin(np.radians(25.0))
    planes = [((0.0, 0.0, 5.0), (c, 0.0, s), (0.0, 1.0, 0.0), None), ((0.1, 0.0, 3.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.45, 0.5))]
    poses = synthetic.arc_poses(views, 2.0, 5.0)
    scene = synthetic.plane_views(height, width, poses, planes, seed=seed, texels_per_unit=96.0, texture_size=512)
    z = depth_hypotheses(np.nanmin(scene["depth"]) / 1.05, np.nanmax(scene["depth"]) * 1.05, depths)
    table = np.array([sorted((u for u in range(views) if u != v), key=lambda u, v=v: (abs(u - v), u))[:sources] for v in range(views)],
                     dtype=np.int32)
    images, K, poses_t = device.to_device(scene["images"], torch.uint8), device.to_device(scene["K"].reshape(9)), device.to_device(poses)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(steps):
            start.record()
            call()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return _stats(times)

    out = {"height": height, "width": width, "views": views, "depths": depths, "sources": sources, "radius": radius, "sweep_ms": {},
           "floor_ms": {}}
    for refs in (1, 8):
        refs_t = device.to_device(np.arange(refs), torch.int32)
        sources_t = device.to_device(table[:refs], torch.int32)
        depths_t = device.to_device(np.ascontiguousarray(np.broadcast_to(z, (refs, depths))))
        for volume in (False, True):
            ws = device.PlaneSweepWorkspace(refs, height, width, depths, dev, volume=volume)
            out["sweep_ms"][f"R={refs}{' volume' if volume else ''}"] = timed(
                lambda: ws.run(images, K, poses_t, refs_t, sources_t, depths_t, radius, 0, 1, 1.0))
            del ws
        out["floor_ms"][f"R={refs}"] = floor_ms(refs, height, width, depths, sources, radius)
    all_refs, all_sources = device.to_device(np.arange(views), torch.int32), device.to_device(table, torch.int32)
    ws = device.PlaneSweepWorkspace(views, height, width, depths, dev)
    ws.run(images, K, poses_t, all_refs, all_sources, device.to_device(np.ascontiguousarray(np.broadcast_to(z, (views, depths)))), radius,
           0, 1, 1.0)
    buffers = device.filter_depth_maps(ws.depth, K, poses_t, all_refs, all_sources, 1.0, 0.01, 2)
    out["filter_ms"] = timed(lambda: device.filter_depth_maps(ws.depth, K, poses_t, all_refs, all_sources, 1.0, 0.01, 2, out=buffers))
    out["filter_kept"] = float(torch.isfinite(buffers[1]).double().mean().item())
    out["winners"] = float((ws.index >= 0).double().mean().item())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--depths", type=int, default=128)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.views < 9:
        ap.error("--views must be at least 9: eight references with distinct sources")
    print(json.dumps(time_all(a.height, a.width, a.views, a.depths, a.sources, a.radius, a.steps, a.warmup, a.seed)))


if __name__ == "__main__":
    main()
