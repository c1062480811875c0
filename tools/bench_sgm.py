"""Timing of the semi-global smoothing of a plane-sweep cost volume (``sfm_sgm_aggregate``) for
profiles/sgm/README.md: the cost volumes of rendered views of 640 x 480 with D = 128 hypotheses, as ``tools/bench_plane_sweep.py``
sweeps them.  One JSON line with

* ``sweep_ms``: for R = 1 and R = 8 references, the sweep that writes the volume (``PlaneSweepWorkspace.run``), re-measured here;
* ``sgm_ms``: ``SgmWorkspace.run`` on that volume where it lies, for 4 and 8 paths, without and with the aggregated volume, HIP
  events around the call (all ``paths + 1`` launches and the allocation of the running sum when it is not kept);
* ``traffic_ms``: the least time the smoothing's traffic takes, one read of C and a read and a write of S per direction (the
  first direction does not read S), the winners' read of C and S, at ``--tbps`` terabytes a second;

every time the median of ``--steps`` timed repetitions after ``--warmup`` (the minimum beside it)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def traffic_ms(refs, height, width, depths, paths, tbps):
    return refs * height * width * depths * 8 * (3 * paths - 1 + 2) / (tbps * 1e12) * 1e3


def _stats(values):
    return {"median": sorted(values)[len(values) // 2], "min": min(values)}


def time_all(height, width, views, depths, sources, radius, steps, warmup, seed, tbps):
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

    out = {"height": height, "width": width, "depths": depths, "sources": sources, "radius": radius, "tbps": tbps, "sweep_ms": {},
           "sgm_ms": {}, "traffic_ms": {}, "changed_winners": {}}
    for refs in (1, 8):
        refs_t = device.to_device(np.arange(refs), torch.int32)
        sources_t = device.to_device(table[:refs], torch.int32)
        depths_t = device.to_device(np.ascontiguousarray(np.broadcast_to(z, (refs, depths))))
        sweep = device.PlaneSweepWorkspace(refs, height, width, depths, dev, volume=True)
        out["sweep_ms"][f"R={refs} volume"] = timed(lambda: sweep.run(images, K, poses_t, refs_t, sources_t, depths_t, radius, 0, 1, 1.0))
        for paths in (4, 8):
            for keep in (False, True):
                ws = device.SgmWorkspace(refs, height, width, depths, dev, aggregated=keep)
                out["sgm_ms"][f"R={refs} paths={paths}{' aggregated' if keep else ''}"] = timed(
                    lambda: ws.run(sweep.volume, depths_t, 0.1, 0.8, 1.0, paths))
                out["changed_winners"][f"R={refs} paths={paths}"] = float((ws.index != sweep.index).double().mean().item())
                del ws
            out["traffic_ms"][f"R={refs} paths={paths}"] = traffic_ms(refs, height, width, depths, paths, tbps)
        del sweep
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
    ap.add_argument("--tbps", type=float, default=6.3, help="the streaming rate the traffic bound is computed with")
    a = ap.parse_args()
    if a.views < 9:
        ap.error("--views must be at least 9: eight references with distinct sources")
    print(json.dumps(time_all(a.height, a.width, a.views, a.depths, a.sources, a.radius, a.steps, a.warmup, a.seed, a.tbps)))


if __name__ == "__main__":
    main()
