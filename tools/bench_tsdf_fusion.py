"""Timing of the fusion (``sfm_tsdf_integrate``, ``sfm_tsdf_extract_mesh``) for profiles/tsdf_fusion/README.md: the
exact depth maps of 32 rendered views of 640 x 480 of the two-plane scene of apps/fuse_depth_maps.py, fused into 256^3 voxels.  One
JSON line with

* ``integrate_ms``: for N = 1, 8 and 32 views per call, without and with grey, the ``tsdf_integrate_`` op on device-resident
  inputs, HIP events around the call (one launch), and ``integrate_gb_per_s``: the traffic the definition cannot avoid (sum and
  count read and written once per voxel and call, 24 bytes, 32 with grey) over that time;
* ``extract_ms``: ``tsdf_extract_mesh_`` on the volume after all 32 views: ``count_only`` with max_triangles = 0 (the count, the
  scan and the tail's one block) and ``full`` with room for every triangle (all six launches); ``triangles`` is their number;

every time the median of ``--steps`` timed repetitions after ``--warmup`` (the minimum beside it)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _stats(values):
    return {"median": sorted(values)[len(values) // 2], "min": min(values)}


def time_all(height, width, views, voxels, steps, warmup, seed):
    import torch

    from structure_from_motion_amd import device, ops, synthetic

    dev = device.require_gpu()
    op = ops.load()
    c, s = np.cos(np.radians(25.0)), np.sin(np.radians(25.0))
    planes = [((0.0, 0.0, 5.0), (c, 0.0, s), (0.0, 1.0, 0.0), None), ((0.1, 0.0, 3.6), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.45, 0.5))]
    poses = synthetic.arc_poses(views, 1.0, 5.0)
    scene = synthetic.plane_views(height, width, poses, planes, seed=seed, texels_per_unit=96.0, texture_size=512)
    size = 4.0 / voxels                     # a cube of 4 units about (0, 0, 4.9): both planes inside the images' frustum
    origin, truncation = (-2.0, -2.0, 2.9), 4.0 * size
    depth, images = device.to_device(scene["depth"]), device.to_device(scene["images"], torch.uint8)
    K, poses_t = device.to_device(scene["K"].reshape(9)), device.to_device(poses)
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

    shape = (voxels, voxels, voxels)
    out = {"height": height, "width": width, "views": views, "voxels": voxels, "integrate_ms": {}, "integrate_gb_per_s": {}}
    for grey in (False, True):
        state = (torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.int32, device=dev),
                 torch.zeros(shape, dtype=torch.int32, device=dev) if grey else None)
        for n in (1, 8, 32):
            listed = device.to_device(np.arange(n) % views, torch.int32)
            status = torch.empty((n,), dtype=torch.int32, device=dev)
            key = f"N={n}{' grey' if grey else ''}"
            out["integrate_ms"][key] = timed(lambda: op.tsdf_integrate_(state[0], state[1], state[2], depth, images if grey else None, K,
                                                                        poses_t, listed, *origin, size, truncation, status))
            out["integrate_gb_per_s"][key] = voxels ** 3 * (32 if grey else 24) / out["integrate_ms"][key]["median"] / 1e6
        del state
    state = [torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.int32, device=dev),
             torch.zeros(shape, dtype=torch.int32, device=dev)]
    every = device.to_device(np.arange(views), torch.int32)
    op.tsdf_integrate_(*state, depth, images, K, poses_t, every, *origin, size, truncation, torch.empty((views,), dtype=torch.int32, device=dev))
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    none = (torch.empty((0, 3, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.float64, device=dev), total)
    out["extract_ms"] = {"count_only": timed(lambda: op.tsdf_extract_mesh_(*state, *origin, size, 2, *none))}
    triangles = int(total.item())
    rows = (torch.empty((triangles, 3, 3), dtype=torch.float64, device=dev), torch.empty((triangles, 3), dtype=torch.float64, device=dev), total)
    out["extract_ms"]["full"] = timed(lambda: op.tsdf_extract_mesh_(*state, *origin, size, 2, *rows))
    out["triangles"] = triangles
    out["voxels_seen_twice"] = float((state[1] >= 2).double().mean().item())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--voxels", type=int, default=256, help="voxels along each axis of the cube")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.views < 1 or a.voxels < 2:
        ap.error("--views must be at least 1 and --voxels at least 2")
    print(json.dumps(time_all(a.height, a.width, a.views, a.voxels, a.steps, a.warmup, a.seed)))


if __name__ == "__main__":
    main()
