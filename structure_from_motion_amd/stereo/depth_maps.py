"""Dense depth maps from posed images: plane-sweep stereo for every reference view in one device call per chunk, the
forward-backward consistency filter across the maps, and the fused point cloud (csrc/sfm_plane_sweep.hip); the
semi-global smoothing of the sweep's cost volume (csrc/sfm_sgm.hip; tests/sgm_oracle.py is its definition).

The device results are defined as a fixed sequence of float64 operations (tests/plane_sweep_oracle.py is the same sequence in
NumPy): a call is reproducible bit for bit, and how the references are split into device calls never changes a result.  The
helpers ``depth_hypotheses``, ``depth_ranges`` and ``select_source_views`` are NumPy only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..epipolar.view_graph import chunk_bounds

MAX_SOURCES, MAX_DEPTHS, MAX_RADIUS = 8, 4096, 5
MAX_SGM_DEPTHS, SGM_PATHS = 256, (4, 8)   # what sfm_sgm_aggregate accepts


@dataclass
class DepthMaps:
    """What ``compute_depth_maps`` returns, on the host.  ``depth`` (R, H, W): the winning hypothesis after the sub-sample step, NaN
    without a winner; ``index`` (R, H, W) int32: the winner, -1 without; ``cost`` (R, H, W): its cost; ``refs`` (R,): the view of
    each map; ``volume`` (R, D, H, W) or None: the cost of every hypothesis, NaN where invalid; ``images``: the grey images the
    maps were computed from (V, H, W) uint8."""
    depth: np.ndarray
    index: np.ndarray
    cost: np.ndarray
    refs: np.ndarray
    volume: Optional[np.ndarray]
    images: np.ndarray


@dataclass
class FilteredDepthMaps:
    """What ``filter_depth_maps`` returns, on the host.  ``depth`` (R, H, W): the depth where at least ``min_consistent`` sources
    agree, else NaN; ``count`` (R, H, W) int32: the agreeing sources; ``points`` (R, H, W, 3): the world point of a kept pixel,
    else NaN; ``refs`` (R,); ``images`` as in ``DepthMaps``."""
    depth: np.ndarray
    count: np.ndarray
    points: np.ndarray
    refs: np.ndarray
    images: np.ndarray


def _integer(value, name: str, low: int, high: Optional[int] = None) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low or (high is not None and value > high):
        bound = f">= {low}" if high is None else f"in [{low}, {high}]"
        raise ValueError(f"{name} must be an integer {bound}, got {value!r}")
    return int(value)


def _bound(value, name: str) -> float:
    value = float(value)
    if not (np.isfinite(value) and value >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {value!r}")
    return value


def _camera(K) -> np.ndarray:
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera matrix must be 3x3, got shape {K.shape}")
    if not np.all(np.isfinite(K)) or K[0, 0] == 0.0 or K[1, 1] == 0.0:
        raise ValueError("the camera matrix must be finite with non-zero K[0,0] and K[1,1]")
    if K[1, 0] != 0.0 or not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise ValueError("the camera matrix must be upper triangular with row 2 equal to (0, 0, 1)")
    return K


def _poses(poses, views: int) -> np.ndarray:
    poses = np.asarray(poses, dtype=np.float64)
    if poses.shape != (views, 12):
        raise ValueError(f"poses must have shape ({views}, 12): R row-major, then t, got {poses.shape}")
    if not np.all(np.isfinite(poses)):
        raise ValueError("poses must be finite")
    return np.ascontiguousarray(poses)


def _refs_and_sources(refs, sources, views: int):
    """refs (R,) int32 in [0, views), default all views; sources (R, S) int32, -1 for an absent slot, 1 <= S <= 8."""
    if refs is None:
        refs = np.arange(views)
    refs = np.asarray(refs)
    if refs.ndim != 1 or (refs.size and not np.issubdtype(refs.dtype, np.integer)):
        raise ValueError(f"refs must be a list of view indices, got shape {refs.shape} and dtype {refs.dtype}")
    if refs.size and (refs.min() < 0 or refs.max() >= views):
        raise ValueError(f"refs must index views 0 .. {views - 1}")
    R = len(refs)
    if sources is None:   # every other view, nearest indices first
        if views < 2:
            raise ValueError("sources=None needs at least two views")
        width = min(MAX_SOURCES, views - 1)
        sources = np.array([sorted((v for v in range(views) if v != r), key=lambda v, r=r: (abs(v - r), v))[:width] for r in refs],
                           dtype=np.int32).reshape(R, width)
    sources = np.asarray(sources)
    if sources.ndim != 2 or sources.shape[0] != R or not 1 <= sources.shape[1] <= MAX_SOURCES:
        raise ValueError(f"sources must have shape ({R}, S) with 1 <= S <= {MAX_SOURCES}, got {sources.shape}")
    if sources.size and not np.issubdtype(sources.dtype, np.integer):
        raise ValueError(f"sources must hold integers, got {sources.dtype}")
    if sources.size and (sources.min() < -1 or sources.max() >= views):
        raise ValueError(f"sources must hold view indices 0 .. {views - 1}, or -1 for an absent slot")
    return np.ascontiguousarray(refs, dtype=np.int32), np.ascontiguousarray(sources, dtype=np.int32)


def _penalties(p1, p2, invalid_cost=1.0, paths=8):
    """The scalars of ``sfm_sgm_aggregate`` as it accepts them: finite, 0 <= p1 <= p2, paths 4 or 8."""
    try:
        p1, p2, invalid_cost = float(p1), float(p2), float(invalid_cost)
    except (TypeError, ValueError):
        raise ValueError(f"p1, p2 and invalid_cost must be numbers, got {p1!r}, {p2!r} and {invalid_cost!r}") from None
    if not (np.isfinite(p1) and np.isfinite(p2) and np.isfinite(invalid_cost) and 0.0 <= p1 <= p2):
        raise ValueError(f"need finite p1, p2 and invalid_cost with 0 <= p1 <= p2, got {p1!r}, {p2!r} and {invalid_cost!r}")
    if isinstance(paths, bool) or not isinstance(paths, (int, np.integer)) or int(paths) not in SGM_PATHS:
        raise ValueError(f"paths must be 4 or 8, got {paths!r}")
    return p1, p2, invalid_cost, int(paths)


def regularize_depth_maps(depth_maps_or_volume, depths, p1: float = 0.1, p2: float = 0.8, invalid_cost: float = 1.0, paths: int = 8,
                          return_aggregated: bool = False, max_refs_per_call: int = 16) -> DepthMaps:
    """Depth maps from a cost volume smoothed by semi-global aggregation, all references of a chunk in one device call.

    ``depth_maps_or_volume``: a ``DepthMaps`` computed with ``return_volume=True``, or a (R, D, H, W) array, NaN where a
    hypothesis has no cost; ``depths``: the (R, D) or (D,) hypotheses the volume was swept with, D <= 256.  Along each of ``paths``
    (4 or 8) scanline directions a hypothesis pays its own cost (``invalid_cost`` where it has none) and the cheapest way to
    reach it from the pixel before: for nothing from the same hypothesis, for ``p1`` from a neighbouring one, for ``p2`` from any.
    The sums over the directions replace the costs: ``index`` is the hypothesis of lowest sum among those that have a cost and
    a valid depth, ``cost`` that sum, ``depth`` its depth after the sweep's parabola step on the sums, and ``volume`` the sums
    with ``return_aggregated`` (else None).  Every argument is checked before any device work (``ValueError``); how the
    references are split into calls of at most ``max_refs_per_call`` never changes a result."""
    refs = images = None
    if isinstance(depth_maps_or_volume, DepthMaps):
        if depth_maps_or_volume.volume is None:
            raise ValueError("regularize_depth_maps needs the cost volume: compute_depth_maps(..., return_volume=True)")
        volume, refs, images = depth_maps_or_volume.volume, depth_maps_or_volume.refs, depth_maps_or_volume.images
    else:
        volume = depth_maps_or_volume
    volume = np.asarray(volume, dtype=np.float64)
    if volume.ndim != 4 or not 1 <= volume.shape[1] <= MAX_SGM_DEPTHS or volume.shape[2] < 1 or volume.shape[3] < 1 or \
            volume.shape[2] * volume.shape[3] >= 2**31:
        raise ValueError(f"the volume must be (R, D, H, W) with 1 <= D <= {MAX_SGM_DEPTHS} and 1 <= H W < 2^31, got shape {volume.shape}")
    R, D, H, W = volume.shape
    depths = np.asarray(depths, dtype=np.float64)
    if depths.ndim == 1:
        depths = np.broadcast_to(depths, (R, len(depths)))
    if depths.shape != (R, D):
        raise ValueError(f"depths must have shape ({R}, {D}) or ({D},), got {depths.shape}")
    p1, p2, invalid_cost, paths = _penalties(p1, p2, invalid_cost, paths)
    chunks = chunk_bounds(R, 1, _integer(max_refs_per_call, "max_refs_per_call", 1))
    if refs is None:
        refs, images = np.arange(R, dtype=np.int32), np.zeros((R, H, W), dtype=np.uint8)
    if R == 0:
        return DepthMaps(np.zeros((0, H, W)), np.zeros((0, H, W), np.int32), np.zeros((0, H, W)), refs,
                         np.zeros((0, D, H, W)) if return_aggregated else None, images)
    from .. import device

    dev = device.require_gpu()
    depths_dev = device.to_device(np.ascontiguousarray(depths))
    parts = []
    for r0, r1 in chunks:
        ws = device.SgmWorkspace(r1 - r0, H, W, D, dev, aggregated=bool(return_aggregated))
        ws.run(device.to_device(np.ascontiguousarray(volume[r0:r1])), depths_dev[r0:r1], p1, p2, invalid_cost, paths)
        parts.append(ws)
    return DepthMaps(depth=np.concatenate([ws.depth.cpu().numpy() for ws in parts]),
                     index=np.concatenate([ws.index.cpu().numpy() for ws in parts]),
                     cost=np.concatenate([ws.cost.cpu().numpy() for ws in parts]), refs=refs,
                     volume=np.concatenate([ws.aggregated.cpu().numpy() for ws in parts]) if return_aggregated else None, images=images)


def compute_depth_maps(images, K, poses, depths, sources=None, refs=None, radius: int = 3, top_k: int = 0, min_sources: int = 1,
                       min_variance: float = 1.0, return_volume: bool = False, max_refs_per_call: int = 64,
                       smoothness=None) -> DepthMaps:
    """One depth map per reference view by plane-sweep stereo, all references of a chunk in one device call.

    ``images``: (V, H, W) uint8 grey, all of one size; ``K``: the shared upper-triangular camera matrix; ``poses``: (V, 12) world
    to camera, R row-major then t; ``depths``: (R, D) hypotheses per reference, or (D,) for all; ``sources``: (R, S) view indices
    per reference, -1 for an absent slot (default: the up to eight nearest view indices); ``refs``: (R,) views to compute
    (default: all).  A hypothesis is scored per source by 1 - NCC over a ``(2 radius + 1)^2`` window of the reference and the
    source warped through the plane's homography; a score is valid when both windows have a variance of at least
    ``min_variance`` grey levels squared; the cost of a hypothesis is the mean of its ``top_k`` lowest valid scores (0: all) and
    needs ``min_sources`` of them.  The winner of a pixel is refined by a parabola through its neighbours, in inverse depth.

    ``smoothness``: None, or the penalties ``(p1, p2)`` of ``regularize_depth_maps``: each chunk's cost volume is then smoothed
    on the device (8 paths, invalid cost 1) before the winners are taken, D <= 256; ``depth``, ``index`` and ``cost`` are those
    of ``regularize_depth_maps`` and ``volume`` stays the sweep's.

    Every argument is checked before any device work (``ValueError``).  Images go up in one upload; the references are split
    into calls of at most ``max_refs_per_call``, which never changes a result."""
    images = np.asarray(images)
    if images.ndim != 3 or images.dtype != np.uint8:
        raise ValueError(f"images must be a (V, H, W) uint8 array, got shape {images.shape} and dtype {images.dtype}")
    V, H, W = images.shape
    radius = _integer(radius, "radius", 1, MAX_RADIUS)
    if V < 1 or H < 2 * radius + 2 or W < 2 * radius + 2 or H * W >= 2**31:
        raise ValueError(f"need at least one image of at least {2 * radius + 2} pixels each way and fewer than 2^31 pixels, got {images.shape}")
    K = _camera(K)
    poses = _poses(poses, V)
    refs, sources = _refs_and_sources(refs, sources, V)
    R = len(refs)
    depths = np.asarray(depths, dtype=np.float64)
    if depths.ndim == 1:
        depths = np.broadcast_to(depths, (R, len(depths)))
    if depths.ndim != 2 or depths.shape[0] != R or not 1 <= depths.shape[1] <= MAX_DEPTHS:
        raise ValueError(f"depths must have shape ({R}, D) or (D,) with 1 <= D <= {MAX_DEPTHS}, got {depths.shape}")
    depths = np.ascontiguousarray(depths)
    D = depths.shape[1]
    top_k = _integer(top_k, "top_k", 0)
    min_sources = _integer(min_sources, "min_sources", 1)
    min_variance = _bound(min_variance, "min_variance")
    chunks = chunk_bounds(R, 1, _integer(max_refs_per_call, "max_refs_per_call", 1))
    if smoothness is not None:
        try:
            p1, p2 = smoothness
        except (TypeError, ValueError):
            raise ValueError(f"smoothness must be None or the two penalties (p1, p2), got {smoothness!r}") from None
        p1, p2, invalid_cost, paths = _penalties(p1, p2)
        if D > MAX_SGM_DEPTHS:
            raise ValueError(f"smoothness needs at most {MAX_SGM_DEPTHS} depth hypotheses, got {D}")
    if R == 0:
        return DepthMaps(np.zeros((0, H, W)), np.zeros((0, H, W), np.int32), np.zeros((0, H, W)), refs,
                         np.zeros((0, D, H, W)) if return_volume else None, images)
    import torch

    from .. import device

    dev = device.require_gpu()
    images_dev = device.to_device(images, torch.uint8)
    K_dev, poses_dev = device.to_device(K.reshape(9)), device.to_device(poses)
    refs_dev, sources_dev = device.to_device(refs, torch.int32), device.to_device(sources, torch.int32)
    depths_dev = device.to_device(depths)
    parts, maps = [], []
    for r0, r1 in chunks:
        ws = device.PlaneSweepWorkspace(r1 - r0, H, W, D, dev, volume=bool(return_volume) or smoothness is not None)
        ws.run(images_dev, K_dev, poses_dev, refs_dev[r0:r1], sources_dev[r0:r1], depths_dev[r0:r1], radius, top_k, min_sources,
               min_variance)
        parts.append(ws)
        # the smoothed maps of a chunk, from its volume where it lies; without smoothness the sweep's own
        maps.append(ws if smoothness is None else device.sgm_aggregate(ws.volume, depths_dev[r0:r1], p1, p2, invalid_cost, paths))
        if smoothness is not None and not return_volume:
            ws.volume = None
    code = np.concatenate([device.read_sweep_status(ws.status) for ws in parts])
    if np.any(code != device.SWEEP_OK):
        raise RuntimeError("compute_depth_maps: the device refused a reference index (SFM_SWEEP_BAD_REFERENCE)")
    return DepthMaps(depth=np.concatenate([ws.depth.cpu().numpy() for ws in maps]),
                     index=np.concatenate([ws.index.cpu().numpy() for ws in maps]),
                     cost=np.concatenate([ws.cost.cpu().numpy() for ws in maps]), refs=refs,
                     volume=np.concatenate([ws.volume.cpu().numpy() for ws in parts]) if return_volume else None, images=images)


def filter_depth_maps(depth_maps, K, poses, sources, max_pixel_error: float = 1.0, max_relative_depth_error: float = 0.01,
                      min_consistent: int = 2) -> FilteredDepthMaps:
    """Keep the depths that the maps of other views confirm.  ``depth_maps``: a ``DepthMaps`` holding one map per view (its
    ``refs`` must be 0 .. V-1 in order), or a (V, H, W) array with NaN for no depth; ``sources``: (V, S) view indices per view,
    -1 for an absent slot.  A pixel's point is carried into each source, to the nearest pixel there and back with that pixel's
    depth; the source agrees when it returns within ``max_pixel_error`` pixels and ``max_relative_depth_error`` of the depth.
    Pixels with fewer than ``min_consistent`` agreeing sources lose their depth.  Every argument is checked before any device
    work (``ValueError``)."""
    images = None
    if isinstance(depth_maps, DepthMaps):
        if not np.array_equal(depth_maps.refs, np.arange(len(depth_maps.refs))):
            raise ValueError("filter_depth_maps needs one depth map per view: depth_maps.refs must be 0 .. V-1 in order")
        depth, images = depth_maps.depth, depth_maps.images
    else:
        depth = depth_maps
    depth = np.asarray(depth, dtype=np.float64)
    if depth.ndim != 3 or depth.shape[0] < 1 or depth.shape[1] < 1 or depth.shape[2] < 1 or depth.shape[1] * depth.shape[2] >= 2**31:
        raise ValueError(f"depth maps must be a non-empty (V, H, W) array of fewer than 2^31 pixels a view, got shape {depth.shape}")
    V, H, W = depth.shape
    K = _camera(K)
    poses = _poses(poses, V)
    refs, sources = _refs_and_sources(None, sources, V)
    max_pixel_error = _bound(max_pixel_error, "max_pixel_error")
    max_relative_depth_error = _bound(max_relative_depth_error, "max_relative_depth_error")
    min_consistent = _integer(min_consistent, "min_consistent", 0)
    import torch

    from .. import device

    device.require_gpu()
    count, filtered, points, status = device.filter_depth_maps(
        device.to_device(np.ascontiguousarray(depth)), device.to_device(K.reshape(9)), device.to_device(poses),
        device.to_device(refs, torch.int32), device.to_device(sources, torch.int32), max_pixel_error, max_relative_depth_error,
        min_consistent)
    if np.any(device.read_sweep_status(status) != device.SWEEP_OK):
        raise RuntimeError("filter_depth_maps: the device refused a reference index (SFM_SWEEP_BAD_REFERENCE)")
    if images is None:
        images = np.zeros((V, H, W), dtype=np.uint8)
    return FilteredDepthMaps(depth=filtered.cpu().numpy(), count=count.cpu().numpy(), points=points.cpu().numpy(), refs=refs,
                             images=images)


def point_cloud(filtered: FilteredDepthMaps):
    """-> (points (N, 3), grey (N,) uint8, view (N,) int32): the finite points of the filtered maps, view by view in row-major
    pixel order, with the grey value of their pixel and the view they come from.  Host only."""
    keep = np.all(np.isfinite(filtered.points), axis=-1)
    view = np.broadcast_to(np.asarray(filtered.refs, dtype=np.int32)[:, None, None], keep.shape)
    grey = filtered.images[np.asarray(filtered.refs, dtype=np.int64)]
    return filtered.points[keep], grey[keep], view[keep]


def depth_hypotheses(near: float, far: float, count: int) -> np.ndarray:
    """``count`` depths from ``near`` to ``far``, both included, uniform in inverse depth (a constant step in disparity).  A
    single hypothesis is ``near``."""
    near, far = float(near), float(far)
    count = _integer(count, "count", 1, MAX_DEPTHS)
    if not (np.isfinite(near) and np.isfinite(far) and 0.0 < near <= far):
        raise ValueError(f"need 0 < near <= far, both finite, got {near!r} and {far!r}")
    if count == 1:
        return np.array([near])
    w = np.arange(count, dtype=np.float64) / (count - 1)
    z = 1.0 / ((1.0 - w) / near + w / far)
    z[0], z[-1] = near, far
    return z


def _observations(camera_indices, point_indices, cameras: Optional[int] = None, points: Optional[int] = None):
    cam, pt = np.asarray(camera_indices), np.asarray(point_indices)
    if cam.ndim != 1 or cam.shape != pt.shape:
        raise ValueError(f"camera_indices and point_indices must be two lists of one length, got {cam.shape} and {pt.shape}")
    if cam.size and not (np.issubdtype(cam.dtype, np.integer) and np.issubdtype(pt.dtype, np.integer)):
        raise ValueError("camera_indices and point_indices must hold integers")
    if cam.size and (cam.min() < 0 or pt.min() < 0 or (cameras is not None and cam.max() >= cameras) or
                     (points is not None and pt.max() >= points)):
        raise ValueError("camera_indices or point_indices out of range")
    return cam.astype(np.int64), pt.astype(np.int64)


def depth_ranges(poses, points, camera_indices, point_indices, margin: float = 0.1):
    """-> (near (V,), far (V,)): per view the least and largest camera depth of the sparse points it observes, widened by
    ``margin`` (near / (1 + margin), far * (1 + margin)).  Observations of points behind their camera or not finite are left
    out; a view with none gets NaN for both."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim != 2 or poses.shape[1] != 12:
        raise ValueError(f"poses must have shape (V, 12), got {poses.shape}")
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must have shape (P, 3), got {points.shape}")
    margin = _bound(margin, "margin")
    V = len(poses)
    cam, pt = _observations(camera_indices, point_indices, V, len(points))
    z = np.einsum("mk,mk->m", poses[cam, 6:9], points[pt]) + poses[cam, 11]
    ok = np.isfinite(z) & (z > 0.0)
    near, far = np.full(V, np.inf), np.full(V, -np.inf)
    np.minimum.at(near, cam[ok], z[ok])
    np.maximum.at(far, cam[ok], z[ok])
    seen = np.isfinite(near)
    return np.where(seen, near / (1.0 + margin), np.nan), np.where(seen, far * (1.0 + margin), np.nan)


def select_source_views(camera_indices, point_indices, num_views: int, count: int) -> np.ndarray:
    """-> (num_views, count) int32: for each view the ``count`` other views that observe most of its points (tracks), most
    first, ties to the lower index; views that share no point are not chosen, and the row is padded with -1."""
    num_views = _integer(num_views, "num_views", 1)
    count = _integer(count, "count", 1, MAX_SOURCES)
    cam, pt = _observations(camera_indices, point_indices, num_views)
    shared = np.zeros((num_views, num_views), dtype=np.int64)
    if cam.size:
        seen = np.zeros((num_views, int(pt.max()) + 1), dtype=np.int64)
        seen[cam, pt] = 1
        shared = seen @ seen.T
    np.fill_diagonal(shared, 0)
    out = np.full((num_views, count), -1, dtype=np.int32)
    for v in range(num_views):
        order = sorted((u for u in range(num_views) if shared[v, u] > 0), key=lambda u: (-shared[v, u], u))[:count]
        out[v, :len(order)] = order
    return out
