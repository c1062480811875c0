"""Absolute pose of every candidate view against a model in one device call: per view a P3P RANSAC pass
over its 2D-3D observations and the refinement of the winner on its inliers — what ``estimate_pose_pnp_with_ransac(...,
solver="p3p", refine_rounds=...)`` answers for one view, for all views at once (csrc/sfm_register_views.hip,
``device.RegisterViewsWorkspace``).  An incremental reconstruction registers every view that sees enough triangulated points
in one round; a set of query images is localised against a finished model in one call."""
from __future__ import annotations

import os
import random
from typing import List, NamedTuple

import numpy as np
import numpy.typing as npt

from .._native import REGISTER_STATUS as _REGISTER_STATUS   # ViewRegistrations.status names by SFM_REGISTER_* code
from ..epipolar.view_graph import _refine_arguments, chunk_bounds, pair_min_extra
from ..ransac.ransac import DEFAULT_MAX_ITERATIONS, ErrorAggregationMethod, aggregation_code
from .pnp import check_camera_matrix

P3P_SAMPLE = 4


class ViewRegistrations(NamedTuple):
    poses: npt.NDArray            # (V, 12) R row-major | t with x_cam = R X + t, NaN unless status is "ok"
    status: List[str]             # per view "ok", "no_model" (no hypothesis passed the gate) or "too_few" (fewer than 4 items)
    inlier_count: npt.NDArray     # (V,) observations within the threshold under the pose (the refinement's count)
    inliers: List[npt.NDArray]    # per view the indices into the caller's M arrays of those observations, ascending
    ransac_count: npt.NDArray     # (V,) the RANSAC winner's sample size plus its extra inliers, 0 without a winner
    error: npt.NDArray            # (V,) RMS squared reprojection error of the pose over its inliers, inf without a pose
    accepted: npt.NDArray         # (V,) refinement rounds whose result was kept (0: the pose is the RANSAC winner)
    lm_steps: npt.NDArray         # (V,) Levenberg-Marquardt trial steps over all rounds


def _checked_observations(points_3d, view_indices, point_indices, pixels, num_views):
    """The checks of the observation arrays -> (points (P, 3), views (M,), points' indices (M,), pixels (M, 2), V)."""
    points = np.asarray(points_3d, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points_3d must have shape (P, 3), got {points.shape}")
    views, index = np.asarray(view_indices), np.asarray(point_indices)
    for name, a in (("view_indices", views), ("point_indices", index)):
        if a.ndim != 1:
            raise ValueError(f"{name} must have shape (M,), got {a.shape}")
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must hold integers, got {a.dtype}")
    M = len(views)
    pix = np.asarray(pixels, dtype=np.float64).reshape(-1, 2) if np.size(pixels) == 0 else np.asarray(pixels, dtype=np.float64)
    if len(index) != M or pix.shape != (M, 2):
        raise ValueError(f"view_indices, point_indices and pixels must be (M,), (M,) and (M, 2), got {views.shape}, {index.shape}, "
                         f"{pix.shape}")
    if M >= 2**31:
        raise ValueError("observations must number fewer than 2^31")
    views, index = views.astype(np.int64), index.astype(np.int64)
    if num_views is None:
        V = int(views.max()) + 1 if M else 0
    else:
        if isinstance(num_views, bool) or not isinstance(num_views, (int, np.integer)) or num_views < 0:
            raise ValueError(f"num_views must be a non-negative integer, got {num_views!r}")
        V = int(num_views)
    if M and (views.min() < 0 or views.max() >= V):
        raise ValueError(f"view_indices must index views 0 .. {V - 1}")
    if M and (index.min() < 0 or index.max() >= len(points)):
        raise ValueError(f"point_indices must index points 0 .. {len(points) - 1}")
    return points, views, index, pix, V


def ragged_order(view_indices, num_views: int):
    """(order, offset): the stable sort of the observations by view and the (V + 1,) offsets of the views in that order —
    position k of the ragged layout is observation ``order[k]`` of the caller."""
    views = np.asarray(view_indices, dtype=np.int64)
    order = np.argsort(views, kind="stable")
    offset = np.zeros(num_views + 1, dtype=np.int64)
    offset[1:] = np.cumsum(np.bincount(views, minlength=num_views)[:num_views])
    return order, offset


def register_views(camera_matrix, points_3d, view_indices, point_indices, pixels, reprojection_threshold: float,
                   num_views: int | None = None, min_num_extra_inliers=10, min_extra_fraction: float = 0.0,
                   max_iterations: int | None = None, refine_rounds: int = 2, refine_max_steps: int = 20,
                   seed: int | None = None, max_hypotheses_per_call: int = 2**21) -> ViewRegistrations:
    """Register all V views against ``points_3d`` in one device call per chunk: observation m is pixel ``pixels[m]`` of
    ``points_3d[point_indices[m]]`` in view ``view_indices[m]`` — the layout ``build_tracks`` returns and ``bundle_adjust``
    takes.  ``num_views`` defaults to the largest view index plus one.

    Per view, ``max_iterations`` Philox samples of four observations serve a P3P pass: an observation is an inlier when its
    squared reprojection error is at most ``reprojection_threshold`` (pixel units, as ``estimate_pose_pnp_with_ransac``
    takes it), the aggregation is RMS and the gate is ``max(min_num_extra_inliers, floor(min_extra_fraction * n_v))``
    (``min_num_extra_inliers``: an int or one per view).  The winner is then refined on its inliers: up to ``refine_rounds``
    rounds of at most ``refine_max_steps`` Levenberg-Marquardt steps, a round kept when it has more inliers, or as many and a
    lower error; the winner's fourth sample item does not seed the refinement.  Only P3P is supported.

    View v draws its samples with ``seed + v`` (``seed``, else ``SFM_SEED``, else 64 bits of ``random``), so the result does
    not depend on how the views are split into device calls (``max_hypotheses_per_call`` view-hypotheses each).  The
    observations are sorted stably by view on the host, uploaded once and gathered on the device.  Every argument is checked
    before any device work (``ValueError``)."""
    K = check_camera_matrix(camera_matrix)
    threshold = float(reprojection_threshold)
    if not (np.isfinite(threshold) and threshold > 0.0):
        raise ValueError(f"reprojection_threshold must be finite and positive, got {reprojection_threshold!r}")
    rounds, steps = _refine_arguments(refine_rounds, refine_max_steps)
    points, views, index, pix, V = _checked_observations(points_3d, view_indices, point_indices, pixels, num_views)
    if max_iterations is None:
        iterations = DEFAULT_MAX_ITERATIONS
    elif isinstance(max_iterations, bool) or not isinstance(max_iterations, (int, np.integer)) or max_iterations < 1:
        raise ValueError(f"max_iterations must be an integer >= 1, got {max_iterations!r}")
    else:
        iterations = int(max_iterations)
    order, offset = ragged_order(views, V)
    counts = np.diff(offset)
    gate = pair_min_extra(counts, min_num_extra_inliers, min_extra_fraction)
    chunks = chunk_bounds(V, iterations, max_hypotheses_per_call)
    if seed is None:
        seed = int(os.environ["SFM_SEED"]) if "SFM_SEED" in os.environ else random.getrandbits(64)
    elif isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    seed = int(seed)
    if V == 0:
        return ViewRegistrations(np.zeros((0, 12)), [], np.zeros(0, np.int64), [], np.zeros(0, np.int64), np.zeros(0),
                                 np.zeros(0, np.int64), np.zeros(0, np.int64))
    import torch

    from .. import device

    dev = device.require_gpu()
    # one upload of each array; the [N, 5] items of the ragged layout are gathered on the device
    points_dev, pix_dev = device.to_device(points), device.to_device(pix)
    order_dev, index_dev = device.to_device(order, torch.int64), device.to_device(index, torch.int64)
    if len(order):
        pts = torch.cat([points_dev[index_dev[order_dev]], pix_dev[order_dev]], dim=1).contiguous()
    else:
        pts = torch.empty((0, 5), dtype=torch.float64, device=dev)
    offset_dev = device.to_device(offset, torch.int64)
    gate_dev = device.to_device(gate.astype(np.float64))
    aggregation = aggregation_code(ErrorAggregationMethod.RMS)
    parts = []
    for v0, v1 in chunks:
        lo, hi = int(offset[v0]), int(offset[v1])
        ws = device.RegisterViewsWorkspace(v1 - v0, hi - lo, iterations, dev)
        ws.run(pts[lo:hi], offset_dev[v0:v1 + 1] - lo, gate_dev[v0:v1], K, threshold, aggregation, seed + v0, seed_stride=1,
               refine_rounds=rounds, refine_max_steps=steps)
        parts.append(ws)
    code = np.concatenate([device.read_register_status(ws.status) for ws in parts])
    if np.any(code == device.REGISTER_BAD_OFFSETS):
        raise RuntimeError("register_views: the device refused the offset table (SFM_REGISTER_BAD_OFFSETS)")
    poses = np.concatenate([ws.pose_out.cpu().numpy() for ws in parts])
    mask_out = np.concatenate([ws.mask_out.cpu().numpy() for ws in parts])
    info = [r for ws in parts for r in device.read_pnp_refine_info(ws.info)]
    records = np.concatenate([ws.result.cpu().numpy() for ws in parts])   # int64 [V, 5]: key, best_h, best_err, first_flagged, counts
    best_h = records[:, 1]
    best_cnt = (records[:, 4] >> 32).astype(np.int64)
    ransac_count = np.where(best_h >= 0, P3P_SAMPLE + best_cnt, 0).astype(np.int64)
    poses[code != device.REGISTER_OK] = np.nan
    inliers = [np.sort(order[offset[v]:offset[v + 1]][mask_out[offset[v]:offset[v + 1]] != 0]) for v in range(V)]
    return ViewRegistrations(poses, [_REGISTER_STATUS[c] for c in code], np.array([r.count for r in info], dtype=np.int64), inliers,
                             ransac_count, np.array([r.error for r in info], dtype=np.float64),
                             np.array([r.accepted for r in info], dtype=np.int64), np.array([r.lm_steps for r in info], dtype=np.int64))
