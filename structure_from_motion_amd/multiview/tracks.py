"""Triangulation of multi-view tracks on the GPU (``sfm_triangulate_tracks``).

Observations come in the layout of bundle adjustment: observation m is pixel ``pixels[m]`` of point ``point_indices[m]``
in camera ``camera_indices[m]``, in any order.  Poses are ``R (9) | t (3)`` rows with ``x_cam = R X + t``.  Each point is
the N-view DLT of all its observations (the reference's two-view rows, stacked), optionally refined by Levenberg-Marquardt
on its summed squared reprojection error, then checked: views, a finite estimate, cheirality, triangulation angle and the
largest reprojection error.  The first failing check gives the point's status (``device.TRACKS_*``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import numpy.typing as npt

from ..bundle.bundle import _INT32, _array, _indices
from ..pnp.pnp import check_camera_matrix


@dataclass
class TracksResult:
    points: npt.NDArray             # (P, 3); NaN for FEW_VIEWS, DEGENERATE and BAD_INDEX
    status: npt.NDArray             # (P,) uint8, device.TRACKS_*
    observation_error: npt.NDArray  # (M,) squared reprojection error in px^2 at the point's final estimate
    angle_deg: npt.NDArray          # (P,) triangulation angle in degrees: the widest-apart pair of rays is the smallest
    info: object                    # device.TracksInfo


def _non_negative_int(value, name: str, low: int = 0) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low or value >= _INT32:
        raise ValueError(f"{name} must be an integer in [{low}, 2^31), got {value!r}")
    return int(value)


def triangulate_tracks(
    camera_matrix: npt.NDArray,
    poses: npt.NDArray,
    camera_indices: Sequence[int],
    point_indices: Sequence[int],
    pixels: npt.NDArray,
    num_points: Optional[int] = None,
    min_views: int = 2,
    min_angle_deg: float = 0.0,
    max_reprojection_error: float = math.inf,
    refine_steps: int = 0,
) -> TracksResult:
    """Triangulate every point of ``range(num_points)`` from its observations.

    ``num_points`` defaults to ``max(point_indices) + 1``.  A point is OK when it has at least ``min_views`` observations,
    a finite estimate in front of every camera that sees it, a triangulation angle of at least ``min_angle_deg`` and no
    observation with a squared reprojection error above ``max_reprojection_error`` (px^2).  ``refine_steps`` > 0 refines
    each point by Levenberg-Marquardt first.  The defaults are the plain linear N-view DLT with no filtering.  An index out
    of range is not an exception: every point then has status ``device.TRACKS_BAD_INDEX`` and ``info.status`` is 1.  Every
    argument is checked before any device work."""
    K = check_camera_matrix(camera_matrix)
    poses = _array(poses, "poses", (-1, 12))
    pixels = _array(pixels, "pixels", (-1, 2))
    m = pixels.shape[0]
    cams = _indices(camera_indices, "camera_indices", m)
    pts = _indices(point_indices, "point_indices", m)
    if poses.shape[0] >= _INT32 or m >= _INT32:
        raise ValueError("cameras and observations must number fewer than 2^31")
    if num_points is None:
        num_points = int(pts.max()) + 1 if m else 0
    num_points = _non_negative_int(num_points, "num_points")
    if num_points >= _INT32 - 1:
        raise ValueError("num_points must be below 2^31 - 1")
    min_views = _non_negative_int(min_views, "min_views", low=2)
    refine_steps = _non_negative_int(refine_steps, "refine_steps")
    try:
        min_angle = float(min_angle_deg)
        max_error = float(max_reprojection_error)
    except (TypeError, ValueError):
        raise ValueError("min_angle_deg and max_reprojection_error must be numbers") from None
    if not (math.isfinite(min_angle) and min_angle >= 0.0):
        raise ValueError(f"min_angle_deg must be finite and >= 0, got {min_angle_deg!r}")
    if not max_error >= 0.0:
        raise ValueError(f"max_reprojection_error must be >= 0 (inf allowed), got {max_reprojection_error!r}")
    import torch

    from .. import device

    device.require_gpu()
    X, status, err, angle, info = device.triangulate_tracks(
        device.to_device(poses), device.to_device(cams, dtype=torch.int32), device.to_device(pts, dtype=torch.int32),
        device.to_device(pixels), num_points, K, min_views, math.radians(min_angle), max_error, refine_steps)
    return TracksResult(X.cpu().numpy(), status.cpu().numpy(), err.cpu().numpy(), np.degrees(angle.cpu().numpy()),
                        device.read_tracks_info(info))
