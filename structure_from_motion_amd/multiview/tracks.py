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


@dataclass
class RobustTracksResult:
    points: npt.NDArray             # (P, 3); NaN unless the status is TRACKS_OK or TRACKS_SMALL_ANGLE
    status: npt.NDArray             # (P,) uint8, device.TRACKS_* (never BEHIND or LARGE_ERROR; TRACKS_NO_CONSENSUS is new)
    observation_error: npt.NDArray  # (M,) squared reprojection error in px^2 at the point's final estimate, NaN without one
    inlier: npt.NDArray             # (M,) bool: the observation's error is within the limit at the final estimate
    angle_deg: npt.NDArray          # (P,) triangulation angle in degrees over the pairs of inlier observations
    info: object                    # device.RobustTracksInfo


def triangulate_tracks_robust(
    camera_matrix: npt.NDArray,
    poses: npt.NDArray,
    camera_indices: Sequence[int],
    point_indices: Sequence[int],
    pixels: npt.NDArray,
    max_reprojection_error: float,
    num_points: Optional[int] = None,
    min_views: int = 2,
    min_angle_deg: float = 0.0,
    refine_steps: int = 0,
    max_hypotheses: int = 64,
) -> RobustTracksResult:
    """``triangulate_tracks`` for tracks that hold wrong observations (``sfm_triangulate_tracks_robust``).

    Per track: two-view hypotheses from pairs of its observations (all of them, or ``max_hypotheses`` evenly spaced ones; no
    random numbers), each scored over the whole track by its inlier count at ``max_reprojection_error`` (px^2, finite) and
    its truncated error sum; the N-view DLT and the optional Levenberg-Marquardt then run over the winner's inliers only.
    ``inlier`` flags the observations within the limit at the final estimate.  A point is OK when it has at least
    ``min_views`` inliers from more than one camera and their triangulation angle is at least ``min_angle_deg``; a track
    without such a consensus is ``device.TRACKS_NO_CONSENSUS``.  An index out of range is not an exception: every point
    then has status ``device.TRACKS_BAD_INDEX`` and ``info.status`` is 1.  Every argument is checked before any device
    work."""
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
    max_hypotheses = _non_negative_int(max_hypotheses, "max_hypotheses", low=1)
    if max_hypotheses > 1024:
        raise ValueError(f"max_hypotheses must be in 1 .. 1024, got {max_hypotheses}")
    try:
        min_angle = float(min_angle_deg)
        max_error = float(max_reprojection_error)
    except (TypeError, ValueError):
        raise ValueError("min_angle_deg and max_reprojection_error must be numbers") from None
    if not (math.isfinite(min_angle) and min_angle >= 0.0):
        raise ValueError(f"min_angle_deg must be finite and >= 0, got {min_angle_deg!r}")
    if not (math.isfinite(max_error) and max_error >= 0.0):
        raise ValueError(f"max_reprojection_error must be finite and >= 0, got {max_reprojection_error!r}")
    import torch

    from .. import device

    device.require_gpu()
    (X, status, err, inlier, angle, info), _ = device.triangulate_tracks_robust(
        device.to_device(poses), device.to_device(cams, dtype=torch.int32), device.to_device(pts, dtype=torch.int32),
        device.to_device(pixels), num_points, K, max_error, min_views, math.radians(min_angle), refine_steps, max_hypotheses)
    return RobustTracksResult(X.cpu().numpy(), status.cpu().numpy(), err.cpu().numpy(), inlier.cpu().numpy().astype(bool),
                              np.degrees(angle.cpu().numpy()), device.read_robust_tracks_info(info))


@dataclass
class TrackBuildResult:
    camera_indices: npt.NDArray     # (M,) int32: the image of each observation
    point_indices: npt.NDArray      # (M,) int32: the track of each observation (tracks 0 .. info.tracks - 1)
    pixels: npt.NDArray             # (M, 2) the feature's pixel
    feature_indices: npt.NDArray    # (M,) int32: the feature's global id, image_offsets[image] + its index in the image
    image_offsets: npt.NDArray      # (I + 1,) int64: first global id of each image, then F
    track_of_feature: npt.NDArray   # (F,) int32: the feature's track, -1 unless its status is BUILD_OK
    feature_status: npt.NDArray     # (F,) uint8, device.BUILD_*
    component: npt.NDArray          # (F,) int32: the smallest global id of the feature's connected component
    info: object                    # device.TrackBuildInfo


def _feature_pixels(value, i: int) -> npt.NDArray:
    if isinstance(value, (list, tuple)) and value and not isinstance(value[0], (list, tuple, np.ndarray)):
        value = [(f.x, f.y) for f in value]   # a list of Feature
    a = np.asarray(value, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 2))
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"features[{i}] must be an (n, 2) pixel array or a list of Feature, got shape {a.shape}")
    return a


def _pair_matches(value, q: int) -> npt.NDArray:
    if isinstance(value, (list, tuple)) and value and not isinstance(value[0], (list, tuple, np.ndarray)):
        value = [(m.a_index, m.b_index) for m in value]   # a list of Match
    a = np.asarray(value)
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"matches[{q}] must be an (n, 2) index array or a list of Match, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"matches[{q}] must hold integers, got {a.dtype}")
    return a.astype(np.int64)


def build_tracks(features: Sequence, pairs, matches: Sequence) -> TrackBuildResult:
    """Multi-view tracks from the matches of image pairs (``sfm_build_tracks``).

    ``features[i]`` is image i's features: an ``(n_i, 2)`` pixel array or a list of ``Feature``; feature k of image i has
    the global id ``image_offsets[i] + k``.  ``pairs`` is ``(Q, 2)`` image indices, two different images per pair;
    ``matches[q]`` is pair q's matches: an ``(n, 2)`` array of ``(a_index, b_index)`` or the ``List[Match]`` of
    ``match_brute_force``.  Duplicate matches and duplicate or reversed pairs are allowed.  The connected components of the
    match graph are the candidate tracks; one holding two features of one image is dropped whole (``BUILD_CONFLICT``), a
    feature no match touches is ``BUILD_UNMATCHED``.  Tracks are numbered by their smallest global id, and the observations
    come by track, then by image: ready for ``triangulate_tracks`` and ``bundle_adjust``.  The result depends on the
    multiset of matches alone.  Every argument is checked before any device work (``ValueError``)."""
    feats = [_feature_pixels(f, i) for i, f in enumerate(features)]
    n = np.array([len(f) for f in feats], dtype=np.int64)
    I, F = len(feats), int(n.sum())
    if I >= _INT32 - 1 or F >= _INT32 - 1:
        raise ValueError("images and features must number fewer than 2^31 - 1")
    pair_arr = np.asarray(pairs)
    if pair_arr.size == 0:
        pair_arr = np.zeros((0, 2), dtype=np.int64)
    if pair_arr.ndim != 2 or pair_arr.shape[1] != 2:
        raise ValueError(f"pairs must have shape (Q, 2), got {pair_arr.shape}")
    if not np.issubdtype(pair_arr.dtype, np.integer):
        raise ValueError(f"pairs must hold integers, got {pair_arr.dtype}")
    Q = pair_arr.shape[0]
    if Q >= _INT32 - 1:
        raise ValueError("pairs must number fewer than 2^31 - 1")
    if len(matches) != Q:
        raise ValueError(f"matches must hold one entry per pair ({Q}), got {len(matches)}")
    if Q and (pair_arr.min() < 0 or pair_arr.max() >= I):
        raise ValueError(f"pairs must index images 0 .. {I - 1}")
    if Q and np.any(pair_arr[:, 0] == pair_arr[:, 1]):
        raise ValueError("a pair must join two different images")
    per_pair = [_pair_matches(m, q) for q, m in enumerate(matches)]
    counts = np.array([len(m) for m in per_pair], dtype=np.int64)
    E = int(counts.sum())
    if E >= _INT32:
        raise ValueError("matches must number fewer than 2^31")
    local = np.concatenate(per_pair) if Q else np.zeros((0, 2), dtype=np.int64)
    if E:
        owner = np.repeat(pair_arr.astype(np.int64), counts, axis=0)
        if local.min() < 0 or np.any(local[:, 0] >= n[owner[:, 0]]) or np.any(local[:, 1] >= n[owner[:, 1]]):
            raise ValueError("a match indexes a feature outside its image")
    import torch

    from .. import device

    dev = device.require_gpu()
    i32 = dict(dtype=torch.int32, device=dev)
    image_offset = torch.zeros(I + 1, **i32)
    image_offset[1:] = torch.cumsum(torch.as_tensor(n, device=dev), 0)
    match_offset = torch.zeros(Q + 1, **i32)
    match_offset[1:] = torch.cumsum(torch.as_tensor(counts, device=dev), 0)
    comp, track, status, cam, pt, fid, info = device.build_tracks(
        image_offset, torch.as_tensor(pair_arr, **i32), match_offset, torch.as_tensor(local, **i32), F)
    info = device.read_track_build_info(info)
    if info.status == 2:
        raise RuntimeError("build_tracks: a bounded device loop gave up (sfm_build_tracks info.status 2)")
    M = info.observations
    pix = torch.as_tensor(np.concatenate(feats) if I else np.zeros((0, 2)), dtype=torch.float64, device=dev)
    fid = fid[:M]
    return TrackBuildResult(cam[:M].cpu().numpy(), pt[:M].cpu().numpy(), pix[fid.long()].cpu().numpy(), fid.cpu().numpy(),
                            image_offset.cpu().numpy().astype(np.int64), track.cpu().numpy(), status.cpu().numpy(),
                            comp.cpu().numpy(), info)
