"""Sub-pixel refinement of track observations by affine least-squares patch matching (DESIGN.md section 6al,
csrc/sfm_track_refine.hip, ``device.refine_observations``).

A keypoint of ``detect_and_describe`` is an integer pixel of the pyramid level it was found on.  Every observation of a track but
the track's reference is aligned here with the reference's window on the two observations' own pyramid planes, so that all
observations of a track look at one surface point; the reference keeps its integer pixel.  The definition is
``tests/track_refine_oracle.py`` and the device result is byte-identical to it.  There is no host fallback.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np
import numpy.typing as npt

from ..feature_matching import keypoints as kp
from ..feature_matching.brief import BINS

MIN_RADIUS, MAX_RADIUS, MAX_ITERATIONS = 2, 7, 50
STATUS_NAMES = ("ok", "reference", "bad_index", "outside", "flat", "singular", "diverged", "low_correlation")
_INT32 = 2**31


class TrackRefinement(NamedTuple):
    pixels: npt.NDArray        # (M, 2) float64 base-image pixels: what triangulate_tracks and bundle_adjust take
    level_xy: npt.NDArray      # (M, 2) float64 pixels of the observation's own pyramid level
    status: npt.NDArray        # (M,) int32, device.REFINE_*; every status but REFINE_OK keeps the integer input position
    correlation: npt.NDArray   # (M,) float64 normalised correlation at the final state, NaN where none was sampled
    iterations: npt.NDArray    # (M,) int32 Gauss-Newton solves done
    warp: npt.NDArray          # (M, 4) float64 (A00, A01, A10, A11): reference window offsets -> offsets on the observation's plane
    reference: npt.NDArray     # (M,) int32 the observation each one was aligned with; -1 for a reference


def level_pixels(xy, level) -> npt.NDArray:
    """Base-image pixels (n, 2) of keypoints found on ``level`` (n,) -> their integer level pixels (n, 2) int64: the rounded
    inverse of ``keypoints.base_coordinates``.  ``ValueError`` unless it reproduces ``xy`` exactly."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    level = np.asarray(level).reshape(-1)
    if len(level) != len(xy):
        raise ValueError(f"xy and level must have one entry per keypoint, got {len(xy)} and {len(level)}")
    if len(level) and (level.min() < 0 or level.max() >= kp.MAX_LEVELS):
        raise ValueError(f"levels must be in 0 .. {kp.MAX_LEVELS - 1}")
    if not np.all(np.isfinite(xy)):
        raise ValueError("keypoint positions must be finite")
    scale = np.float64(1.25) ** level.astype(np.float64)
    rounded = np.rint((xy + 0.5) / scale[:, None] - 0.5)
    if len(xy) and np.abs(rounded).max() >= _INT32:
        raise ValueError("keypoint positions must stay below 2^31 level pixels")
    if not np.array_equal(kp.base_coordinates(rounded, level), xy):
        raise ValueError("xy is not the position of an integer pixel of its level (1.25^level (pixel + 0.5) - 0.5)")
    return rounded.astype(np.int64)


def track_references(point_indices) -> npt.NDArray:
    """(M,) int32: per observation the lowest observation index of its track, -1 for that observation itself."""
    point_indices = np.asarray(point_indices, dtype=np.int64).reshape(-1)
    M = len(point_indices)
    if M == 0:
        return np.zeros(0, dtype=np.int32)
    first = np.full(int(point_indices.max()) + 1, M, dtype=np.int64)
    np.minimum.at(first, point_indices, np.arange(M))
    reference = first[point_indices]
    reference[reference == np.arange(M)] = -1
    return reference.astype(np.int32)


def bin_rotation(bin_reference, bin_observation) -> npt.NDArray:
    """(M, 4) float64: the rotation by the angle between the centres of two orientation bins of section 6o (bin b is centred on
    2 pi b / 30, measured from +x towards +y), which turns the reference's window offsets into the observation's."""
    angle = (np.asarray(bin_observation, dtype=np.float64) - np.asarray(bin_reference, dtype=np.float64)) * (2.0 * np.pi / BINS)
    c, s = np.cos(angle), np.sin(angle)
    return np.column_stack([c, -s, s, c]).reshape(-1, 4)


def _checked_options(radius, max_iterations, min_step, max_shift, min_correlation, levels):
    for name, value, lo, hi in (("radius", radius, MIN_RADIUS, MAX_RADIUS), ("max_iterations", max_iterations, 1, MAX_ITERATIONS),
                                ("levels", levels, 1, kp.MAX_LEVELS)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {value!r}")
    for name, value in (("min_step", min_step), ("max_shift", max_shift)):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value) \
                or not value > 0:
            raise ValueError(f"{name} must be a positive finite number, got {value!r}")
    if isinstance(min_correlation, bool) or not isinstance(min_correlation, (int, float, np.integer, np.floating)) \
            or np.isnan(min_correlation):
        raise ValueError(f"min_correlation must be a number, got {min_correlation!r}")
    return int(radius), int(max_iterations), float(min_step), float(max_shift), float(min_correlation), int(levels)


def _checked_images(images):
    if isinstance(images, np.ndarray) and images.ndim == 2:
        raise TypeError("images must be a sequence of 2-D uint8 arrays, got a single array")
    checked = []
    for i, image in enumerate(images):
        if not isinstance(image, np.ndarray):
            raise TypeError(f"images[{i}] must be a NumPy array")
        if image.dtype != np.uint8:
            raise TypeError(f"images[{i}]: the refinement works on uint8 images and converts nothing, got dtype {image.dtype}")
        if image.ndim != 2 or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"images[{i}] must be a non-empty single-channel (2-D) image, got shape {image.shape}")
        checked.append(np.ascontiguousarray(image))
    return checked


def _int_array(value, name, M=None):
    a = np.asarray(value)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must hold integers, got {a.dtype}")
    a = a.reshape(-1).astype(np.int64)
    if M is not None and len(a) != M:
        raise ValueError(f"{name} must have one entry per observation ({M}), got {len(a)}")
    if len(a) and (a.min() < -_INT32 or a.max() >= _INT32):
        raise ValueError(f"{name} must fit 32 bits")
    return a


def refine_observations(images: Sequence, image_indices, level, level_xy, reference, warp0, *, radius: int = 7,
                        max_iterations: int = 10, min_step: float = 1e-3, max_shift: float = 3.0, min_correlation: float = 0.8,
                        levels: int = 8) -> TrackRefinement:
    """``refine_track_observations`` on plain arrays: observation o is the integer pixel ``level_xy[o]`` of level ``level[o]`` of
    image ``image_indices[o]``, aligned with observation ``reference[o]`` (itself or -1: a reference) from the warp
    ``warp0[o]`` = (A00, A01, A10, A11) — a caller who knows the poses can start from a better warp than the bins give.  A
    reference outside the list or a pixel outside its plane is the status ``REFINE_BAD_INDEX``, not an error; an image index
    or a level that the collection does not have is a ``ValueError``, like every other argument error, before any device work."""
    images = _checked_images(images)
    radius, max_iterations, min_step, max_shift, min_correlation, levels = _checked_options(
        radius, max_iterations, min_step, max_shift, min_correlation, levels)
    image_indices = _int_array(image_indices, "image_indices")
    M = len(image_indices)
    level, reference = _int_array(level, "level", M), _int_array(reference, "reference", M)
    xy_in = np.asarray(level_xy)
    if xy_in.size and not np.issubdtype(xy_in.dtype, np.integer):
        raise TypeError(f"level_xy must hold integer level pixels, got {xy_in.dtype}")
    if xy_in.size != 2 * M:
        raise ValueError(f"level_xy must have shape ({M}, 2), got {xy_in.shape}")
    xy_in = _int_array(xy_in, "level_xy").reshape(M, 2)
    warp0 = np.ascontiguousarray(np.asarray(warp0, dtype=np.float64).reshape(-1))
    if warp0.size != 4 * M:
        raise ValueError(f"warp0 must have shape ({M}, 4), got {warp0.size} values")
    warp0 = warp0.reshape(M, 4)
    layout = kp.plan([im.shape for im in images], 1, levels)   # the pool check, before any device work
    plane_of = {(row[0], row[1]): p for p, row in enumerate(layout.rows)}
    if M and (image_indices.min() < 0 or image_indices.max() >= len(images)):
        raise ValueError(f"image_indices must index images 0 .. {len(images) - 1}")
    try:
        plane = np.array([plane_of[(int(i), int(l))] for i, l in zip(image_indices, level)], dtype=np.int32)
    except KeyError as missing:
        raise ValueError(f"image {missing.args[0][0]} has no pyramid level {missing.args[0][1]} with levels={levels}") from None
    if M == 0:
        return TrackRefinement(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32),
                               np.zeros((0, 4)), np.zeros(0, np.int32))
    import torch

    from .. import device

    dev = device.require_gpu()
    host = np.concatenate([im.reshape(-1) for im in images])
    pool = torch.empty((layout.pool_bytes,), dtype=torch.uint8, device=dev)
    pool[:host.size].copy_(torch.as_tensor(host))
    table = device.keypoint_plane_table(layout.rows)
    workspace = device.build_pyramid(table, len(layout.rows), len(images), pool)
    ints = torch.as_tensor(np.stack([plane, xy_in[:, 0].astype(np.int32), xy_in[:, 1].astype(np.int32),
                                     reference.astype(np.int32)]), device=dev)
    start = torch.as_tensor(warp0, device=dev)
    out = torch.empty((7, M), dtype=torch.float64, device=dev)   # xy | warp | correlation, read back with one copy
    counts = torch.empty((2, M), dtype=torch.int32, device=dev)   # iterations | status
    device.refine_observations(table, len(layout.rows), len(images), pool, ints[0], ints[1], ints[2], ints[3], start, radius,
                               max_iterations, min_step, max_shift, min_correlation, out[:2].view(-1).view(M, 2),
                               out[2:6].view(-1).view(M, 4), out[6], counts[0], counts[1], workspace)
    result, tallies = out.cpu().numpy(), counts.cpu().numpy()
    refined = result[:2].reshape(-1).reshape(M, 2).copy()
    own = reference.copy()
    own[own == np.arange(M)] = -1
    return TrackRefinement(kp.base_coordinates(refined, level), refined, tallies[1].copy(), result[6].copy(), tallies[0].copy(),
                           result[2:6].reshape(-1).reshape(M, 4).copy(), own.astype(np.int32))


def track_observations(keypoints: Sequence, build):
    """(image, level, integer level pixel, reference, warp0) of the observations of ``build`` (a ``TrackBuildResult``) among
    ``keypoints`` (the ``ImageKeypoints`` list the tracks were built from); every check of the two against each other."""
    image = _int_array(build.camera_indices, "build.camera_indices")
    M = len(image)
    feature, track = _int_array(build.feature_indices, "build.feature_indices", M), _int_array(build.point_indices, "build.point_indices", M)
    offsets = np.asarray(build.image_offsets, dtype=np.int64).reshape(-1)
    counts = np.array([len(k.level) for k in keypoints], dtype=np.int64)
    if len(offsets) != len(counts) + 1 or not np.array_equal(np.diff(offsets), counts) or (len(offsets) and offsets[0] != 0):
        raise ValueError("build.image_offsets does not fit the keypoint lists: the tracks were built from other features")
    if M and (image.min() < 0 or image.max() >= len(counts)):
        raise ValueError(f"build.camera_indices must index images 0 .. {len(counts) - 1}")
    local = feature - offsets[image]
    if M and (local.min() < 0 or np.any(local >= counts[image])):
        raise ValueError("build.feature_indices names a feature outside its image")
    if M and track.min() < 0:
        raise ValueError("build.point_indices must not be negative")
    level, bins, xy = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64), np.zeros((M, 2))
    for i, k in enumerate(keypoints):
        mine = image == i
        level[mine], bins[mine] = np.asarray(k.level)[local[mine]], np.asarray(k.descriptors.angle_bin)[local[mine]]
        xy[mine] = np.asarray(k.xy, dtype=np.float64).reshape(-1, 2)[local[mine]]
    reference = track_references(track)
    ref_index = np.where(reference >= 0, reference, np.arange(M))
    return image, level, level_pixels(xy, level), reference, bin_rotation(bins[ref_index], bins)


def refine_track_observations(images: Sequence, keypoints: Sequence, build, *, radius: int = 7, max_iterations: int = 10,
                              min_step: float = 1e-3, max_shift: float = 3.0, min_correlation: float = 0.8,
                              levels: int = 8) -> TrackRefinement:
    """Refines the observations of the tracks of a collection to sub-pixel positions on the GPU (``sfm_refine_observations``).

    ``images`` are the uint8 images, ``keypoints`` the ``ImageKeypoints`` list ``detect_and_describe`` made of them (with the same
    ``levels``) and ``build`` the ``TrackBuildResult`` ``build_tracks`` made of their ``xy``.  A track's reference is its
    observation with the lowest index; every other observation is aligned with the reference's (2 ``radius`` + 1)^2 window by at
    most ``max_iterations`` Gauss-Newton steps on six affine parameters, starting from the rotation between the two keypoints'
    orientation bins (the pyramid levels carry the scale).  An observation keeps its integer pixel unless the fit stays within
    ``max_shift`` level pixels, inside its plane, and ends with a normalised correlation of at least ``min_correlation``.

    Returns a ``TrackRefinement``; its ``pixels`` go in place of ``build.pixels`` into ``triangulate_tracks`` and
    ``bundle_adjust``.  Every argument is checked before any device work (``TypeError`` / ``ValueError``); a collection without
    tracks needs no GPU."""
    checked = _checked_images(images)
    if len(keypoints) != len(checked):
        raise ValueError(f"keypoints must hold one entry per image ({len(checked)}), got {len(keypoints)}")
    _checked_options(radius, max_iterations, min_step, max_shift, min_correlation, levels)
    image, level, pixel, reference, warp0 = track_observations(keypoints, build)
    return refine_observations(checked, image, level, pixel, reference, warp0, radius=radius, max_iterations=max_iterations,
                               min_step=min_step, max_shift=max_shift, min_correlation=min_correlation, levels=levels)
