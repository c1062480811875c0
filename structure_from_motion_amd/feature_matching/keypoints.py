"""Multi-scale FAST keypoints with oriented BRIEF per pyramid level, for a whole image collection in one device submission
(DESIGN.md section 6x): from the images to the ``xy`` that ``verify_pairs`` and ``build_tracks`` take as features and the
descriptors that ``match_image_pairs`` takes (csrc/sfm_keypoints.hip, ``device.detect_keypoints``).

An integer image pyramid at scale 5/4 per level, FAST-9 corners with a score, 3 x 3 non-maximum suppression, a per-level quota
of the strongest corners and ``compute_brief``'s descriptor evaluated on the level each keypoint was found on.  Everything is
integer arithmetic; the definition is ``tests/keypoint_oracle.py`` and the device result is byte-identical to it.  The device
selects by a per-plane score cutoff; the host sorts the candidates and trims the ties at the cutoff.  There is no host fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np
import numpy.typing as npt

from .brief import BINS, DESCRIPTOR_BYTES, PATCH_RADIUS, BriefDescriptors, _pattern_on

MAX_LEVELS = 12                           # 1.25^l (x + 0.5) - 0.5 is exact in float64 up to here
MIN_SIDE = 48                             # a level above 0 has both sides at least this long
MAX_PLANES_PER_CALL = 65535
SLACK_PER_PLANE = 64                      # candidate slots beyond the quota: what ties at the cutoff may fill
_INT32 = 2**31


class ImageKeypoints(NamedTuple):
    xy: npt.NDArray                       # (n, 2) float64, base-image pixels: 1.25^level (level pixel + 0.5) - 0.5
    level: npt.NDArray                    # (n,) uint8
    score: npt.NDArray                    # (n,) int32 FAST score, 9 .. 4064
    descriptors: BriefDescriptors         # of the keypoint's pixel on its own level; always valid


def level_shapes(height: int, width: int, levels: int) -> List[tuple]:
    """``[(H_l, W_l)]`` of the levels an image has: level l + 1 is (4 H_l // 5, 4 W_l // 5) and exists iff l + 1 < levels and
    both sides are at least 48."""
    shapes = [(int(height), int(width))]
    while len(shapes) < levels:
        h, w = 4 * shapes[-1][0] // 5, 4 * shapes[-1][1] // 5
        if h < MIN_SIDE or w < MIN_SIDE:
            break
        shapes.append((h, w))
    return shapes


def level_quotas(num_levels: int, num_features: int) -> List[int]:
    """How many keypoints each of an image's levels keeps: ``num_features`` shared in proportion to the levels' side
    lengths (w_l = 4^l 5^(L-1-l), exact integers), the remainder to level 0."""
    weights = [4 ** l * 5 ** (num_levels - 1 - l) for l in range(num_levels)]
    total = sum(weights)
    quotas = [int(num_features) * w // total for w in weights]
    quotas[0] += int(num_features) - sum(quotas)
    return quotas


def base_coordinates(level_xy, level) -> npt.NDArray:
    """Level pixels (n, 2) on levels (n,) -> base-image pixels: bilinear sampling at scale 5/4 with pixel centres aligned."""
    scale = np.float64(1.25) ** np.asarray(level, dtype=np.float64)
    return (scale[:, None] * (np.asarray(level_xy, dtype=np.float64).reshape(-1, 2) + 0.5) - 0.5).reshape(-1, 2)


def _survivor_bound(height: int, width: int) -> int:
    """No two survivors of the suppression touch, so a plane has at most this many."""
    h, w = height - 2 * PATCH_RADIUS, width - 2 * PATCH_RADIUS
    return ((h + 1) // 2) * ((w + 1) // 2) if h > 0 and w > 0 else 0


def _checked_arguments(images: Sequence, num_features, levels, threshold):
    """Every check of ``detect_and_describe``, in ``graph_matching._checked_arguments``'s style -> (images, num_features, levels,
    threshold)."""
    if isinstance(images, np.ndarray) and images.ndim == 2:
        raise TypeError("images must be a sequence of 2-D uint8 arrays, got a single array")
    checked = []
    for i, image in enumerate(images):
        if not isinstance(image, np.ndarray):
            raise TypeError(f"images[{i}] must be a NumPy array")
        if image.dtype != np.uint8:
            raise TypeError(f"images[{i}]: detect_and_describe works on uint8 images and converts nothing, got dtype {image.dtype}")
        if image.ndim != 2 or image.shape[0] < 1 or image.shape[1] < 1:
            raise ValueError(f"images[{i}] must be a non-empty single-channel (2-D) image, got shape {image.shape}")
        checked.append(np.ascontiguousarray(image))
    for name, value, lo, hi in (("num_features", num_features, 1, _INT32 - 1), ("levels", levels, 1, MAX_LEVELS),
                                ("threshold", threshold, 1, 254)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {value!r}")
    return checked, int(num_features), int(levels), int(threshold)


class Plan(NamedTuple):
    rows: list                            # per plane (image, level, height, width, offset, quota), levels ascending
    pool_bytes: int
    capacity: int


def plan(shapes: Sequence[tuple], num_features: int, levels: int) -> Plan:
    """The plane table of a collection of images of ``shapes``: all planes of level 0 first, then level 1 of the images that
    have one, ...; the planes lie in the pool in that order.  Raises ``ValueError`` for a pool of 2^31 bytes or more."""
    per_image = [level_shapes(h, w, levels) for h, w in shapes]
    quotas = [level_quotas(len(s), num_features) for s in per_image]
    rows, offset = [], 0
    for level in range(max((len(s) for s in per_image), default=0)):
        for i, s in enumerate(per_image):
            if level < len(s):
                rows.append((i, level, s[level][0], s[level][1], offset, quotas[i][level]))
                offset += s[level][0] * s[level][1]
    if offset >= _INT32:
        raise ValueError("the pyramids of the images must hold fewer than 2^31 pixels in total")
    if len(rows) > MAX_PLANES_PER_CALL:
        raise ValueError(f"the images must have at most {MAX_PLANES_PER_CALL} pyramid levels in total")
    bounds = [_survivor_bound(h, w) for _, _, h, w, _, _ in rows]
    wanted = sum(min(q, b) for (_, _, _, _, _, q), b in zip(rows, bounds)) + SLACK_PER_PLANE * len(rows)
    capacity = max(1, min(wanted, sum(bounds)))
    if capacity >= _INT32:
        raise ValueError("num_features times the number of images must stay below 2^31")
    return Plan(rows, offset, capacity)


class _Run(NamedTuple):
    """One finished device call: what the tests read the planes and score maps from."""
    plan: Plan
    pool: object                          # device uint8 [pool_bytes]
    score: object                         # device uint16 [pool_bytes]
    kept: object
    found: int                            # candidates the device counted
    capacity: int                         # of the call that held them all
    calls: int
    candidates: npt.NDArray               # (found, 4) int32 (plane, x, y, score), device slot order
    bits: npt.NDArray
    valid: npt.NDArray
    angle_bin: npt.NDArray


def _run(images, num_features: int, levels: int, threshold: int, capacity=None) -> _Run:
    """Upload, one device call (a second one iff the candidates outnumber the capacity), one read-back."""
    import torch

    from .. import device

    layout = plan([im.shape for im in images], num_features, levels)
    dev = device.require_gpu()
    offsets, boundaries = _pattern_on(dev)
    # the level-0 planes are the head of the pool: all images go up in one buffer, the device fills the levels above
    host = np.concatenate([im.reshape(-1) for im in images])
    pool = torch.empty((layout.pool_bytes,), dtype=torch.uint8, device=dev)
    pool[:host.size].copy_(torch.as_tensor(host))
    maps = torch.empty((2, layout.pool_bytes), dtype=torch.int16, device=dev)
    table = device.keypoint_plane_table(layout.rows)
    capacity = layout.capacity if capacity is None else max(1, int(capacity))
    workspace, calls = None, 0
    while True:
        # counter | candidates | descriptors | ok | angle bin in one buffer, read back with one copy
        at_desc = 16 + 16 * capacity
        at_ok = at_desc + DESCRIPTOR_BYTES * capacity
        out = torch.empty((at_ok + 2 * capacity,), dtype=torch.uint8, device=dev)
        workspace = device.detect_keypoints(
            table, len(layout.rows), len(images), pool, threshold, offsets, boundaries, BINS, maps[0], maps[1], capacity,
            out[:4].view(torch.int32), out[16:at_desc].view(torch.int32), out[at_desc:at_ok], out[at_ok:at_ok + capacity],
            out[at_ok + capacity:], workspace)
        calls += 1
        result = out.cpu().numpy()
        found = int(result[:4].view(np.int32)[0])
        if found <= capacity:
            break
        capacity = found                                 # sizes the buffers; the second call holds every candidate
    return _Run(layout, pool, maps[0], maps[1], found, capacity, calls,
                result[16:16 + 16 * found].view(np.int32).reshape(found, 4),
                result[at_desc:at_desc + DESCRIPTOR_BYTES * found].reshape(found, DESCRIPTOR_BYTES),
                result[at_ok:at_ok + found].astype(bool), result[at_ok + capacity:at_ok + capacity + found].copy())


def _assemble(run: _Run, num_images: int) -> List[ImageKeypoints]:
    """Sort the candidates into the definition's order and trim every plane to its quota."""
    rows = np.array(run.plan.rows, dtype=np.int64).reshape(-1, 6)
    plane, x, y, score = (run.candidates[:, k].astype(np.int64) for k in range(4))
    image, level, quota = rows[plane, 0], rows[plane, 1], rows[plane, 5]
    order = np.lexsort((x, y, -score, level, image))
    # rank within the plane: sorted candidates of one plane are contiguous
    sorted_plane = plane[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(sorted_plane))[0] + 1]) if len(order) else np.zeros(0, np.int64)
    first = np.zeros(len(order), dtype=np.int64)
    first[starts] = starts
    rank = np.arange(len(order)) - np.maximum.accumulate(first)
    order = order[rank < quota[order]]
    cuts = np.searchsorted(image[order], np.arange(1, num_images), side="left")
    out = []
    for part in np.split(order, cuts):
        xy = base_coordinates(np.column_stack([x[part], y[part]]), level[part])
        out.append(ImageKeypoints(xy, level[part].astype(np.uint8), score[part].astype(np.int32),
                                  BriefDescriptors(run.bits[part], run.valid[part], run.angle_bin[part])))
    return out


def _detect(images: Sequence, num_features: int = 1000, levels: int = 8, threshold: int = 20, capacity=None):
    """``detect_and_describe`` with the candidate capacity of the first device call given -> (keypoints, ``_Run`` or None)."""
    images, num_features, levels, threshold = _checked_arguments(images, num_features, levels, threshold)
    layout = plan([im.shape for im in images], num_features, levels)   # the pool check, before any device work
    if not layout.rows:
        return [], None
    run = _run(images, num_features, levels, threshold, capacity)
    return _assemble(run, len(images)), run


def detect_and_describe(images: Sequence, *, num_features: int = 1000, levels: int = 8, threshold: int = 20) -> List[ImageKeypoints]:
    """Keypoints and descriptors of every image of a collection on the GPU (``sfm_detect_keypoints``).

    ``images`` is a sequence of 2-D ``uint8`` arrays, of any mix of sizes.  Each image gets a pyramid of at most ``levels``
    levels (1 .. 12; each 4/5 of the one below, none smaller than 48 x 48), FAST-9 corners with integer ``threshold``
    (1 .. 254) on every level, 3 x 3 non-maximum suppression, and keeps at most ``num_features`` keypoints: every level its
    share by side length, the strongest first (score descending, then y, then x).  A keypoint's descriptor is ``compute_brief``'s at its
    pixel on its own level; only pixels with a whole 31 x 31 patch around them are tested, so every descriptor is valid.
    ``levels=1`` is plain single-scale FAST.

    Returns one ``ImageKeypoints`` per image, listed by level and then by strength: ``xy`` is what ``verify_pairs`` and
    ``build_tracks`` take as features, ``descriptors`` what ``match_image_pairs`` takes.  All images go to the device in one
    buffer and all candidates come back in one read.  Every argument is checked before any device work (``TypeError`` /
    ``ValueError``; nothing is converted); an empty sequence needs no GPU."""
    return _detect(images, num_features, levels, threshold)[0]
