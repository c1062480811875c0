"""Guided descriptor matching over a verified view graph: ``match_image_pairs``'s nearest-neighbour
search and validation repeated with each pair restricted to the partners its two-view model admits — the features within the
inlier threshold of the epipolar line for an ``"essential"`` pair, or of the transferred point for a ``"homography"`` pair
(csrc/sfm_match_pairs.hip, ``device.match_pairs_guided``).

On repeated structure Lowe's ratio and the mutual check reject exactly the features whose runner-up looks alike; with the
look-alikes that lie off the epipolar line out of the contest, those features come back.  The definition is
``tests/guided_matching_oracle.py``; the device result is bit-identical to it.  There is no host fallback.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import numpy.typing as npt

from .brief import DESCRIPTOR_BYTES
from .graph_matching import MAX_PAIRS_PER_CALL, PairMatches, _checked_arguments, call_bounds

KIND_CODES = {"none": 0, "essential": 1, "homography": 2}   # the view graph's codes (sfm_pair_verdict.kind)


def _kind_codes(kinds, Q: int) -> npt.NDArray:
    """The graph's strings or the codes -> int32 (Q,) of 0 / 1 / 2."""
    if isinstance(kinds, (str, bytes)):
        raise TypeError(f"kinds must hold one kind per pair, got {kinds!r}")
    values = list(kinds)
    if len(values) != Q:
        raise ValueError(f"kinds must hold one entry per pair ({Q}), got {len(values)}")
    codes = np.zeros(Q, dtype=np.int32)
    for q, k in enumerate(values):
        if isinstance(k, str):
            if k not in KIND_CODES:
                raise ValueError(f"kinds[{q}] must be 'none', 'essential' or 'homography', got {k!r}")
            codes[q] = KIND_CODES[k]
        elif isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"kinds[{q}] must be a kind name or an integer code, got {k!r}")
        elif not 0 <= k <= 2:
            raise ValueError(f"kinds[{q}] must be 0 (none), 1 (essential) or 2 (homography), got {k!r}")
        else:
            codes[q] = int(k)
    return codes


def _checked_guided_arguments(descriptors, features, camera_matrix, pairs, models, kinds, thresholds, max_distance, ratio,
                              cross_check, max_pairs_per_call):
    """Every check of ``guided_match_models``: ``graph_matching._checked_arguments`` plus the guide's arguments ->
    (its tuple, pixels per image, K, models (Q, 9), kind codes (Q,), thresholds (Q,))."""
    from ..epipolar.homography import check_camera_matrix   # here: epipolar imports this package at its top
    from ..multiview.tracks import _feature_pixels

    checked = _checked_arguments(descriptors, pairs, max_distance, ratio, cross_check, max_pairs_per_call)
    images, pair_arr = checked[0], checked[1]
    Q = len(pair_arr)
    K = check_camera_matrix(camera_matrix)
    if len(features) != len(images):
        raise ValueError(f"features must hold one entry per image ({len(images)}), got {len(features)}")
    pixels = [_feature_pixels(f, i) for i, f in enumerate(features)]
    for i, (p, (_, valid)) in enumerate(zip(pixels, images)):
        if len(p) != len(valid):
            raise ValueError(f"features[{i}] and descriptors[{i}] must have equal length, got {len(p)} and {len(valid)}")
    model_arr = np.asarray(models, dtype=np.float64)
    if model_arr.size == 0 and Q == 0:
        model_arr = np.zeros((0, 3, 3))
    if model_arr.shape != (Q, 3, 3):
        raise ValueError(f"models must have shape ({Q}, 3, 3), got {model_arr.shape}")
    codes = _kind_codes(kinds, Q)
    thr = np.asarray(thresholds)
    if thr.dtype == np.bool_ or not (np.issubdtype(thr.dtype, np.floating) or np.issubdtype(thr.dtype, np.integer)):
        raise TypeError(f"thresholds must be a number or one number per pair, got {thr.dtype}")
    thr = thr.astype(np.float64)
    if thr.ndim == 0:
        thr = np.full(Q, thr)
    if thr.shape != (Q,):
        raise ValueError(f"thresholds must be a number or one number per pair ({Q}), got shape {thr.shape}")
    return checked, pixels, K, np.ascontiguousarray(model_arr.reshape(Q, 9)), codes, np.ascontiguousarray(thr)


def normalized_coordinates(K, pixels) -> npt.NDArray:
    """(n, 2) pixels -> K-normalised ``((u - cx) / fx, (v - cy) / fy)``: the arithmetic of ``normalize_kernel``, which reads
    fx, fy, cx and cy only."""
    out = np.empty((len(pixels), 2), dtype=np.float64)
    out[:, 0] = (pixels[:, 0] - K[0, 2]) / K[0, 0]
    out[:, 1] = (pixels[:, 1] - K[1, 2]) / K[1, 1]
    return out


def guided_match_models(descriptors: Sequence, features: Sequence, camera_matrix, pairs, models, kinds, thresholds, *,
                        max_distance: int = 64, ratio=0.8, cross_check: bool = True,
                        max_pairs_per_call: int = MAX_PAIRS_PER_CALL) -> PairMatches:
    """``match_image_pairs`` with every pair restricted to what its two-view model admits (``sfm_match_pairs_guided``).

    ``descriptors`` and ``pairs`` are ``match_image_pairs``'s; ``features[i]`` holds image i's pixels as ``verify_pairs`` takes
    them (an (n, 2) array or a list of ``Feature``), one per descriptor; ``models`` is ``(Q, 3, 3)``, ``kinds`` the view
    graph's strings (``"essential"``, ``"homography"``, ``"none"``) or their codes 1, 2, 0 and ``thresholds`` a number or one
    per pair, in the K-normalised units of ``verify_pairs``'s ``inlier_threshold``.  For pair (i, j), feature a of image i and
    feature b of image j are admissible iff both are valid and the symmetric epipolar distance (essential) or the symmetric
    transfer error (homography) of (a, b) under the pair's model is at most its threshold; a ``"none"`` pair, a NaN model and a
    NaN threshold admit nothing.  Nearest column, runner-up, ``max_distance``, ``ratio`` and ``cross_check`` then mean what
    they mean in ``match_image_pairs``, over the admissible partners only.  With ``cross_check`` no feature appears twice in a
    list.

    Descriptors, flags, coordinates (normalised once per image on the host), models and all index tables go up in one buffer
    and all rows come back in one read; the host only compacts.  Splitting into calls of ``max_pairs_per_call`` pairs changes
    no byte.  Every argument is checked before any device work (``ValueError`` / ``TypeError``); no pairs, or no features in
    any first image, need no GPU."""
    checked, pixels, K, model_arr, codes, thr = _checked_guided_arguments(
        descriptors, features, camera_matrix, pairs, models, kinds, thresholds, max_distance, ratio, cross_check,
        max_pairs_per_call)
    images, pair_arr, max_distance, ratio, cross_check, per_call = checked
    Q = len(pair_arr)
    sizes = np.array([len(v) for _, v in images], dtype=np.int64)
    row_offset = np.zeros(Q + 1, dtype=np.int64)
    row_offset[1:] = np.cumsum(sizes[pair_arr[:, 0]])
    rows = int(row_offset[-1])
    if rows == 0:
        return PairMatches(pair_arr, [np.zeros((0, 2), np.int64) for _ in range(Q)], [np.zeros(0, np.int32) for _ in range(Q)])
    import torch

    from .. import device

    dev = device.require_gpu()
    I, F = len(images), int(sizes.sum())
    chunks = call_bounds(sizes, pair_arr, per_call)
    # one upload: descriptors | flags | coordinates, models, thresholds (float64) | per call its row offsets from 0 (int64) |
    # image offsets, pair images, kinds (int32)
    call_rows = [row_offset[q0:q1 + 1] - row_offset[q0] for q0, q1 in chunks]
    image_offset = np.zeros(I + 1, dtype=np.int32)
    image_offset[1:] = np.cumsum(sizes)
    at_ok = F * DESCRIPTOR_BYTES
    at_xy = (at_ok + F + 7) // 8 * 8
    at_model = at_xy + 16 * F
    at_thr = at_model + 72 * Q
    at_rows = at_thr + 8 * Q
    at_images = at_rows + 8 * sum(len(r) for r in call_rows)
    at_pairs = at_images + 4 * (I + 1)
    at_kind = at_pairs + 8 * Q
    host = np.zeros(at_kind + 4 * Q, dtype=np.uint8)
    host[:at_ok] = np.concatenate([b for b, _ in images]).reshape(-1)
    host[at_ok:at_ok + F] = np.concatenate([v for _, v in images])
    host[at_xy:at_model] = np.concatenate([normalized_coordinates(K, p) for p in pixels]).reshape(-1).view(np.uint8)
    host[at_model:at_thr] = model_arr.reshape(-1).view(np.uint8)
    host[at_thr:at_rows] = thr.view(np.uint8)
    host[at_rows:at_images] = np.concatenate(call_rows).view(np.uint8)
    host[at_images:at_pairs] = image_offset.view(np.uint8)
    host[at_pairs:at_kind] = np.ascontiguousarray(pair_arr, dtype=np.int32).reshape(-1).view(np.uint8)
    host[at_kind:] = codes.view(np.uint8)
    buf = torch.as_tensor(host).to(dev)
    desc, ok = buf[:at_ok], buf[at_ok:at_ok + F]
    xy = buf[at_xy:at_model].view(torch.float64).view(F, 2)
    model_dev = buf[at_model:at_thr].view(torch.float64).view(Q, 9)
    thr_dev = buf[at_thr:at_rows].view(torch.float64)
    rows_dev = buf[at_rows:at_images].view(torch.int64)
    image_offset_dev = buf[at_images:at_pairs].view(torch.int32)
    pair_images_dev = buf[at_pairs:at_kind].view(torch.int32).view(Q, 2)
    kind_dev = buf[at_kind:].view(torch.int32)
    out = torch.empty((2 * rows + Q,), dtype=torch.int32, device=dev)   # partner | distance | pair status: one read
    partner, distance, status = out[:rows], out[rows:2 * rows], out[2 * rows:]
    workspace, at = None, 0
    for (q0, q1), r in zip(chunks, call_rows):
        lo, hi = int(row_offset[q0]), int(row_offset[q1])
        largest = int(sizes[pair_arr[q0:q1]].max())
        workspace = device.match_pairs_guided(I, F, image_offset_dev, desc, ok, xy, pair_images_dev[q0:q1],
                                              rows_dev[at:at + len(r)], model_dev[q0:q1], kind_dev[q0:q1], thr_dev[q0:q1],
                                              hi - lo, largest, max_distance, ratio, cross_check, partner[lo:hi],
                                              distance[lo:hi], status[q0:q1], workspace)
        at += len(r)
    result = out.cpu().numpy()
    if np.any(result[2 * rows:] != 0):
        raise RuntimeError("guided_match_models: the device refused a pair the host had checked (sfm_match_pairs_guided "
                           "pair_status)")
    partner_host, distance_host = result[:rows], result[rows:2 * rows]
    kept = np.nonzero(partner_host >= 0)[0]
    owner = np.searchsorted(row_offset, kept, side="right") - 1
    table = np.column_stack([kept - row_offset[owner], partner_host[kept].astype(np.int64)]).astype(np.int64).reshape(-1, 2)
    cuts = np.searchsorted(kept, row_offset[1:-1], side="left")
    return PairMatches(pair_arr, np.split(table, cuts), np.split(distance_host[kept], cuts))


def essential_from_pose(R, t) -> npt.NDArray:
    """``E = [t]x R`` of (Q, 3, 3) rotations and (Q, 3) translations, each entry two products and one subtraction (DESIGN.md
    section 6ac, ``essential_of`` of csrc/sfm_view_graph_refine.hip)."""
    R, t = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3), np.asarray(t, dtype=np.float64).reshape(-1, 3)
    E = np.empty_like(R)
    with np.errstate(invalid="ignore"):
        for j in range(3):
            E[:, 0, j] = t[:, 1] * R[:, 2, j] - t[:, 2] * R[:, 1, j]
            E[:, 1, j] = t[:, 2] * R[:, 0, j] - t[:, 0] * R[:, 2, j]
            E[:, 2, j] = t[:, 0] * R[:, 1, j] - t[:, 1] * R[:, 0, j]
    return E


def graph_models(graph, use_pose: bool = False):
    """(models (Q, 3, 3), kinds) of a ``ViewGraph`` (duck-typed: ``pairs``, ``kind``, ``E``, ``H`` and, with ``use_pose``,
    ``pose.R`` / ``.t`` / ``.status``): E of an ``"essential"`` pair, H of a ``"homography"`` pair, NaN for ``"none"``.  With
    ``use_pose`` an essential pair whose pose status is ``"ok"`` takes ``E = [t]x R`` of its pose."""
    if not isinstance(use_pose, (bool, np.bool_)):
        raise TypeError(f"use_pose must be a bool, got {use_pose!r}")
    for name in ("pairs", "kind", "E", "H"):
        if not hasattr(graph, name):
            raise TypeError(f"graph must be a ViewGraph (pairs, kind, E, H), it has no {name!r}")
    kinds = list(graph.kind)
    Q = len(kinds)
    E, H = np.asarray(graph.E, dtype=np.float64), np.asarray(graph.H, dtype=np.float64)
    if E.size == 0 and H.size == 0 and Q == 0:
        return np.zeros((0, 3, 3)), kinds
    if E.shape != (Q, 3, 3) or H.shape != (Q, 3, 3):
        raise ValueError(f"graph.E and graph.H must have shape ({Q}, 3, 3), got {E.shape} and {H.shape}")
    if use_pose:
        pose = getattr(graph, "pose", None)
        if pose is None:
            raise ValueError("use_pose needs a graph with poses (verify_pairs(relative_pose=True))")
        from_pose = essential_from_pose(pose.R, pose.t)
        if from_pose.shape != (Q, 3, 3) or len(pose.status) != Q:
            raise ValueError(f"graph.pose must hold one pose per pair ({Q})")
        E = np.where(np.array([s == "ok" for s in pose.status], dtype=bool)[:, None, None], from_pose, E)
    models = np.full((Q, 3, 3), np.nan)
    for q, k in enumerate(kinds):
        if k == "essential":
            models[q] = E[q]
        elif k == "homography":
            models[q] = H[q]
    return models, kinds


def guided_match_pairs(descriptors: Sequence, features: Sequence, camera_matrix, graph, inlier_threshold, *,
                       use_pose: bool = False, max_distance: int = 64, ratio=0.8, cross_check: bool = True,
                       max_pairs_per_call: int = MAX_PAIRS_PER_CALL) -> PairMatches:
    """The second matching pass over a verified ``ViewGraph``: ``guided_match_models`` with the pairs, kinds and models of
    ``graph`` (``verify_pairs``'s result) and ``inlier_threshold`` (a number or one per pair; usually the one the graph was
    verified with).  With ``use_pose`` an essential pair whose ``graph.pose.status`` is ``"ok"`` is gated by ``E = [t]x R`` of
    ``graph.pose`` — the refined pose when ``refine_pose_rounds`` ran — instead of the five-point winner.  The result's
    ``matches`` go straight into ``verify_pairs`` and ``build_tracks``."""
    models, kinds = graph_models(graph, use_pose)
    return guided_match_models(descriptors, features, camera_matrix, graph.pairs, models, kinds, inlier_threshold,
                               max_distance=max_distance, ratio=ratio, cross_check=cross_check,
                               max_pairs_per_call=max_pairs_per_call)
