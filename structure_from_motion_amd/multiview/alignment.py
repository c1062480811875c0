"""Similarity alignment of two reconstructions: ``b ~ s R a + t`` from 3-D / 3-D pairs, some of them wrong.

Every reconstruction lives in a gauge of its own — an origin, an orientation and a unit of length.  Two sub-models that share
tracks, a model and its ground truth, or a model and surveyed points are related by a similarity, and this module estimates
it: ``estimate_similarity_with_ransac`` robustly (three-point hypotheses, scored over every pair, the winner refitted on its
inliers — all on the GPU, ``csrc/sfm_similarity.hip``), ``fit_similarity`` by plain least squares over the pairs it is given
(Umeyama 1991; Horn 1987).  The host helpers below apply, compose and invert the result and carry camera poses across.

The error of a pair is ``|s R a + t - b|^2``: squared, and in the units of side B.

A collection reconstructed in K parts needs one alignment per pair of parts that share tracks: ``align_models`` estimates them
all in one ragged device call (``csrc/sfm_align_models.hip``), pair q exactly as
``estimate_similarity_with_ransac`` would on its own, and ``merge_frames`` puts the K parts into one frame from the result.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import numpy.typing as npt

from .._native import ALIGN_STATUS as _ALIGN_STATUS   # ModelAlignments.status names by SFM_ALIGN_* code
from ..ransac.ransac import ErrorAggregationMethod, aggregation_code

SAMPLE_SIZE = 3


class SimilarityCalculationError(Exception):
    """Raised when the given pairs do not determine a similarity (collinear or coincident points, fewer than three)."""


@dataclass
class SimilarityEstimate:
    scale: float
    R: npt.NDArray           # (3, 3), a proper rotation
    t: npt.NDArray           # (3,)
    inliers: npt.NDArray     # int64 indices of the pairs with an error of at most the threshold, ascending
    error: float             # aggregated error over the inliers
    refined: bool            # a refit round was kept: the model is the least-squares one of an inlier set, not a sample's


def _points(points, name: str) -> npt.NDArray:
    array = np.asarray(points, dtype=np.float64)
    if array.ndim != 2 or array.shape[1] != 3:
        raise ValueError(f"{name} must have shape (n, 3), got {array.shape}")
    if not np.all(np.isfinite(array)):
        raise ValueError(f"{name} must be finite")
    return np.ascontiguousarray(array)


def _pairs(points_a, points_b) -> npt.NDArray:
    a, b = _points(points_a, "points_a"), _points(points_b, "points_b")
    if len(a) != len(b):
        raise ValueError(f"points_a and points_b must have equal lengths, got {len(a)} and {len(b)}")
    if len(a) < SAMPLE_SIZE:
        raise ValueError(f"At least three pairs are expected, got {len(a)}.")
    return np.ascontiguousarray(np.hstack([a, b]))


def _non_negative(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return int(value)


def estimate_similarity_with_ransac(
    points_a,
    points_b,
    inlier_threshold: float,
    iterations: int = 1000,
    min_num_extra_inliers: Optional[int] = None,
    error_aggregation: Optional[ErrorAggregationMethod] = None,
    refine_rounds: int = 2,
    seed: int = 0,
) -> Optional[SimilarityEstimate]:
    """The similarity that maps ``points_a`` onto ``points_b`` (both ``(n, 3)``, row i of one paired with row i of the other)
    by RANSAC over three-pair hypotheses, on the GPU.

    A pair is an inlier when ``|s R a + t - b|^2 <= inlier_threshold`` (squared units of side B).  ``iterations`` hypotheses
    are drawn with the Philox sampler from ``seed`` (the call is deterministic in it); a hypothesis competes when it has at
    least ``min_num_extra_inliers`` inliers besides its sample (default 0), and the lowest aggregated error wins
    (``error_aggregation``, default RMS).  The winner is then refitted on its inliers up to ``refine_rounds`` times, each
    round kept iff it has more inliers, or as many and a lower error.  Returns ``None`` when no hypothesis passes the gate,
    or for ``iterations <= 0``.  Every argument is checked before any device work (``ValueError``)."""
    pairs = _pairs(points_a, points_b)
    threshold = float(inlier_threshold)
    if np.isnan(threshold):
        raise ValueError("inlier_threshold must not be NaN")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)):
        raise ValueError(f"iterations must be an integer, got {iterations!r}")
    min_extra = 0 if min_num_extra_inliers is None else _non_negative(min_num_extra_inliers, "min_num_extra_inliers")
    try:
        aggregation = aggregation_code(ErrorAggregationMethod.RMS if error_aggregation is None else error_aggregation)
    except NotImplementedError:
        raise ValueError(f"error_aggregation must be an ErrorAggregationMethod, got {error_aggregation!r}") from None
    rounds = _non_negative(refine_rounds, "refine_rounds")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    if iterations <= 0:
        return None
    from .. import device

    dev = device.require_gpu()
    n = len(pairs)
    items = device.to_device(pairs).reshape(1, n, 6)
    ws = device.SimilarityWorkspace(1, n, int(iterations), dev)
    ws.run(items, threshold, min_extra, aggregation, philox=(int(seed), 0, 1))
    if rounds > 0:
        ws.refine(items, threshold, aggregation, rounds)
    outcome = ws.outcome()
    if outcome.best_h < 0:
        return None
    model, mask, error, refined = outcome.model, outcome.mask, outcome.error, False
    if rounds > 0:
        info = device.read_similarity_refine_info(ws.info)[0]
        if info.accepted > 0:
            model, mask, error, refined = ws.model_out[0].cpu().numpy(), ws.mask_out[0].cpu().numpy(), info.error, True
    scale, R, t = device.model_similarity(model)
    return SimilarityEstimate(scale, R, t, np.nonzero(mask)[0].astype(np.int64), float(error), refined)


def fit_similarity(points_a, points_b, mask=None) -> SimilarityEstimate:
    """The least-squares similarity over the pairs with a non-zero ``mask`` (all pairs when it is ``None``), on the GPU: for
    evaluation against a truth, and for callers who already trust their pairs.  ``inliers`` are the indices used and
    ``error`` the root mean square of their errors.  Raises ``SimilarityCalculationError`` when the pairs do not determine
    a similarity."""
    pairs = _pairs(points_a, points_b)
    n = len(pairs)
    keep = None
    if mask is not None:
        keep = np.asarray(mask)
        if keep.shape != (n,):
            raise ValueError(f"mask must have shape ({n},), got {keep.shape}")
        keep = np.ascontiguousarray(keep != 0).astype(np.uint8)
    import torch

    from .. import device

    device.require_gpu()
    items = device.to_device(pairs).reshape(1, n, 6)
    model, flags = device.fit_similarity(items, None if keep is None else device.to_device(keep, torch.uint8).reshape(1, n))
    if int(flags.cpu()[0]) != 0:
        raise SimilarityCalculationError("The pairs do not determine a similarity: collinear, coincident or too few points.")
    scale, R, t = device.model_similarity(model[0].cpu().numpy())
    used = np.arange(n, dtype=np.int64) if keep is None else np.nonzero(keep)[0].astype(np.int64)
    estimate = SimilarityEstimate(scale, R, t, used, 0.0, False)
    residual = apply_similarity(estimate, pairs[used, :3]) - pairs[used, 3:]
    estimate.error = float(np.sqrt(np.mean(np.sum(residual * residual, axis=1))))
    return estimate


# ---- host helpers (NumPy only) ------------------------------------------------------------------------------------------
def _parts(sim):
    """(s, R, t) of a SimilarityEstimate or of a plain (s, R, t) triple."""
    if isinstance(sim, SimilarityEstimate):
        return float(sim.scale), np.asarray(sim.R, dtype=np.float64), np.asarray(sim.t, dtype=np.float64).reshape(3)
    s, R, t = sim
    return float(s), np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)


def _like(sim, s, R, t):
    if isinstance(sim, SimilarityEstimate):
        return SimilarityEstimate(s, R, t, sim.inliers, sim.error, sim.refined)
    return s, R, t


def apply_similarity(sim, points) -> npt.NDArray:
    """``s R X + t`` for every row X of ``points`` (n, 3)."""
    s, R, t = _parts(sim)
    return s * (np.asarray(points, dtype=np.float64) @ R.T) + t


def transform_poses(sim, poses) -> npt.NDArray:
    """Camera poses of frame A as poses of frame B.  ``poses``: (m, 12) rows ``R | t`` (or (m, 3, 4) matrices ``[R | t]``) with
    ``x_cam = R X + t``; with ``X_b = s Rs X_a + ts`` the result is ``R' = R Rs^T``, ``t' = s t - R' ts``, in the shape given.
    Camera coordinates scale by s, so every projection is unchanged."""
    s, Rs, ts = _parts(sim)
    given = np.asarray(poses, dtype=np.float64)
    if given.ndim == 2 and given.shape[1] == 12:
        R, t = given[:, :9].reshape(-1, 3, 3), given[:, 9:]
    elif given.ndim == 3 and given.shape[1:] == (3, 4):
        R, t = given[:, :, :3], given[:, :, 3]
    else:
        raise ValueError(f"poses must have shape (m, 12) or (m, 3, 4), got {given.shape}")
    R2 = R @ Rs.T
    t2 = s * t - R2 @ ts
    if given.ndim == 2:
        return np.hstack([R2.reshape(-1, 9), t2])
    return np.concatenate([R2, t2[:, :, None]], axis=2)


def compose(second, first):
    """The similarity that applies ``first``, then ``second``."""
    s1, R1, t1 = _parts(first)
    s2, R2, t2 = _parts(second)
    return _like(second, s2 * s1, R2 @ R1, s2 * (R2 @ t1) + t2)


def invert(sim):
    """The similarity that maps side B back onto side A."""
    s, R, t = _parts(sim)
    return _like(sim, 1.0 / s, R.T, -(R.T @ t) / s)


# ---- every overlapping pair of sub-models in one call ---------------------------------------------------------
@dataclass
class ModelAlignments:
    """One row per pair (i, j): the similarity that maps model i's frame onto model j's, ``X_j ~ scale R X_i + t``."""
    scale: npt.NDArray              # (Q,) NaN unless status is "ok"
    R: npt.NDArray                  # (Q, 3, 3)
    t: npt.NDArray                  # (Q, 3)
    status: List[str]               # per pair "ok", "no_model" (no hypothesis passed the gate) or "too_few" (fewer than 3 common ids)
    inlier_count: npt.NDArray       # (Q,) common points within the threshold under the similarity (the refinement's count)
    inliers: List[npt.NDArray]      # per pair the common ids that are inliers, ascending
    common_count: npt.NDArray       # (Q,) ids the two models share: the items of the pair
    ransac_count: npt.NDArray       # (Q,) the RANSAC winner's sample size plus its extra inliers, 0 without a winner
    error: npt.NDArray              # (Q,) aggregated error of the similarity over its inliers, inf without one
    accepted: npt.NDArray           # (Q,) refit rounds whose result was kept (0: the similarity is the RANSAC winner)
    common_ids: List[npt.NDArray]   # per pair the common ids, ascending: item k of the pair is id common_ids[q][k]
    centroid: npt.NDArray           # (Q, 3) the mean of model i's common points (NaN without any): where merge_frames compares

    def estimate(self, q: int) -> Optional[SimilarityEstimate]:
        """Pair q as ``estimate_similarity_with_ransac`` returns it on the pair's items (``inliers``: positions among the common
        ids), or ``None`` unless its status is "ok"."""
        if self.status[q] != "ok":
            return None
        at = np.searchsorted(self.common_ids[q], self.inliers[q]).astype(np.int64)
        return SimilarityEstimate(float(self.scale[q]), self.R[q].copy(), self.t[q].copy(), at, float(self.error[q]),
                                  bool(self.accepted[q] > 0))


def _integer(value, name: str, minimum=None) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or (minimum is not None and value < minimum):
        at_least = "" if minimum is None else f" >= {minimum}"
        raise ValueError(f"{name} must be an integer{at_least}, got {value!r}")
    return int(value)


def _checked_models(points, point_ids):
    """-> (list of (P_k, 3) arrays, list of (P_k,) int64 id arrays), ids unique within a model."""
    if len(points) != len(point_ids):
        raise ValueError(f"points and point_ids must hold one entry per model, got {len(points)} and {len(point_ids)}")
    clouds, ids = [], []
    for k, (p, i) in enumerate(zip(points, point_ids)):
        cloud = _points(np.zeros((0, 3)) if np.size(p) == 0 else p, f"points[{k}]")
        index = np.asarray(i)
        if index.size == 0:
            index = np.zeros(0, dtype=np.int64)
        if index.ndim != 1 or len(index) != len(cloud):
            raise ValueError(f"point_ids[{k}] must have shape ({len(cloud)},), got {index.shape}")
        if not np.issubdtype(index.dtype, np.integer):
            raise ValueError(f"point_ids[{k}] must hold integers, got {index.dtype}")
        index = index.astype(np.int64)
        if len(np.unique(index)) != len(index):
            raise ValueError(f"point_ids[{k}] repeats an id")
        clouds.append(cloud)
        ids.append(index)
    return clouds, ids


def _checked_model_pairs(pairs, num_models: int) -> npt.NDArray:
    pair_arr = np.asarray(pairs)
    if pair_arr.size == 0:
        pair_arr = np.zeros((0, 2), dtype=np.int64)
    if pair_arr.ndim != 2 or pair_arr.shape[1] != 2:
        raise ValueError(f"pairs must have shape (Q, 2), got {pair_arr.shape}")
    if not np.issubdtype(pair_arr.dtype, np.integer):
        raise ValueError(f"pairs must hold integers, got {pair_arr.dtype}")
    if len(pair_arr) and (pair_arr.min() < 0 or pair_arr.max() >= num_models):
        raise ValueError(f"pairs must index models 0 .. {num_models - 1}")
    if np.any(pair_arr[:, 0] == pair_arr[:, 1]):
        raise ValueError("a pair must join two different models")
    return pair_arr.astype(np.int64)


def common_items(point_ids, pairs):
    """The items of every pair: per pair (common ids ascending, their positions in model i, their positions in model j) —
    ``np.intersect1d`` of the two id arrays."""
    out = []
    for i, j in np.asarray(pairs).tolist():
        common, at_i, at_j = np.intersect1d(point_ids[i], point_ids[j], assume_unique=True, return_indices=True)
        out.append((common.astype(np.int64), at_i.astype(np.int64), at_j.astype(np.int64)))
    return out


def align_models(points, point_ids, pairs, inlier_threshold, iterations: int = 1000, min_num_extra_inliers=3,
                 min_extra_fraction: float = 0.0, error_aggregation: Optional[ErrorAggregationMethod] = None,
                 refine_rounds: int = 2, seed: int = 0, max_hypotheses_per_call: int = 2**21) -> ModelAlignments:
    """The similarity between every pair of sub-models that share tracks, in one device call per chunk.

    ``points[k]`` is ``(P_k, 3)`` and ``point_ids[k]`` ``(P_k,)``: integers unique within a model, the global track ids.
    ``pairs`` is ``(Q, 2)`` rows ``(i, j)`` with ``i != j``.  The items of pair q are the ids common to models i and j in
    ascending order, side A from model i and side B from model j, and ``inlier_threshold`` (a scalar or one per pair) is in
    squared units of side j.

    Per pair, ``iterations`` Philox samples of three items serve a similarity pass; the gate is ``max(min_num_extra_inliers
    (an int or one per pair), floor(min_extra_fraction * n_q))``, the lowest aggregated error wins (``error_aggregation``,
    default RMS), and the winner is refitted on its inliers up to ``refine_rounds`` times, each round kept iff it has more
    inliers, or as many and a lower error.  Pair q draws with ``seed + q``, so the result does not depend on how the pairs are
    split into device calls (``max_hypotheses_per_call`` pair-hypotheses each), and ``estimate(q)`` is exactly what
    ``estimate_similarity_with_ransac`` returns for the pair's items, threshold, gate and ``seed + q``.

    Each point array is uploaded once and the ``[N, 6]`` items are gathered on the device.  Every argument is checked before
    any device work (``ValueError``)."""
    from ..epipolar.view_graph import chunk_bounds, pair_min_extra

    clouds, ids = _checked_models(points, point_ids)
    pair_arr = _checked_model_pairs(pairs, len(clouds))
    Q = len(pair_arr)
    threshold = np.asarray(inlier_threshold, dtype=np.float64)
    if threshold.ndim == 0:
        threshold = np.full(Q, float(threshold))
    if threshold.shape != (Q,):
        raise ValueError(f"inlier_threshold must be a scalar or one per pair ({Q}), got shape {threshold.shape}")
    if np.any(np.isnan(threshold)):
        raise ValueError("inlier_threshold must not be NaN")
    h = _integer(iterations, "iterations")
    try:
        aggregation = aggregation_code(ErrorAggregationMethod.RMS if error_aggregation is None else error_aggregation)
    except NotImplementedError:
        raise ValueError(f"error_aggregation must be an ErrorAggregationMethod, got {error_aggregation!r}") from None
    rounds = _non_negative(refine_rounds, "refine_rounds")
    seed = _integer(seed, "seed")
    per_call = _integer(max_hypotheses_per_call, "max_hypotheses_per_call", 1)
    items = common_items(ids, pair_arr)
    counts = np.array([len(c) for c, _, _ in items], dtype=np.int64)
    if counts.sum() >= 2**31:
        raise ValueError("the common points of all pairs must number fewer than 2^31")
    gate = pair_min_extra(counts, min_num_extra_inliers, min_extra_fraction)
    chunks = chunk_bounds(Q, h, per_call)
    offset = np.zeros(Q + 1, dtype=np.int64)
    offset[1:] = np.cumsum(counts)
    N = int(offset[-1])
    first = np.zeros(len(clouds) + 1, dtype=np.int64)   # model k's points are rows first[k] .. of the one uploaded array
    first[1:] = np.cumsum([len(c) for c in clouds])
    centroid = np.full((Q, 3), np.nan)
    for q, ((i, _), (_, at_i, _)) in enumerate(zip(pair_arr.tolist(), items)):
        if len(at_i):
            centroid[q] = clouds[i][at_i].mean(axis=0)
    common_ids = [c for c, _, _ in items]
    code = np.where(counts < SAMPLE_SIZE, 2, 1).astype(np.int32)   # before any device work: too_few / no_model
    model_out, mask_out = np.full((Q, 13), np.nan), np.zeros(N, dtype=np.uint8)
    info_count, info_error, info_accepted = np.zeros(Q, np.int64), np.full(Q, np.inf), np.zeros(Q, np.int64)
    ransac_count = np.zeros(Q, dtype=np.int64)
    if Q and h > 0:
        import torch

        from .. import device

        dev = device.require_gpu()
        side_a = np.concatenate([first[i] + at_i for (i, _), (_, at_i, _) in zip(pair_arr.tolist(), items)]) if N else np.zeros(0, np.int64)
        side_b = np.concatenate([first[j] + at_j for (_, j), (_, _, at_j) in zip(pair_arr.tolist(), items)]) if N else np.zeros(0, np.int64)
        if N:
            cloud_dev = device.to_device(np.concatenate(clouds))
            a_dev, b_dev = device.to_device(side_a, torch.int64), device.to_device(side_b, torch.int64)
            items_dev = torch.cat([cloud_dev[a_dev], cloud_dev[b_dev]], dim=1).contiguous()
        else:
            items_dev = torch.empty((0, 6), dtype=torch.float64, device=dev)
        offset_dev = device.to_device(offset, torch.int64)
        thr_dev, gate_dev = device.to_device(threshold), device.to_device(gate.astype(np.float64))
        parts = []
        for q0, q1 in chunks:
            lo, hi = int(offset[q0]), int(offset[q1])
            ws = device.AlignModelsWorkspace(q1 - q0, hi - lo, h, int(counts[q0:q1].max()), dev)
            ws.run(items_dev[lo:hi], offset_dev[q0:q1 + 1] - lo, thr_dev[q0:q1], gate_dev[q0:q1], aggregation, seed + q0,
                   seed_stride=1, refine_rounds=rounds)
            parts.append(ws)
        code = np.concatenate([device.read_align_status(ws.status) for ws in parts])
        if np.any(code == device.ALIGN_BAD_OFFSETS):
            raise RuntimeError("align_models: the device refused the offset table (SFM_ALIGN_BAD_OFFSETS)")
        model_out = np.concatenate([ws.model_out.cpu().numpy() for ws in parts])
        mask_out = np.concatenate([ws.mask_out.cpu().numpy() for ws in parts])
        info = [r for ws in parts for r in device.read_similarity_refine_info(ws.info)]
        info_count = np.array([r.count for r in info], dtype=np.int64)
        info_error = np.array([r.error for r in info], dtype=np.float64)
        info_accepted = np.array([r.accepted for r in info], dtype=np.int64)
        records = np.concatenate([ws.result.cpu().numpy() for ws in parts])   # int64 [Q, 5]: key, best_h, best_err, first_flagged, counts
        ransac_count = np.where(records[:, 1] >= 0, SAMPLE_SIZE + (records[:, 4] >> 32), 0).astype(np.int64)
        model_out[code != device.ALIGN_OK] = np.nan
    inliers = [common_ids[q][mask_out[offset[q]:offset[q + 1]] != 0] for q in range(Q)]
    return ModelAlignments(model_out[:, 12].copy(), model_out[:, :9].reshape(Q, 3, 3).copy(), model_out[:, 9:12].copy(),
                           [_ALIGN_STATUS[c] for c in code], info_count, inliers, counts, ransac_count, info_error, info_accepted,
                           common_ids, centroid)


@dataclass
class ModelFrames:
    """K sub-models in the frame of ``root``: ``X_root ~ scale[k] R[k] X_k + t[k]``."""
    scale: npt.NDArray          # (K,) NaN for a model the tree does not reach from the root
    R: npt.NDArray              # (K, 3, 3)
    t: npt.NDArray              # (K, 3)
    reached: npt.NDArray        # (K,) bool
    tree_pairs: npt.NDArray     # int64 indices of the pairs of the spanning forest, in the order Kruskal took them
    usable: npt.NDArray         # (Q,) bool: status "ok" with at least min_inliers inliers
    # the disagreement of every usable pair between reached models with the frames, NaN elsewhere: compose(G_j, S_q) against G_i
    rotation_deg: npt.NDArray   # (Q,) the angle of the rotation between the two
    log_scale: npt.NDArray      # (Q,) |log| of the ratio of their scales
    distance: npt.NDArray       # (Q,) between the two images of model i's centroid of common points, in root units

    def frame(self, k: int):
        """(scale, R, t) of model k."""
        return float(self.scale[k]), self.R[k], self.t[k]


def merge_frames(num_models: int, pairs, alignments: ModelAlignments, root: int = 0, min_inliers: int = 3) -> ModelFrames:
    """Put ``num_models`` sub-models into the frame of ``root`` from the pairwise alignments of ``align_models`` (NumPy only).

    A pair is usable when its status is "ok" and it has at least ``min_inliers`` inliers.  Kruskal's algorithm takes a maximum
    spanning forest over the usable pairs, weighted by ``inlier_count``, ties to the lower pair index; every model the tree
    reaches from ``root`` gets ``G_k``, composed along the tree with ``compose`` and ``invert``.  Every usable pair between
    reached models is then compared with the frames: ``compose(G_j, S_q)`` against ``G_i`` — a tree pair disagrees by
    round-off only, another pair by what its loop accumulates (``inconsistent_alignments``)."""
    K = _integer(num_models, "num_models", 0)
    pair_arr = _checked_model_pairs(pairs, K)
    Q = len(pair_arr)
    if len(alignments.status) != Q:
        raise ValueError(f"alignments must hold one row per pair ({Q}), got {len(alignments.status)}")
    root = _integer(root, "root", 0)
    if root >= K:
        raise ValueError(f"root must index models 0 .. {K - 1}, got {root}")
    min_inliers = _integer(min_inliers, "min_inliers", 0)
    count = np.asarray(alignments.inlier_count, dtype=np.int64)
    usable = np.array([s == "ok" for s in alignments.status], dtype=bool).reshape(Q) & (count >= min_inliers)
    sims = [(float(alignments.scale[q]), np.asarray(alignments.R[q], dtype=np.float64), np.asarray(alignments.t[q], dtype=np.float64))
            for q in range(Q)]
    # Kruskal: heaviest first, ties to the lower index
    parent = list(range(K))

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k
    tree = []
    for q in sorted(np.nonzero(usable)[0].tolist(), key=lambda q: (-int(count[q]), q)):
        a, b = find(int(pair_arr[q, 0])), find(int(pair_arr[q, 1]))
        if a != b:
            parent[a] = b
            tree.append(q)
    neighbours = [[] for _ in range(K)]
    for q in tree:
        i, j = pair_arr[q].tolist()
        neighbours[i].append((j, q, True))    # leaving i over S_q: G_j is known from G_i by the inverse
        neighbours[j].append((i, q, False))
    scale, R, t = np.full(K, np.nan), np.full((K, 3, 3), np.nan), np.full((K, 3), np.nan)
    reached = np.zeros(K, dtype=bool)
    if K:
        scale[root], R[root], t[root], reached[root] = 1.0, np.eye(3), np.zeros(3), True
        queue = [root]
        while queue:
            k = queue.pop(0)
            for other, q, forward in neighbours[k]:
                if reached[other]:
                    continue
                G_k = (float(scale[k]), R[k], t[k])
                # S_q maps i onto j: G_i = G_j o S_q, and G_j = G_i o S_q^-1
                s, Rn, tn = compose(G_k, invert(sims[q])) if forward else compose(G_k, sims[q])
                scale[other], R[other], t[other], reached[other] = s, Rn, tn, True
                queue.append(other)
    rotation_deg, log_scale, distance = np.full(Q, np.nan), np.full(Q, np.nan), np.full(Q, np.nan)
    for q in np.nonzero(usable)[0].tolist():
        i, j = pair_arr[q].tolist()
        if not (reached[i] and reached[j]):
            continue
        via = compose((float(scale[j]), R[j], t[j]), sims[q])
        direct = (float(scale[i]), R[i], t[i])
        cosine = (np.trace(via[1] @ direct[1].T) - 1.0) / 2.0
        # the angle from the sine and the cosine: acos alone loses half the digits near 0
        skew = via[1] @ direct[1].T
        sine = 0.5 * np.sqrt((skew[2, 1] - skew[1, 2]) ** 2 + (skew[0, 2] - skew[2, 0]) ** 2 + (skew[1, 0] - skew[0, 1]) ** 2)
        rotation_deg[q] = np.degrees(np.arctan2(sine, cosine))
        log_scale[q] = abs(np.log(via[0] / direct[0]))
        c = np.asarray(alignments.centroid[q], dtype=np.float64)
        distance[q] = float(np.linalg.norm(apply_similarity(via, c[None]) - apply_similarity(direct, c[None])))
    return ModelFrames(scale, R, t, reached, np.array(tree, dtype=np.int64), usable, rotation_deg, log_scale, distance)


def inconsistent_alignments(frames: ModelFrames, max_rotation_deg: float, max_log_scale: float) -> npt.NDArray:
    """The pairs whose alignment disagrees with the frames by more than ``max_rotation_deg`` degrees or ``max_log_scale`` in
    ``|log|`` of the scale ratio: int64 indices, ascending.  A tree pair never does; a pair named here closes a loop that does
    not close."""
    with np.errstate(invalid="ignore"):
        bad = (frames.rotation_deg > float(max_rotation_deg)) | (frames.log_scale > float(max_log_scale))
    return np.nonzero(bad)[0].astype(np.int64)
