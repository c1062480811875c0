"""Similarity alignment of two reconstructions: ``b ~ s R a + t`` from 3-D / 3-D pairs, some of them wrong.

Every reconstruction lives in a gauge of its own — an origin, an orientation and a unit of length.  Two sub-models that share
tracks, a model and its ground truth, or a model and surveyed points are related by a similarity, and this module estimates
it: ``estimate_similarity_with_ransac`` robustly (three-point hypotheses, scored over every pair, the winner refitted on its
inliers — all on the GPU, ``csrc/sfm_similarity.hip``), ``fit_similarity`` by plain least squares over the pairs it is given
(Umeyama 1991; Horn 1987).  The host helpers below apply, compose and invert the result and carry camera poses across.

The error of a pair is ``|s R a + t - b|^2``: squared, and in the units of side B.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import numpy.typing as npt

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
