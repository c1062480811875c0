"""RANSAC estimation of a homography between two views, and the choice between an essential matrix and a homography as the
model of an image pair.

The hot path — four-point fits, the symmetric transfer error of every hypothesis on every match, selection, mask — runs as
HIP kernels (csrc/sfm_homography.hip, ``device.HomographyWorkspace``).  ``homography_model_fitter`` and
``calculate_transfer_error_score`` are the host forms of one fit and one score, with the arithmetic of the kernels;
``fit_with_ransac`` recognises partials of them and runs the whole loop on the GPU.
"""
from __future__ import annotations

from functools import partial
from typing import NamedTuple, Optional, Tuple

import numpy as np
import numpy.typing as npt

from ..common.feature import Feature
from ..feature_matching.matching import Match
from ..ransac.ransac import (DEFAULT_MAX_ITERATIONS, ErrorAggregationMethod, aggregation_code, fit_with_ransac,
                             solver_sample_size)
from . import _engine
from .eight_point import to_normalized_image_coords

FeaturePair = Tuple[Feature, Feature]

DEGENERATE_FLOOR = 1e-9   # a sample is degenerate when sigma_8 / sigma_1 of its conditioned 8 x 9 system is below this
MAX_HOMOGRAPHY_RATIO = 0.8   # COLMAP's max_H_inlier_ratio


class HomographyCalculationError(ArithmeticError):
    """A four-item sample does not determine a homography: a repeated item, three points collinear in both images, or four
    coincident points."""


def check_camera_matrix(camera_matrix) -> npt.NDArray:
    """K as a float64 (3, 3) array with finite entries and non-zero focal lengths (what the K-normalisation divides by)."""
    K = np.asarray(camera_matrix, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera matrix must be 3x3, got shape {K.shape}")
    if not np.all(np.isfinite(K)) or K[0, 0] == 0.0 or K[1, 1] == 0.0:
        raise ValueError("the camera matrix must be finite with non-zero K[0,0] and K[1,1]")
    return K


def _condition(x, y):
    """Centroid and scale (mean distance sqrt(2)) of four points, in the kernel's operation order."""
    cx = (((x[0] + x[1]) + x[2]) + x[3]) / 4.0
    cy = (((y[0] + y[1]) + y[2]) + y[3]) / 4.0
    dist = np.float64(0.0)
    for i in range(4):
        dx, dy = x[i] - cx, y[i] - cy
        dist = dist + np.sqrt(dx * dx + dy * dy)
    return cx, cy, np.sqrt(np.float64(2.0)) / (dist / 4.0)


def fit_homography(xa, ya, xb, yb):
    """Four-point DLT of x_b ~ H x_a -> (H (9,) row-major with ||H||_F = 1 and det H >= 0, sigma_8 / sigma_1 of the
    conditioned 8 x 9 system).  The sample is degenerate when ``not (ratio >= DEGENERATE_FLOOR)``; H is then returned as
    it comes out (NaNs for a system that is not finite)."""
    xa, ya, xb, yb = (np.asarray(v, dtype=np.float64) for v in (xa, ya, xb, yb))
    with np.errstate(all="ignore"):
        cax, cay, sa = _condition(xa, ya)
        cbx, cby, sb = _condition(xb, yb)
        A = np.zeros((8, 9))
        for i in range(4):
            x, y = (xa[i] - cax) * sa, (ya[i] - cay) * sa
            u, v = (xb[i] - cbx) * sb, (yb[i] - cby) * sb
            A[2 * i] = [x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u]
            A[2 * i + 1] = [0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v]
        if not np.all(np.isfinite(A)):
            return np.full(9, np.nan), np.float64(np.nan)
        _, sigma, vt = np.linalg.svd(A)
        ht = vt[-1]
        ratio = sigma[7] / sigma[0]
        m = np.empty(9)
        for r in range(3):
            m[3 * r] = sa * ht[3 * r]
            m[3 * r + 1] = sa * ht[3 * r + 1]
            m[3 * r + 2] = ht[3 * r + 2] - sa * (ht[3 * r] * cax + ht[3 * r + 1] * cay)
        h = np.empty(9)
        for c in range(3):
            h[c] = m[c] / sb + cbx * m[6 + c]
            h[3 + c] = m[3 + c] / sb + cby * m[6 + c]
            h[6 + c] = m[6 + c]
        norm2 = np.float64(0.0)
        for k in range(9):
            norm2 = norm2 + h[k] * h[k]
        h = h / np.sqrt(norm2)
        det = (h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6])) + h[2] * (h[3] * h[7] - h[4] * h[6])
        return (-h if det < 0.0 else h), ratio


def transfer_error(h, xa, ya, xb, yb):
    """Symmetric transfer error of {xa, ya, xb, yb} under H (9 values, row-major) in the kernel's operation order: the
    squared distance of H x_a from x_b plus that of adj(H) x_b from x_a; +inf when either point maps through the line at
    infinity (third coordinate <= 0).  Floats or arrays."""
    h = [np.float64(v) for v in np.ravel(h)]
    g = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
         h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
         h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    with np.errstate(all="ignore"):
        p0 = (h[0] * xa + h[1] * ya) + h[2]
        p1 = (h[3] * xa + h[4] * ya) + h[5]
        p2 = (h[6] * xa + h[7] * ya) + h[8]
        q0 = (g[0] * xb + g[1] * yb) + g[2]
        q1 = (g[3] * xb + g[4] * yb) + g[5]
        q2 = (g[6] * xb + g[7] * yb) + g[8]
        du, dv = p0 / p2 - xb, p1 / p2 - yb
        eu, ev = q0 / q2 - xa, q1 / q2 - ya
        e = (du * du + dv * dv) + (eu * eu + ev * ev)
        return np.where((p2 <= 0.0) | (q2 <= 0.0), np.inf, e)[()]


def homography_model_fitter(matching_features: list[FeaturePair], camera_matrix: npt.NDArray) -> npt.NDArray:
    """Homography (3, 3) from exactly four pixel-coordinate pairs, mapping K-normalised coordinates of image a to image b
    (the RANSAC model fitter).  Raises ``HomographyCalculationError`` for a degenerate sample."""
    if 4 != len(matching_features):
        raise ValueError("Four feature pairs are expected.")
    a = [to_normalized_image_coords(pair[0], camera_matrix) for pair in matching_features]
    b = [to_normalized_image_coords(pair[1], camera_matrix) for pair in matching_features]
    h, ratio = fit_homography([f.x for f in a], [f.y for f in a], [f.x for f in b], [f.y for f in b])
    if not (ratio >= DEGENERATE_FLOOR):
        raise HomographyCalculationError(
            "The four pairs of a sample do not determine a homography (a repeated pair or three collinear points).")
    return h.reshape(3, 3)


def calculate_transfer_error_score(h: npt.NDArray, matching_features: FeaturePair, camera_matrix: npt.NDArray) -> float:
    """Symmetric transfer error of one pixel-coordinate pair under ``h`` after K-normalisation (the RANSAC scorer)."""
    a = to_normalized_image_coords(matching_features[0], camera_matrix)
    b = to_normalized_image_coords(matching_features[1], camera_matrix)
    return float(transfer_error(h, np.float64(a.x), np.float64(a.y), np.float64(b.x), np.float64(b.y)))


# fit_with_ransac recognises partials of these and runs the whole loop on the GPU.
homography_model_fitter._sfm_hip_role = "homography_fitter"
calculate_transfer_error_score._sfm_hip_role = "transfer_scorer"


def _check_call(camera_matrix, matches):
    """What both public functions refuse before any device work."""
    K = check_camera_matrix(camera_matrix)
    if len(matches) < 4:
        raise ValueError("Four feature pairs are expected.")
    return K


def estimate_homography_with_ransac(
    camera_matrix: npt.NDArray,
    features_a: list[Feature],
    features_b: list[Feature],
    matches: list[Match],
    transfer_inlier_threshold: float,
    min_num_extra_inliers: int | None = None,
    error_aggregation_method: ErrorAggregationMethod | None = None,
    max_iterations: int | None = None,
) -> Tuple[npt.NDArray, list[FeaturePair]]:
    """Estimate H from matched pixel features with RANSAC over four-point hypotheses scored by the symmetric transfer error
    in K-normalised coordinates (so ``transfer_inlier_threshold`` is in the unit of ``sed_inlier_threshold``).  The
    contract of ``estimate_essential_mat_with_ransac``: the same two samplers, the winner's sample first among the inliers
    and then the survivors in the order of the shuffled list, deep copies of the caller's features.

    Returns ``(H (3, 3), inlier (Feature, Feature) pairs)``.  H maps K-normalised coordinates, x_b ~ H x_a, with
    ||H||_F = 1 and det H >= 0; for pixels use ``K @ H @ inv(K)``.

    Raises ``ValueError`` for fewer than four matches or when no hypothesis has enough inliers, and
    ``HomographyCalculationError`` when a sampled four-tuple is degenerate (``SFM_DEGENERATE=skip`` ignores such hypotheses
    instead)."""
    K = _check_call(camera_matrix, matches)
    with _engine.gc_paused():
        feature_pairs = _engine.match_pairs(features_a, features_b, matches)
        return fit_with_ransac(
            feature_pairs,
            model_fit_data_count=solver_sample_size("homography", "homography"),
            model_fitter=partial(homography_model_fitter, camera_matrix=K),
            inlier_scorer=partial(calculate_transfer_error_score, camera_matrix=K),
            inlier_threshold=transfer_inlier_threshold,
            min_num_extra_inliers=min_num_extra_inliers,
            error_aggregation_method=error_aggregation_method,
            max_iterations=max_iterations,
        )


class TwoViewModel(NamedTuple):
    kind: str                          # "essential" or "homography"
    E: Optional[npt.NDArray]           # (3, 3), None when no essential matrix has enough inliers
    essential_inliers: list
    H: Optional[npt.NDArray]           # (3, 3), None when no homography has enough inliers
    homography_inliers: list
    homography_count: int              # the winner's sample size plus its extra inliers (0 without a winner)
    essential_count: int
    ratio: float                       # homography_count / essential_count (inf when essential_count is 0)


def select_two_view_model(
    camera_matrix: npt.NDArray,
    features_a: list[Feature],
    features_b: list[Feature],
    matches: list[Match],
    inlier_threshold: float,
    min_num_extra_inliers: int | None = None,
    max_iterations: int | None = None,
    essential_solver: str = "five_point",
    max_homography_ratio: float = MAX_HOMOGRAPHY_RATIO,
) -> TwoViewModel:
    """Which model explains an image pair: an essential matrix (a baseline and a scene with depth) or a homography (a
    plane, or a rotation without translation, where E fits every match for any t and the recovered t is arbitrary).

    One upload of the matches and one sample table serve both RANSAC passes: the homography pass reads the first four
    entries of each row, the essential pass (``essential_solver``: ``"five_point"``, the default because its E stays valid
    on a plane, or ``"eight_point"``) the first six or eight of the same rows.  Both use ``inlier_threshold`` in
    K-normalised units, the RMS aggregation and ``min_num_extra_inliers``.  A count is the winner's sample size plus its
    extra inliers; ``kind`` is ``"homography"`` when E has no winner or ``homography_count / essential_count >
    max_homography_ratio`` (0.8 is COLMAP's ``max_H_inlier_ratio``), else ``"essential"``.

    Both passes ignore hypotheses whose sample is degenerate, whatever ``SFM_DEGENERATE`` says: the question asked here is
    which model explains the pair, and a degenerate sample is an answer, not an error.

    Raises ``ValueError`` for fewer than four matches, an unknown ``essential_solver``, or when neither model has a
    winner.  Telling a plane from a pure rotation, decomposing H and refitting the winner are out of scope."""
    from ..ransac._device_route import two_view_passes

    K = _check_call(camera_matrix, matches)
    solver_sample_size("essential", essential_solver)   # ValueError for an unknown solver
    iterations = DEFAULT_MAX_ITERATIONS if max_iterations is None else max_iterations
    min_extra = 0 if min_num_extra_inliers is None else min_num_extra_inliers
    with _engine.gc_paused():
        pairs = _engine.match_pairs(features_a, features_b, matches)
        h, h_inliers, h_count, e, e_inliers, e_count = two_view_passes(
            pairs, K, inlier_threshold, min_extra, aggregation_code(ErrorAggregationMethod.RMS), iterations, essential_solver)
    if h is None and e is None:
        raise ValueError("Could not estimate an essential matrix or a homography with RANSAC.")
    ratio = h_count / e_count if e_count else float("inf")
    kind = "homography" if e is None or ratio > max_homography_ratio else "essential"
    return TwoViewModel(kind, e, e_inliers, h, h_inliers, h_count, e_count, ratio)
