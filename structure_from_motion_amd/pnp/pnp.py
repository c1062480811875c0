"""RANSAC absolute pose (PnP): register a further view against 3-D points that are already triangulated.

Data items are ``(X, f)`` pairs: ``X`` a 3-D point (length-3 float array) in the frame of camera 1, ``f`` the ``Feature`` of
its match in the new image, in pixels.  The model is ``(R, t)`` with ``x_cam = R X + t`` — the convention of
``recover_r_t_from_e`` and ``Transform3D.from_rmat_t``.  The RANSAC contract is the reference's ``fit_with_ransac``
(``lib/ransac/ransac.py``) with a six-item sample (the DLT) or a four-item one (P3P, ``solver="p3p"``):
``estimate_pose_pnp_with_ransac`` passes the tagged fitter / scorer below, which ``fit_with_ransac`` routes to the HIP
kernels of ``csrc/sfm_pnp.hip``; the same call with untagged callables runs on the host.
"""
from __future__ import annotations

from functools import partial
from typing import Sequence, Tuple

import numpy as np
import numpy.typing as npt

from ..common.feature import Feature
from ..epipolar import _engine
from ..feature_matching.matching import Match
from ..ransac.ransac import (DEFAULT_MAX_ITERATIONS, DeviceSpec, ErrorAggregationMethod, aggregation_code, fit_with_ransac,
                             solver_sample_size)
from . import p3p

PnPItem = Tuple[npt.NDArray, Feature]
PnPModel = Tuple[npt.NDArray, npt.NDArray]

SAMPLE_SIZE = 6
# sigma_11 / sigma_1 of the conditioned 12 x 12 DLT matrix below this: the sample is degenerate (coplanar or collinear
# points have three or more null vectors).  The same floor as kPnPDegenerateFloor of csrc/sfm_pnp.hip.
DEGENERATE_FLOOR = 1e-9


class PnPCalculationError(Exception):
    """Raised when a sampled six-tuple is degenerate (like EightPointCalculationError for the essential matrix)."""


def check_camera_matrix(camera_matrix) -> npt.NDArray:
    """K as a float64 (3, 3) array; row 2 must be (0, 0, 1) (the scorer's p_2 = c_2) and the 2 x 2 block of rows 0 and 1
    invertible.  All six entries of rows 0 and 1 count everywhere in this module: K may carry skew and K[1, 0]."""
    K = np.asarray(camera_matrix, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera matrix must be 3x3, got shape {K.shape}")
    if not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise ValueError("row 2 of the camera matrix must be (0, 0, 1)")
    det = K[0, 0] * K[1, 1] - K[0, 1] * K[1, 0]
    if det == 0.0 or np.isnan(det):
        raise ValueError("the camera matrix is singular: K[0,0] K[1,1] - K[0,1] K[1,0] is zero or not a number")
    return K


def normalized_coords(K, u, v):
    """(x, y) with (x, y, 1) = K^-1 (u, v, 1), in the operation order of csrc/sfm_pnp.h (normalized_coords): the 2 x 2 block
    of K by Cramer's rule; when K[0][1] and K[1][0] are both exactly zero, the two plain divisions (the same values, and the
    bits of the results at such cameras).  u, v: floats or arrays."""
    du = u - K[0][2]
    dv = v - K[1][2]
    if K[0][1] == 0.0 and K[1][0] == 0.0:
        return du / K[0][0], dv / K[1][1]
    det = K[0][0] * K[1][1] - K[0][1] * K[1][0]
    return (du * K[1][1] - K[0][1] * dv) / det, (K[0][0] * dv - K[1][0] * du) / det


def pnp_model_fitter(items: Sequence[PnPItem], camera_matrix: npt.NDArray) -> PnPModel:
    """(R, t) from exactly six 2D-3D pairs by the six-point DLT (the RANSAC model fitter; host form).

    K-normalised 2-D side (``normalized_coords``: the whole 2 x 2 block of K); the 3-D side conditioned (centroid
    subtracted, mean distance sqrt(3)); the null vector of the 12 x 12 system A p = 0 as P = [M | p4]; conditioning
    undone; P negated if det(M) < 0; R = U V^T of M = U S V^T; t = p4 / mean(S).  Raises PnPCalculationError for a degenerate sample (see DEGENERATE_FLOOR)."""
    if len(items) != SAMPLE_SIZE:
        raise ValueError("Six 2D-3D pairs are expected.")
    K = np.asarray(camera_matrix, dtype=np.float64)
    X = np.array([np.asarray(item[0], dtype=np.float64).reshape(3) for item in items])
    x, y = normalized_coords(K, np.array([float(item[1].x) for item in items]), np.array([float(item[1].y) for item in items]))
    centroid = X.mean(axis=0)
    scale = np.sqrt(3.0) / np.linalg.norm(X - centroid, axis=1).mean()
    Xh = np.hstack([(X - centroid) * scale, np.ones((SAMPLE_SIZE, 1))])
    A = np.zeros((2 * SAMPLE_SIZE, 12))
    A[0::2, 0:4] = Xh
    A[0::2, 8:12] = -x[:, None] * Xh
    A[1::2, 4:8] = Xh
    A[1::2, 8:12] = -y[:, None] * Xh
    _, sigma, vt = np.linalg.svd(A)
    if not sigma[10] / sigma[0] >= DEGENERATE_FLOOR:
        raise PnPCalculationError("The six 3-D points of the sample are coplanar or collinear: cannot estimate the pose.")
    P = vt[-1].reshape(3, 4)
    M = scale * P[:, :3]
    p4 = P[:, 3] - M @ centroid
    if np.linalg.det(M) < 0:
        M, p4 = -M, -p4
    u, s, wt = np.linalg.svd(M)
    return u @ wt, p4 / s.mean()


def calculate_reprojection_score(model: PnPModel, item: PnPItem, camera_matrix: npt.NDArray) -> float:
    """Squared reprojection error in pixels of one 2D-3D pair under (R, t) (the RANSAC scorer); +inf for a point behind the
    camera (c_z <= 0).  Operation order fixed as in csrc/sfm_pnp.hip (pnp_score), so the device value is this one bit for bit."""
    R, t = model
    R = np.asarray(R, dtype=np.float64).tolist()
    t = np.asarray(t, dtype=np.float64).tolist()
    K = np.asarray(camera_matrix, dtype=np.float64).tolist()
    X, Y, Z = (float(v) for v in np.asarray(item[0], dtype=np.float64).reshape(3))
    c0 = ((R[0][0] * X + R[0][1] * Y) + R[0][2] * Z) + t[0]
    c1 = ((R[1][0] * X + R[1][1] * Y) + R[1][2] * Z) + t[1]
    c2 = ((R[2][0] * X + R[2][1] * Y) + R[2][2] * Z) + t[2]
    if c2 <= 0.0:
        return float("inf")
    p0 = (K[0][0] * c0 + K[0][1] * c1) + K[0][2] * c2
    p1 = (K[1][0] * c0 + K[1][1] * c1) + K[1][2] * c2
    du = p0 / c2 - float(item[1].x)
    dv = p1 / c2 - float(item[1].y)
    return du * du + dv * dv


P3P_SAMPLE_SIZE = 4


def p3p_candidates(items: Sequence[PnPItem], camera_matrix: npt.NDArray) -> list:
    """Every candidate (R, t) of the P3P solve on items 0-2, in the solver's fixed order (``pnp/p3p.py``); [] for a
    collinear triple."""
    K = np.asarray(camera_matrix, dtype=np.float64).tolist()
    X = [[float(v) for v in np.asarray(item[0], dtype=np.float64).reshape(3)] for item in items[:3]]
    if p3p.collinear(*X):
        return []
    f = [p3p.bearing(float(item[1].x), float(item[1].y), K) for item in items[:3]]
    return [(np.array(R), np.array(t)) for R, t in p3p.p3p_solve(X, f)]


def p3p_model_fitter(items: Sequence[PnPItem], camera_matrix: npt.NDArray) -> PnPModel:
    """(R, t) from exactly four 2D-3D pairs by P3P (the RANSAC model fitter of ``solver="p3p"``; host form of
    ``sfm_p3p_fit``).  Items 0-2 are solved for (up to four candidates, ``p3p_candidates``); item 3 picks the candidate with
    the strictly lowest ``calculate_reprojection_score``, the earliest on ties.  When no candidate scores below +inf the
    sample has no solution and the model is (R, t) of NaNs, which never becomes an inlier nor wins.  Raises
    PnPCalculationError when the three solve points are collinear or coincide (coplanar samples are not degenerate)."""
    if len(items) != P3P_SAMPLE_SIZE:
        raise ValueError("Four 2D-3D pairs are expected.")
    K = np.asarray(camera_matrix, dtype=np.float64)
    X = [[float(v) for v in np.asarray(item[0], dtype=np.float64).reshape(3)] for item in items[:3]]
    if p3p.collinear(*X):
        raise PnPCalculationError("The three 3-D points of the sample are collinear: cannot estimate the pose.")
    best, best_e = (np.full((3, 3), np.nan), np.full(3, np.nan)), float("inf")
    for R, t in p3p_candidates(items, K):
        e = calculate_reprojection_score((R, t), items[3], K)
        if e < best_e:
            best, best_e = (R, t), e
    return best


# fit_with_ransac recognises partials of these (with model_fit_data_count 6 for the DLT, 4 for P3P) and runs the whole loop
# on the GPU.
pnp_model_fitter._sfm_hip_role = "pnp_fitter"
p3p_model_fitter._sfm_hip_role = "p3p_fitter"
calculate_reprojection_score._sfm_hip_role = "reprojection_scorer"


def estimate_pose_pnp_with_ransac(
    camera_matrix: npt.NDArray,
    points_3d: Sequence[npt.NDArray],
    features: Sequence[Feature],
    matches: Sequence[Match],
    reprojection_threshold: float,
    min_num_extra_inliers: int | None = None,
    error_aggregation_method: ErrorAggregationMethod | None = None,
    max_iterations: int | None = None,
    refine_rounds: int = 0,
    solver: str = "dlt",
) -> Tuple[npt.NDArray, npt.NDArray, list]:
    """Pose (R, t) of a further view from 2D-3D matches with RANSAC over six-point DLT hypotheses (``solver="dlt"``, the
    default) or P3P hypotheses on four-item samples (``solver="p3p"``, ``p3p_model_fitter``).

    ``matches[i].a_index`` indexes ``points_3d`` and ``b_index`` indexes ``features`` (pixels of the new view).  A pair is an
    inlier when its squared reprojection error is at most ``reprojection_threshold`` (pixels squared).  Returns
    ``(R, t, inlier (X, Feature) pairs)``.  Raises ``ValueError`` for fewer than six matches, a malformed camera matrix or
    when no hypothesis has enough inliers, and ``PnPCalculationError`` when a sampled six-tuple is degenerate
    (``SFM_DEGENERATE=skip`` ignores such hypotheses instead).

    ``refine_rounds > 0`` refines the RANSAC winner on its inliers on the device, right after the pass (see
    ``refine_pose_pnp``, at most 20 Levenberg-Marquardt steps per round).  If no round is kept the result is exactly the
    unrefined one; otherwise the inliers are the pairs with an error of at most the threshold under the refined pose, in
    match order.  0 (the default) runs the unrefined path unchanged.

    P3P needs at least four matches and handles planar scenes, which the DLT flags as degenerate.  Its samples without a
    real solution are not errors: they never win.  Only a sample whose three solve points are collinear is degenerate
    (``PnPCalculationError`` under the default policy).  An unknown ``solver`` raises ``ValueError`` before any device
    work."""
    K = check_camera_matrix(camera_matrix)
    sample_size = solver_sample_size("pose", solver)
    if len(matches) < sample_size:
        if solver == "dlt":
            raise ValueError(f"At least six 2D-3D matches are expected, got {len(matches)}.")
        raise ValueError(f"At least four 2D-3D matches are expected for solver 'p3p', got {len(matches)}.")
    refine_rounds = _non_negative(refine_rounds, "refine_rounds")
    if refine_rounds > 0:
        return _ransac_refined(K, points_3d, features, matches, reprojection_threshold, min_num_extra_inliers,
                               error_aggregation_method, max_iterations, refine_rounds, solver)
    fitter = pnp_model_fitter if solver == "dlt" else p3p_model_fitter
    with _engine.gc_paused():
        items = [(np.asarray(points_3d[m.a_index], dtype=np.float64).reshape(3), features[m.b_index]) for m in matches]
        model, inliers = fit_with_ransac(
            items,
            model_fit_data_count=sample_size,
            model_fitter=partial(fitter, camera_matrix=K),
            inlier_scorer=partial(calculate_reprojection_score, camera_matrix=K),
            inlier_threshold=reprojection_threshold,
            min_num_extra_inliers=min_num_extra_inliers,
            error_aggregation_method=error_aggregation_method,
            max_iterations=max_iterations,
        )
    if model is None:
        raise ValueError("Could not estimate the pose with RANSAC.")
    R, t = model
    return R, t, inliers


def _non_negative(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
    return int(value)


def _items(points_3d, features, matches):
    return [(np.asarray(points_3d[m.a_index], dtype=np.float64).reshape(3), features[m.b_index]) for m in matches]


def _ransac_refined(K, points_3d, features, matches, threshold, min_extra, method, max_iterations, rounds, solver="dlt"):
    """The device route of fit_with_ransac (the one the tagged pair takes) with the refinement chained after the pass."""
    from ..ransac._device_route import ransac_on_device

    iterations = DEFAULT_MAX_ITERATIONS if max_iterations is None else max_iterations
    method = ErrorAggregationMethod.RMS if method is None else method
    min_extra = 0 if min_extra is None else min_extra
    with _engine.gc_paused():
        items = _items(points_3d, features, matches)
        model, inliers = ransac_on_device(items, DeviceSpec(K, solver), threshold, min_extra, aggregation_code(method),
                                          iterations, refine_rounds=rounds)
    if model is None:
        raise ValueError(f"No model could be found with at least {min_extra + solver_sample_size('pose', solver)} inliers.")
    R, t = model
    return R, t, inliers


def refine_pose_pnp(
    camera_matrix: npt.NDArray,
    points_3d: Sequence[npt.NDArray],
    features: Sequence[Feature],
    matches: Sequence[Match],
    R: npt.NDArray,
    t: npt.NDArray,
    reprojection_threshold: float,
    rounds: int = 1,
    max_steps: int = 20,
    error_aggregation_method: ErrorAggregationMethod | None = None,
) -> Tuple[npt.NDArray, npt.NDArray, list]:
    """Refine a pose (R, t) on its inliers by Levenberg-Marquardt on the squared reprojection error (``sfm_pnp_refine``).

    The inliers of (R, t) are the pairs with an error of at most ``reprojection_threshold``.  Up to ``rounds`` times,
    at most ``max_steps`` LM steps minimise the sum of their errors, every pair is re-scored, and the result is kept iff it
    has more inliers, or as many and a lower aggregated error (``error_aggregation_method``, default RMS).  Returns
    ``(R, t, inlier (X, Feature) pairs in match order)``; when no round is kept, R and t are the given ones.  Every
    argument is checked before any device work."""
    K = check_camera_matrix(camera_matrix)
    if len(matches) < SAMPLE_SIZE:
        raise ValueError(f"At least six 2D-3D matches are expected, got {len(matches)}.")
    R = np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if R.shape != (3, 3) or t.size != 3:
        raise ValueError(f"R must be 3x3 and t of length 3, got shapes {R.shape} and {t.shape}")
    rounds = _non_negative(rounds, "rounds")
    max_steps = _non_negative(max_steps, "max_steps")
    method = ErrorAggregationMethod.RMS if error_aggregation_method is None else error_aggregation_method
    aggregation = aggregation_code(method)
    from .. import device
    from . import _engine as pnp_engine

    with _engine.gc_paused():
        items = _items(points_3d, features, matches)
    n = len(items)
    dev = device.require_gpu()
    pts = device.to_device(pnp_engine.item_array(items)).reshape(1, n, 5)
    model = np.concatenate([R.reshape(9), t.reshape(3)])
    mask, err = _score_pose(pts, model, K, reprojection_threshold, aggregation, dev)
    model_out, mask_out, info = device.pnp_refine(pts, device.to_device(model).reshape(1, 12), mask, err, K,
                                                  reprojection_threshold, aggregation, rounds, max_steps)
    if device.read_pnp_refine_info(info)[0].accepted > 0:
        m = model_out[0].cpu().numpy()
        R, t, keep = m[:9].reshape(3, 3).copy(), m[9:].copy(), mask_out[0].cpu().numpy()
    else:
        R, t, keep = R.copy(), t.reshape(3).copy(), mask[0].cpu().numpy()
    return R, t, [items[i] for i in np.nonzero(keep)[0].tolist()]


def _score_pose(pts, model, K, threshold, aggregation, dev):
    """(mask uint8 [1,N], err f64 [1]) of one pose by the device scorer: the mask of sfm_pnp_inlier_mask (e <= threshold),
    and the aggregated error of its inliers from sfm_pnp_score, with six of them standing in as the sample (a sample item
    with e <= threshold enters the sums like any other inlier)."""
    import torch

    from .. import device

    n = pts.shape[1]
    model_d = device.to_device(model).reshape(1, 1, 12)
    none = torch.full((1, 1, 8), -1, dtype=torch.int32, device=dev)
    record = torch.zeros((1, 5), dtype=torch.int64, device=dev)   # best_h = 0: the single model
    mask = device.pnp_inlier_mask(pts, model_d, none, K, record, threshold)
    inliers = torch.nonzero(mask[0]).flatten()
    if inliers.numel() < SAMPLE_SIZE:
        return mask, torch.full((1,), float("inf"), dtype=torch.float64, device=dev)
    S = torch.full((1, 1, 8), -1, dtype=torch.int32, device=dev)
    S[0, 0, :SAMPLE_SIZE] = inliers[:SAMPLE_SIZE].to(torch.int32)
    cnt, s1, s2 = device.pnp_score(pts, model_d, S, K, threshold)
    count = cnt.to(torch.float64) + SAMPLE_SIZE
    err = [s1, s2, s1 / count, torch.sqrt(s2 / count)][aggregation]
    return mask, err.reshape(1).contiguous()
