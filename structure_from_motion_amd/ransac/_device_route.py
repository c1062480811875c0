"""The device route of ``fit_with_ransac``: what happens between a tagged fitter / scorer pair (``ransac.DeviceSpec``) and the
``(model, inliers)`` the caller gets, written once for every solver of ``ransac.SOLVERS``.

``ROUTES`` holds the facts in which the solvers differ, those of a model shared through its ``Model``; ``ransac_on_device``
is the one driver over them, and ``two_view_passes`` composes the same stages (``Model.upload``, ``draw_samples``, ``run_pass``,
``ws.outcome``, ``log_pass``, ``winner``) for two passes over one upload and one sample table."""
from __future__ import annotations

import copy
import logging
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from .. import device
from ..epipolar import _engine
from ..epipolar._engine import (copy_pairs, degenerate_policy, draw_samples, inlier_order, local_optimisation_rounds,
                                pair_arrays)
from ..epipolar.eight_point import EightPointCalculationError
from ..epipolar.five_point import FivePointCalculationError
from ..epipolar.homography import HomographyCalculationError
from ..pnp import _engine as pnp_engine
from ..pnp.pnp import PnPCalculationError, check_camera_matrix
from .ransac import SOLVERS, DeviceSpec, solver_sample_size


def _upload_pairs(data, camera_matrix) -> torch.Tensor:
    """(Feature, Feature) pairs -> K-normalised corr [1, n, 4], in one upload."""
    pix = device.to_device(pair_arrays(data))   # [2, n, 2]
    return device.normalize_correspondences(pix[0], pix[1], camera_matrix).reshape(1, len(data), 4)


def _upload_items(data, camera_matrix) -> torch.Tensor:
    """(X, Feature) items -> pts [1, n, 5]."""
    return device.to_device(pnp_engine.item_array(data)).reshape(1, len(data), 5)


def _copy_items(data, order) -> list:
    return [copy.deepcopy(data[i]) for i in order.tolist()]


def _refine_pose(ws, pts, K, threshold, aggregation, rounds, steps):
    """``PnPWorkspace.refine`` chained on the pass's own buffers -> (model [1,12], mask [1,n], whether a round was kept)."""
    model, mask, info = ws.refine(pts, K, threshold, aggregation, rounds, steps)
    return model, mask, lambda: device.read_pnp_refine_info(info)[0].accepted > 0


def _refit_essential(ws, corr, best_h, threshold, aggregation, rounds):
    """``SFM_LOCAL_OPTIMIZATION``: the winner refitted on all its inliers -> as ``_refine_pose``."""
    err = ws.result.view(torch.float64)[:, 2]
    E, mask, info = device.refine_inliers(corr, ws.E[:, best_h], ws.mask, err, threshold, aggregation, rounds)
    return E, mask, lambda: device.read_refine_info(info)[0][2] > 0


class Model(NamedTuple):
    """What the solvers of one model share."""
    upload: Callable       # (data, camera_matrix) -> the items on the device, [1, n, width]
    copies: Callable       # (data, int64 indices) -> new objects equal to data[i]
    noun: str              # of the items in the debug line
    logger: logging.Logger   # one line per call, never per hypothesis
    workspace: type        # of device: the buffers of a pass
    run: Callable          # (ws, x, K, threshold, min_extra, aggregation, philox, solver): ws.run with this model's arguments
    decode: Callable       # the winner's row -> the model as the caller gets it
    tag: str               # of the debug line
    check_camera: Optional[Callable] = None   # called after the size check, before any device work
    refine: Optional[Callable] = None         # the refinement ``refine_rounds`` asks for, enqueued before the readback
    refit: Optional[Callable] = None          # the local optimisation of a winner that is known on the host


_PAIRS = dict(upload=_upload_pairs, copies=copy_pairs, noun="matches", logger=_engine.logger)
_ESSENTIAL = Model(
    **_PAIRS, workspace=device.RansacWorkspace, decode=device.model_matrix, tag="E", refit=_refit_essential,
    run=lambda ws, x, K, thr, min_extra, agg, philox, solver: ws.run(x, thr, min_extra, agg, philox=philox, solver=solver))
_HOMOGRAPHY = Model(
    **_PAIRS, workspace=device.HomographyWorkspace, decode=device.model_matrix, tag="H",
    run=lambda ws, x, K, thr, min_extra, agg, philox, solver: ws.run(x, thr, min_extra, agg, philox=philox))
_POSE = Model(
    upload=_upload_items, copies=_copy_items, noun="pairs", logger=pnp_engine.logger, workspace=device.PnPWorkspace,
    decode=device.model_pose, tag="PnP", check_camera=check_camera_matrix, refine=_refine_pose,
    run=lambda ws, x, K, thr, min_extra, agg, philox, solver: ws.run(x, K, thr, min_extra, agg, philox=philox, solver=solver))


class Route(NamedTuple):
    """The facts of one solver; its sample size is ``SOLVERS[name].sample_size``."""
    model: Model
    too_few: str              # the ValueError for fewer items than a sample
    size_check_first: bool    # whether that check comes before the ``iterations <= 0`` return (else after it)
    degenerate: type          # raised for a degenerate sample under SFM_DEGENERATE=raise ...
    degenerate_text: str      # ... with this text and "(hypothesis k, m in total)"
    philox_table: bool = False    # Philox samples come from a sampling launch of their own, not from the fit launch
    # SFM_LOCAL_OPTIMIZATION: "refit" on the winner's inliers after the readback, "refused" (the refit would take item 5 of a
    # five-point sample, which only picked the solution and may be an outlier, as a sample point), or None: not read
    local_optimisation: Optional[str] = None


ROUTES = {
    "eight_point": Route(
        # reference: data[:8] is short, eight_point_model_fitter raises (epipolar_ransac.py:31-32)
        _ESSENTIAL, "Eight feature pairs are expected.", False, EightPointCalculationError,
        "More than one eigenvalue of Y.T @ Y is small. Cannot confidently estimate fundamental matrix.",
        philox_table=True, local_optimisation="refit"),
    "five_point": Route(
        _ESSENTIAL, "Six feature pairs are expected.", True, FivePointCalculationError,
        "A sampled six-tuple is degenerate for the five-point solver", local_optimisation="refused"),
    "homography": Route(
        _HOMOGRAPHY, "Four feature pairs are expected.", True, HomographyCalculationError,
        "A sampled four-tuple does not determine a homography (a repeated pair or three collinear points)."),
    "dlt": Route(
        _POSE, "Six 2D-3D pairs are expected.", False, PnPCalculationError,
        "The six 3-D points of a sample are coplanar or collinear: cannot estimate the pose."),
    "p3p": Route(
        _POSE, "Four 2D-3D pairs are expected.", False, PnPCalculationError,
        "The three 3-D points a P3P sample solves for are collinear: cannot estimate the pose."),
}
assert ROUTES.keys() == SOLVERS.keys()


def run_pass(solver: str, ws, x, threshold, min_extra, aggregation, philox=None, camera_matrix=None) -> None:
    """One pass of ``solver`` on the workspace ``ws`` over the uploaded items ``x``, for the sample table in ``ws.S`` or, with
    ``philox`` (the third value of ``draw_samples``), for Philox samples: every solver draws them inside its fit launch but the
    eight-point pass, which fills its table with a sampling launch first.  ``camera_matrix``: pose solvers only."""
    route = ROUTES[solver]
    if philox is not None and route.philox_table:
        device.sample_philox(philox[0], 0, ws.h, ws.n, out=ws.S)
        philox = None
    route.model.run(ws, x, camera_matrix, threshold, min_extra, aggregation, philox, solver)


def log_pass(solver: str, ws, sampler: str, outcome) -> None:
    """The one debug line of a pass and its ``ws.outcome``."""
    model = ROUTES[solver].model
    if model.logger.isEnabledFor(logging.DEBUG):
        model.logger.debug("RANSAC-%s: %d %s x %d hypotheses (%s sampler): best hypothesis %d, %d extra inliers, "
                           "aggregated error %.6g, %d degenerate sample(s)", model.tag, ws.n, model.noun, ws.h, sampler,
                           outcome.best_h, outcome.extra_inliers, outcome.error, outcome.n_flagged)


def winner(solver: str, data, table, outcome):
    """``(model, inliers)`` of a pass: the winner's model and new copies of its inliers in the reference's order
    (``inlier_order``), or ``(None, [])`` without a winner."""
    if outcome.best_h < 0:
        return None, []
    model = ROUTES[solver].model
    return model.decode(outcome.model), model.copies(data, inlier_order(table, outcome, SOLVERS[solver].sample_size))


def ransac_on_device(data, spec: DeviceSpec, threshold, min_extra, aggregation, iterations, refine_rounds=0, refine_steps=20):
    """Device route of ``fit_with_ransac`` for the items ``data`` of ``spec.solver``.  Returns (model or None, inliers).

    Sampler ``pyshuffle`` (default) draws the hypothesis samples from the global ``random`` state exactly like the
    reference's cumulative ``random.shuffle`` (ransac.py:59-64) and advances it; ``philox`` (``SFM_SAMPLER=philox``, seed
    ``SFM_SEED`` or 64 bits from ``random``) is the counter-based sampler for large H, generated on the device.  A solver
    with fewer items than the eight of a table row reads the first ones of the same rows.  The inliers come back as new
    objects, the winner's sample first, then the survivors in the order of the shuffled list (``philox``: index order).  A
    degenerate sample raises the solver's exception under the default policy (``SFM_DEGENERATE=skip``: it never wins).

    ``refine_rounds > 0`` (pose solvers) refines the winner on its inliers right after the pass, on the pass's own buffers
    (``PnPWorkspace.refine``, at most ``refine_steps`` steps a round); ``SFM_LOCAL_OPTIMIZATION=<k>`` refits an eight-point
    winner on its inliers up to k times.  When a round is kept, the model is the refined one and the inliers are the items
    within the threshold under it, in index order (it has no "sample"); otherwise the result is the unrefined one."""
    solver = spec.solver
    route = ROUTES[solver]
    model = route.model
    n = len(data)
    short = n < SOLVERS[solver].sample_size
    if short and route.size_check_first:
        raise ValueError(route.too_few)
    if route.local_optimisation == "refused" and local_optimisation_rounds():
        raise ValueError(f"SFM_LOCAL_OPTIMIZATION is not supported with solver={solver!r}")
    if iterations <= 0:
        return None, []
    if short:
        raise ValueError(route.too_few)
    K = spec.camera_matrix if model.check_camera is None else model.check_camera(spec.camera_matrix)
    dev = device.require_gpu()
    x = model.upload(data, K)
    ws = model.workspace(1, n, iterations, dev)
    sampler, table, philox = draw_samples(ws.S, n, iterations)
    run_pass(solver, ws, x, threshold, min_extra, aggregation, philox, K)
    refined = model.refine(ws, x, K, threshold, aggregation, refine_rounds, refine_steps) if refine_rounds > 0 else None
    outcome = ws.outcome(0)
    if outcome.n_flagged and degenerate_policy() == "raise":
        raise route.degenerate(
            f"{route.degenerate_text} (hypothesis {outcome.first_flagged}, {outcome.n_flagged} in total)")
    log_pass(solver, ws, sampler, outcome)
    if outcome.best_h < 0:
        return None, []
    if route.local_optimisation == "refit":
        rounds = local_optimisation_rounds()
        if rounds:
            refined = model.refit(ws, x, outcome.best_h, threshold, aggregation, rounds)
    if refined is not None:
        row, mask, kept = refined
        if kept():   # else the unrefined winner, in the reference's ordering
            keep = np.nonzero(mask[0].cpu().numpy())[0]
            return model.decode(row[0].cpu().numpy()), model.copies(data, keep)
    return winner(solver, data, table, outcome)


def two_view_passes(data, camera_matrix, threshold, min_extra, aggregation, iterations, essential_solver):
    """The homography pass and the essential pass of ``homography.select_two_view_model`` over one upload of the pairs and
    one sample table: the homography pass reads the first four entries of each row, the essential pass the first six or
    eight of the same rows.  Flagged hypotheses never compete and never raise.  Returns (H or None, its inlier pairs, its
    count, E or None, its inlier pairs, its count), a count being the winner's sample size plus its extra inliers.  Fewer
    pairs than the essential solver's sample leave E without a winner."""
    e_size = solver_sample_size("essential", essential_solver)
    n = len(data)
    if n < SOLVERS["homography"].sample_size:
        raise ValueError(ROUTES["homography"].too_few)
    if iterations <= 0:
        return None, [], 0, None, [], 0
    dev = device.require_gpu()
    corr = _upload_pairs(data, camera_matrix)
    hws = device.HomographyWorkspace(1, n, iterations, dev)
    sampler, table, philox = draw_samples(hws.S, n, iterations)
    run_pass("homography", hws, corr, threshold, min_extra, aggregation, philox)   # Philox: the fit launch fills S
    passes = [("homography", hws)]
    if n >= e_size:
        ews = device.RansacWorkspace(1, n, iterations, dev)
        ews.S.copy_(hws.S)   # the same rows: a Philox row holds all eight entries of its sample
        run_pass(essential_solver, ews, corr, threshold, min_extra, aggregation)
        passes.append((essential_solver, ews))
    results = []
    for solver, ws in passes:
        outcome = ws.outcome(0)
        log_pass(solver, ws, sampler, outcome)
        count = SOLVERS[solver].sample_size + outcome.extra_inliers if outcome.best_h >= 0 else 0
        results += [*winner(solver, data, table, outcome), count]
    if len(passes) == 1:
        results += [None, [], 0]
    return tuple(results)
