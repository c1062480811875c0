"""Device route of fit_with_ransac for PnP items ((X, Feature) pairs): host glue around device.PnPWorkspace."""
from __future__ import annotations

import copy
import logging

import numpy as np

from .. import device
from ..epipolar._engine import degenerate_policy, draw_samples, inlier_order
from ..ransac.ransac import solver_sample_size

logger = logging.getLogger(__name__)


def item_array(data) -> np.ndarray:
    """(len, 5) float64 {X, Y, Z, u, v} of (X, Feature) items."""
    n = len(data)
    out = np.empty((n, 5), dtype=np.float64)
    if n:
        out[:, :3] = np.array([np.asarray(item[0], dtype=np.float64).reshape(3) for item in data])
        out[:, 3] = np.fromiter((item[1].x for item in data), dtype=np.float64, count=n)
        out[:, 4] = np.fromiter((item[1].y for item in data), dtype=np.float64, count=n)
    return out


def ransac_pnp_items(data, camera_matrix, threshold, min_extra, aggregation, iterations, refine_rounds=0, refine_steps=20,
                     solver="dlt"):
    """Returns ((R, t) or None, inlier items) with the semantics of ransac._host_loop: sample ``pyshuffle`` (default) replays
    the reference's cumulative ``random.shuffle`` and advances the global ``random`` state; ``philox`` draws on the device
    (seed ``SFM_SEED`` or 64 bits of ``random``).  Inliers come back as deep copies, the sample first, then the survivors
    in the order of the shuffled list (``philox``: index order).

    ``refine_rounds > 0`` refines the winner on its inliers right after the pass, on the pass's own buffers
    (``PnPWorkspace.refine``).  When a round is kept, the pose is the refined one and the inliers are the items with
    e <= threshold under it, in index order; otherwise the return value is the unrefined one.

    ``solver`` is ``"dlt"`` (six-item samples) or ``"p3p"`` (four-item samples: ``PyShuffleTable.S[:, :4]``, the first four
    of ``philox_sample8``); the sample size sets the minimum n, the sample the inliers start with and the degenerate error."""
    from .pnp import PnPCalculationError, check_camera_matrix

    sample_size = solver_sample_size("pose", solver)
    n = len(data)
    if iterations <= 0:
        return None, []
    if n < sample_size:
        raise ValueError(f"{'Six' if sample_size == 6 else 'Four'} 2D-3D pairs are expected.")
    K = check_camera_matrix(camera_matrix)
    dev = device.require_gpu()
    pts = device.to_device(item_array(data)).reshape(1, n, 5)
    ws = device.PnPWorkspace(1, n, iterations, dev)
    sampler, table, philox = draw_samples(ws.S, n, iterations)
    ws.run(pts, K, threshold, min_extra, aggregation, philox=philox, solver=solver)
    refined = ws.refine(pts, K, threshold, aggregation, refine_rounds, refine_steps) if refine_rounds > 0 else None
    outcome = ws.outcome(0)
    if outcome.n_flagged and degenerate_policy() == "raise":
        what = ("The six 3-D points of a sample are coplanar or collinear" if solver == "dlt" else
                "The three 3-D points a P3P sample solves for are collinear")
        raise PnPCalculationError(
            f"{what}: cannot estimate the pose. (hypothesis {outcome.first_flagged}, {outcome.n_flagged} in total)")
    if logger.isEnabledFor(logging.DEBUG):
        logger.debug("RANSAC-PnP: %d pairs x %d hypotheses (%s sampler): best hypothesis %d, %d extra inliers, "
                     "aggregated error %.6g, %d degenerate sample(s)", n, iterations, sampler, outcome.best_h,
                     outcome.extra_inliers, outcome.error, outcome.n_flagged)
    if outcome.best_h < 0:
        return None, []
    if refined is not None:
        model, mask, info = refined
        if device.read_pnp_refine_info(info)[0].accepted > 0:
            m = model[0].cpu().numpy()
            keep = np.nonzero(mask[0].cpu().numpy())[0]
            return (m[:9].reshape(3, 3).copy(), m[9:].copy()), [copy.deepcopy(data[i]) for i in keep.tolist()]
    return (outcome.R, outcome.t), [copy.deepcopy(data[i]) for i in inlier_order(table, outcome, sample_size).tolist()]
