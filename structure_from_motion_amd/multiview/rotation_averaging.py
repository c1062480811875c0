"""Rotation averaging over a verified view graph on the GPU (``sfm_average_rotations``).

A view graph holds one relative rotation per verified pair (``verify_pairs(..., relative_pose=True)``: ``graph.pose.R[q]``
with ``x_j ~ R_q x_i``).  ``average_rotations`` solves for one absolute world -> camera rotation per camera that agrees with
all of them at once, ``R_q ~ R_j R_i^T``: a start from the heaviest breadth-first spanning tree of the root, then
iteratively reweighted Gauss-Newton steps on the weighted graph Laplacian, each solved by conjugate gradients.  It also
returns every edge's residual against the result, which exposes a pair whose rotation disagrees with the loops it sits in.

The squared loss is pulled far off by one wrong pair.  ``"huber"`` from the tree start tolerates them.  ``"cauchy"`` rejects
them best but wants a start: from the tree it usually stays in a bad minimum, so run Huber first and pass its rotations as
``initial_rotations``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import numpy.typing as npt

from ._graph_args import LOSSES, MAX_EDGES, _checked, _positive, _root_alone, _scatter  # noqa: F401

ROTATION_TOLERANCE = 1e-6   # an active edge's R_q: max |R^T R - I| and det > 0


@dataclass
class GlobalRotations:
    R: npt.NDArray             # (C, 3, 3) world -> camera; the root's is the identity (or its given one); NaN where unregistered
    registered: npt.NDArray    # (C,) bool: connected to the root through active edges
    level: npt.NDArray         # (C,) edges on the shortest active path to the root, -1 where unregistered
    residual_deg: npt.NDArray  # (Q,) angle of R_j^T R_q R_i in degrees; NaN for an inactive edge or an unregistered end
    steps: int                 # completed Gauss-Newton steps
    cg_iterations: int         # conjugate-gradient iterations over all steps
    initial_cost: float        # sum of w rho(angle^2) in rad^2 at the start (NaN for "bad_index")
    final_cost: float          # ... at the result
    status: str                # "converged", "max_steps", "cg_failed" or "bad_index"


def active_edges(relative_rotations: npt.NDArray, weights: npt.NDArray) -> npt.NDArray:
    """(Q,) bool: the weight finite and > 0 and the nine entries of R_q finite."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(weights) & (weights > 0) & np.all(np.isfinite(relative_rotations.reshape(-1, 9)), axis=1)


def average_rotations(num_cameras: int, pairs, relative_rotations, weights=None, root: int = 0, loss: str = "squared",
                      loss_scale_deg: float = 1.0, initial_rotations=None, max_steps: int = 50, max_cg_iterations: int = 500,
                      cg_tolerance: float = 1e-6, step_tolerance: float = 1e-8) -> GlobalRotations:
    """Absolute rotations of ``num_cameras`` cameras from Q relative ones.

    ``pairs`` (Q, 2) integer camera indices (i, j), either orientation, parallel pairs allowed, no self-pair;
    ``relative_rotations`` (Q, 3, 3) with ``R_q ~ R_j R_i^T`` (the convention of ``PairPoses.R``); ``weights`` (Q,), default
    ones.  An edge whose weight is not finite and positive, or whose rotation has a non-finite entry, is inactive: it is
    ignored and its residual is NaN.  An active edge's matrix must be a rotation (``|R^T R - I| <= 1e-6``, ``det > 0``).
    Cameras that active edges do not connect to ``root`` are unregistered (``R`` NaN).  The root is held at the identity, or
    with ``initial_rotations`` (C, 3, 3) at its given rotation; the given rotations replace the spanning-tree start (those
    of unregistered cameras are not read).  ``loss`` is ``"squared"``, ``"huber"`` or ``"cauchy"`` on the edge angle with
    the scale ``loss_scale_deg``.  ``"cauchy"`` wants a start: pass the rotations of a ``"huber"`` run as
    ``initial_rotations``; from the tree it usually stays far from the answer.  The steps stop when the largest component
    of a step is at most ``step_tolerance`` radians (``"converged"``), after ``max_steps`` (``"max_steps"``), or when the
    conjugate gradients (at most ``max_cg_iterations`` per step, to ``cg_tolerance`` relative residual) break down
    (``"cg_failed"``).  A call is reproducible bit for bit.  Every argument is checked before any device work
    (``ValueError``); ``Q = 0`` needs no GPU."""
    C, pair_arr, rel, w, root, angle, init, limits = _checked(
        num_cameras, pairs, (relative_rotations, "relative_rotations", (3, 3)), weights, root, loss, loss_scale_deg, math.inf,
        math.radians, (initial_rotations, "initial_rotations", (3, 3)),
        dict(max_steps=max_steps, max_cg_iterations=max_cg_iterations, cg_tolerance=cg_tolerance, step_tolerance=step_tolerance))
    act = active_edges(rel, w)
    if act.any():
        Ra = rel[act]
        gram = np.einsum("qki,qkj->qij", Ra, Ra) - np.eye(3)
        if np.max(np.abs(gram)) > ROTATION_TOLERANCE or np.any(np.linalg.det(Ra) <= 0):
            bad = np.nonzero(act)[0][int(np.argmax((np.max(np.abs(gram), axis=(1, 2)) > ROTATION_TOLERANCE) |
                                                   (np.linalg.det(Ra) <= 0)))]
            raise ValueError(f"relative_rotations[{bad}] is not a rotation (|R^T R - I| <= {ROTATION_TOLERANCE}, det > 0)")
    if len(pair_arr) == 0:   # nothing to average: the root alone is registered
        R = np.full((C, 3, 3), np.nan)
        R[root] = np.eye(3) if init is None else init[root]
        return GlobalRotations(R, *_root_alone(C, root), np.zeros(0), 0, 0, 0.0, 0.0, "converged")
    import torch

    from .. import device

    device.require_gpu()
    R, registered, level, residual, info = device.average_rotations(
        device.to_device(pair_arr.astype(np.int32), torch.int32), device.to_device(rel), device.to_device(w), C, root,
        None if init is None else device.to_device(init), loss, math.radians(angle), **limits)
    rec = device.read_rotavg_info(info)
    return GlobalRotations(R.cpu().numpy(), registered.cpu().numpy().astype(bool), level.cpu().numpy().astype(np.int64),
                           np.degrees(residual.cpu().numpy()),
                           rec.steps, rec.cg_iterations, rec.initial_cost, rec.final_cost, device.ROTAVG_STATUS[rec.status])


def graph_edges(graph, kinds: Sequence[str] = ("essential",)):
    """The edges ``average_graph_rotations`` uses: (indices into the graph's pairs, pairs (n, 2), R (n, 3, 3), weights (n,)) of
    the pairs with ``pose.status == "ok"`` and a kind in ``kinds``; the weight is ``pose.in_front``."""
    if graph.pose is None:
        raise ValueError("average_graph_rotations needs graph.pose: call verify_pairs with relative_pose=True")
    use = np.array([s == "ok" and k in kinds for s, k in zip(graph.pose.status, graph.kind)], dtype=bool)
    idx = np.nonzero(use)[0]
    return idx, np.asarray(graph.pairs).reshape(-1, 2)[idx], np.asarray(graph.pose.R).reshape(-1, 3, 3)[idx], \
        np.asarray(graph.pose.in_front, dtype=np.float64)[idx]


def average_graph_rotations(graph, num_images: int, root: Optional[int] = None, kinds: Sequence[str] = ("essential",),
                            **options) -> GlobalRotations:
    """``average_rotations`` on a ``ViewGraph``: the pairs with ``pose.status == "ok"`` and a kind in ``kinds``, each with its
    ``pose.R`` and the weight ``pose.in_front`` (the inliers in front of both cameras).  ``residual_deg`` has one entry per pair
    of the graph, NaN for the pairs that were not used.  ``root=None`` is the lower image of the heaviest used pair (the
    first of equals), image 0 when no pair is used.  ``ValueError`` without ``graph.pose``.  ``options`` as
    ``average_rotations``."""
    idx, pairs, R, w = graph_edges(graph, kinds)
    if root is None:
        root = int(pairs[int(np.argmax(w))].min()) if len(idx) else 0
    r = average_rotations(num_images, pairs, R, w, root=root, **options)
    r.residual_deg = _scatter(r.residual_deg, idx, len(graph.kind))
    return r


def inconsistent_pairs(result: GlobalRotations, max_residual_deg: float) -> npt.NDArray:
    """The indices of the edges whose residual is above ``max_residual_deg`` (NaN residuals are not)."""
    limit = _positive(max_residual_deg, "max_residual_deg")
    with np.errstate(invalid="ignore"):
        return np.nonzero(result.residual_deg > limit)[0]
