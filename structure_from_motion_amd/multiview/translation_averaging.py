"""Translation averaging over a verified view graph on the GPU (``sfm_average_translations``).

A view graph holds one unit translation per verified pair (``verify_pairs(..., relative_pose=True)``: ``graph.pose.t[q]`` with
``x_j ~ R_q x_i + t_q``).  With the global rotations of ``average_rotations`` every pair gives a world direction between two
camera centres, ``v_q = -R_j^T t_q ~ c_j - c_i``.  ``average_translations`` solves for one position per camera that agrees
with all directions at once, by the bilinear angle-based objective of Zhuang, Cheong and Lee (BATA, CVPR 2018): the cost of
an edge is a loss of the sine of the angle between ``c_j - c_i`` and ``v_q``, so that short baselines are not favoured.  The
start is the heaviest breadth-first spanning tree of the root with unit baselines; the unit of the result is one tree
baseline, and the root sits at the origin.  ``global_poses`` joins rotations and positions into camera matrices.

The squared loss is pulled far off by one wrong direction.  ``"huber"`` with the warm-up (the first steps take every scale as
1, a convex problem whose answer does not depend on the tree) tolerates them.  ``"cauchy"`` rejects them best but wants a
start: run Huber first and pass its positions as ``initial_positions``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import numpy.typing as npt

from . import _graph_args
from ._graph_args import _array, _integer, _root_alone, _scatter
from .rotation_averaging import LOSSES, MAX_EDGES, GlobalRotations, graph_edges, inconsistent_pairs  # noqa: F401

UNIT_TOLERANCE = 1e-6   # an active edge's direction: | |v| - 1 |


@dataclass
class GlobalPositions:
    c: npt.NDArray             # (C, 3) camera centres in the world frame; the root's is 0 (or its given one); NaN where unregistered
    registered: npt.NDArray    # (C,) bool: connected to the root through active edges
    level: npt.NDArray         # (C,) edges on the shortest active path to the root, -1 where unregistered
    residual_deg: npt.NDArray  # (Q,) angle between c_j - c_i and v_q in degrees (0..180); NaN for an edge that was not used
    scale: npt.NDArray         # (Q,) d_q = max(<c_j - c_i, v_q>, 0) / |c_j - c_i|^2: 1 / baseline for an edge that fits, 0 for one that points backwards
    steps: int                 # completed steps
    cg_iterations: int         # conjugate-gradient iterations over all steps
    initial_cost: float        # sum of w rho(|d (c_j - c_i) - v|^2) at the first linearisation (NaN for "bad_index")
    final_cost: float          # ... at the result
    status: str                # "converged", "max_steps", "cg_failed" or "bad_index"


def _device_scale(angle_deg: float) -> float:
    """The loss scale the device receives: the sine of the angle."""
    return math.sin(math.radians(angle_deg))


def _checked(num_cameras, pairs, directions, weights, root, loss, loss_scale_deg, initial_positions, warmup_steps, max_steps,
             max_cg_iterations, cg_tolerance, step_tolerance):
    C, pair_arr, v, w, root, angle, init, options = _graph_args._checked(
        num_cameras, pairs, (directions, "directions", (3,)), weights, root, loss, loss_scale_deg, 90.0, _device_scale,
        (initial_positions, "initial_positions", (3,)),
        dict(warmup_steps=warmup_steps, max_steps=max_steps, max_cg_iterations=max_cg_iterations, cg_tolerance=cg_tolerance,
             step_tolerance=step_tolerance))
    return C, pair_arr, v, w, root, _device_scale(angle), init, options


def active_edges(directions: npt.NDArray, weights: npt.NDArray) -> npt.NDArray:
    """(Q,) bool: the weight finite and > 0 and the three entries of v_q finite."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(weights) & (weights > 0) & np.all(np.isfinite(directions), axis=1)


def _empty(C: int, root: int, init) -> GlobalPositions:
    c = np.full((C, 3), np.nan)
    c[root] = 0.0 if init is None else init[root]
    return GlobalPositions(c, *_root_alone(C, root), np.zeros(0), np.zeros(0), 0, 0, 0.0, 0.0, "converged")


def _run(C, pair_arr, v, w, root, loss, scale, init, options, rotations=None) -> GlobalPositions:
    import torch

    from .. import device

    device.require_gpu()
    c, registered, level, residual, d, info = device.average_translations(
        device.to_device(pair_arr.astype(np.int32), torch.int32), device.to_device(v), device.to_device(w), C, root,
        None if rotations is None else device.to_device(rotations), None if init is None else device.to_device(init), loss,
        scale, **options)
    rec = device.read_transavg_info(info)
    return GlobalPositions(c.cpu().numpy(), registered.cpu().numpy().astype(bool), level.cpu().numpy().astype(np.int64),
                           np.degrees(residual.cpu().numpy()), d.cpu().numpy(), rec.steps, rec.cg_iterations,
                           rec.initial_cost, rec.final_cost, device.TRANSAVG_STATUS[rec.status])


def average_translations(num_cameras: int, pairs, directions, weights=None, root: int = 0, loss: str = "squared",
                         loss_scale_deg: float = 2.0, initial_positions=None, warmup_steps: int = 10, max_steps: int = 500,
                         max_cg_iterations: int = 500, cg_tolerance: float = 1e-6,
                         step_tolerance: float = 1e-8) -> GlobalPositions:
    """Positions of ``num_cameras`` cameras from Q directions between them.

    ``pairs`` (Q, 2) integer camera indices (i, j), either orientation, parallel pairs allowed, no self-pair; ``directions``
    (Q, 3) unit vectors in the world frame with ``v_q ~ c_j - c_i``; ``weights`` (Q,), default ones.  An edge whose weight is
    not finite and positive, or whose direction has a non-finite entry, is inactive: it is ignored and its residual and scale
    are NaN.  An active edge's direction must be unit to 1e-6.  Cameras that active edges do not connect to ``root`` are
    unregistered (``c`` NaN).  The root is held at the origin, or with ``initial_positions`` (C, 3) at its given position; the
    given positions replace the spanning-tree start (those of unregistered cameras are not read; those of the others must be
    finite).  ``loss`` is ``"squared"``, ``"huber"`` or ``"cauchy"`` on the sine of the angle between ``c_j - c_i`` and
    ``v_q``, with the scale ``sin(loss_scale_deg)``.  The first ``warmup_steps`` steps take every edge's scale as 1, which
    frees the result from the tree; ``"cauchy"`` wants a start besides: pass the positions of a ``"huber"`` run as
    ``initial_positions`` (with ``warmup_steps=0``).  The steps stop when the largest component of a step after the warm-up is
    at most ``step_tolerance`` tree baselines (``"converged"``), after ``max_steps`` (``"max_steps"``; the alternation
    converges linearly, a few hundred steps to 1e-8), or when the conjugate gradients (at most ``max_cg_iterations`` per step,
    to ``cg_tolerance`` relative residual) break down (``"cg_failed"``).  A call is reproducible bit for bit.  Every argument
    is checked before any device work (``ValueError``); ``Q = 0`` needs no GPU."""
    C, pair_arr, v, w, root, scale, init, options = _checked(
        num_cameras, pairs, directions, weights, root, loss, loss_scale_deg, initial_positions, warmup_steps, max_steps,
        max_cg_iterations, cg_tolerance, step_tolerance)
    act = active_edges(v, w)
    if act.any():
        off = np.abs(np.linalg.norm(v[act], axis=1) - 1.0)
        if np.max(off) > UNIT_TOLERANCE:
            raise ValueError(f"directions[{np.nonzero(act)[0][int(np.argmax(off > UNIT_TOLERANCE))]}] is not a unit vector "
                             f"(| |v| - 1 | <= {UNIT_TOLERANCE})")
    if len(pair_arr) == 0:   # nothing to average: the root alone is registered
        return _empty(C, root, init)
    if init is not None:
        touched = np.zeros(C, dtype=bool)
        touched[pair_arr[act].reshape(-1)] = True
        touched[root] = True
        if not np.all(np.isfinite(init[touched])):
            raise ValueError("initial_positions must be finite for the root and every camera with an active edge")
    return _run(C, pair_arr, v, w, root, loss, scale, init, options)


def average_graph_translations(graph, rotations: GlobalRotations, num_images: int, root: Optional[int] = None,
                               kinds: Sequence[str] = ("essential",), **options) -> GlobalPositions:
    """``average_translations`` on a ``ViewGraph`` and the global rotations of ``average_graph_rotations``: of the pairs with
    ``pose.status == "ok"`` and a kind in ``kinds`` (those rotation averaging uses) the ones whose two images are registered
    in ``rotations``, each with the weight ``pose.in_front`` and the world direction ``-(R_j^T t_q) / |t_q|`` computed on the
    device from ``pose.t`` and ``rotations.R``.  ``residual_deg`` and ``scale`` have one entry per pair of the graph, NaN for
    the pairs that were not used.  ``root=None`` is the root of ``rotations`` (its camera of level 0).  ``ValueError`` without
    ``graph.pose``.  ``options`` as ``average_translations``."""
    idx, pairs, _, w = graph_edges(graph, kinds)
    C = _integer(num_images, "num_images", 1)
    R = _array(rotations.R, "rotations.R", (C, 3, 3), "(C, 3, 3)")
    reg = np.asarray(rotations.registered, dtype=bool)
    if reg.shape != (C,):
        raise ValueError(f"rotations.registered must have shape ({C},), got {reg.shape}")
    keep = reg[pairs[:, 0]] & reg[pairs[:, 1]] if len(idx) else np.zeros(0, dtype=bool)
    idx, pairs, w = idx[keep], pairs[keep], w[keep]
    t = np.asarray(graph.pose.t, dtype=np.float64).reshape(-1, 3)[idx]
    if root is None:
        at = np.nonzero(np.asarray(rotations.level) == 0)[0]
        root = int(at[0]) if len(at) else 0
    defaults = dict(loss="squared", loss_scale_deg=2.0, initial_positions=None, warmup_steps=10, max_steps=500,
                    max_cg_iterations=500, cg_tolerance=1e-6, step_tolerance=1e-8)
    unknown = set(options) - set(defaults)
    if unknown:
        raise ValueError(f"unknown options {sorted(unknown)}")
    defaults.update(options)
    loss = defaults.pop("loss")
    C, pair_arr, t, w, root, scale, init, opts = _checked(
        C, pairs, t, w, root, loss, defaults.pop("loss_scale_deg"), defaults.pop("initial_positions"), **defaults)
    if len(pair_arr) == 0:
        r = _empty(C, root, init)
    else:
        r = _run(C, pair_arr, t, w, root, loss, scale, init, opts, rotations=np.where(reg[:, None, None], R, np.nan))
    r.residual_deg, r.scale = _scatter(r.residual_deg, idx, len(graph.kind)), _scatter(r.scale, idx, len(graph.kind))
    return r


def global_poses(rotations: GlobalRotations, positions: GlobalPositions) -> npt.NDArray:
    """(C, 3, 4) camera matrices ``[R | -R c]`` (world -> camera, the ``poses`` of ``triangulate_tracks`` and ``bundle_adjust``
    once flattened); NaN where the camera is unregistered in either."""
    R, c = np.asarray(rotations.R, dtype=np.float64), np.asarray(positions.c, dtype=np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or c.shape != (R.shape[0], 3):
        raise ValueError(f"rotations.R must be (C, 3, 3) and positions.c (C, 3), got {R.shape} and {c.shape}")
    P = np.concatenate([R, -np.einsum("cij,cj->ci", R, c)[:, :, None]], axis=2)
    P[~(np.asarray(rotations.registered, dtype=bool) & np.asarray(positions.registered, dtype=bool))] = np.nan
    return P
