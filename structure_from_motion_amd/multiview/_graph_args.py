"""What the solvers over a view graph (``rotation_averaging``, ``translation_averaging``) share on the host: the checks of their
arguments, the result of a graph without edges and the way of a per-edge result back onto a view graph's pairs."""
from __future__ import annotations

import math

import numpy as np

from .._native import loss_scale_ok

LOSSES = ("squared", "huber", "cauchy")
_INT32 = 2**31
MAX_EDGES = 2**30


def _integer(value, name: str, low: int, high: int = _INT32) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low or value >= high:
        raise ValueError(f"{name} must be an integer in [{low}, {high}), got {value!r}")
    return int(value)


def _positive(value, name: str, below: float = math.inf, loss_scale=None) -> float:
    """``value`` as a float, finite and in (0, ``below``).  ``loss_scale``: the map from ``value`` to the loss scale the device
    receives (degrees to radians, or to a sine), which must pass ``loss_scale_ok``."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {value!r}") from None
    if not (math.isfinite(v) and 0.0 < v < below):
        raise ValueError(f"{name} must be finite and in (0, {below}), got {value!r}")
    if loss_scale is not None and not loss_scale_ok(loss_scale(v)):
        raise ValueError(f"{name} must give a loss scale with a normal finite square, got {value!r}")
    return v


def _array(value, name: str, shape, what: str):
    try:
        arr = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a float array of shape {what}") from None
    if arr.size == 0 and 0 in shape:
        arr = np.zeros(shape)
    if arr.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, got {arr.shape}")
    return arr


def _named(rows: str, per_row) -> str:
    return "(" + ", ".join([rows, *map(str, per_row)]) + ")"


def _checked(num_cameras, pairs, measured, weights, root, loss, loss_scale_deg, scale_below, device_scale, initial, limits):
    """Every argument both solvers take, checked in the order of their signatures -> (C, pairs (Q, 2), the measurements, weights
    (Q,), root, loss_scale_deg as a float below ``scale_below`` whose ``device_scale`` (the scale the device receives) passes
    ``loss_scale_ok``, the start or None, the limits as Python numbers).  ``measured``
    and ``initial`` are (value, name, shape of one row): one row per edge and one per camera (value None: no start).
    ``limits`` maps ``max_steps``, ``max_cg_iterations``, ``cg_tolerance``, ``step_tolerance`` and any further step count to
    its value; they are checked in its order."""
    C = _integer(num_cameras, "num_cameras", 1)
    try:
        pair_arr = np.asarray(pairs)
    except (TypeError, ValueError):
        raise ValueError("pairs must be an integer array of shape (Q, 2)") from None
    if pair_arr.size == 0:
        pair_arr = np.zeros((0, 2), dtype=np.int64)
    if pair_arr.ndim != 2 or pair_arr.shape[1] != 2 or not np.issubdtype(pair_arr.dtype, np.integer):
        raise ValueError(f"pairs must be an integer array of shape (Q, 2), got {pair_arr.dtype} {pair_arr.shape}")
    Q = pair_arr.shape[0]
    if Q >= MAX_EDGES:
        raise ValueError("pairs must number fewer than 2^30")
    if Q and (pair_arr.min() < 0 or pair_arr.max() >= C):
        raise ValueError(f"pairs must hold camera indices in [0, {C})")
    if np.any(pair_arr[:, 0] == pair_arr[:, 1]):
        raise ValueError("pairs must not join a camera with itself")
    value, name, row = measured
    m = _array(value, name, (Q, *row), _named("Q", row))
    w = np.ones(Q) if weights is None else _array(weights, "weights", (Q,), "(Q,)")
    root = _integer(root, "root", 0, C)
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    scale = _positive(loss_scale_deg, "loss_scale_deg", below=scale_below, loss_scale=device_scale)
    value, name, row = initial
    init = None if value is None else _array(value, name, (C, *row), _named("C", row))
    options = {}
    for name, value in limits.items():
        if name.endswith("_tolerance"):
            options[name] = _positive(value, name, below=1.0 if name == "cg_tolerance" else math.inf)
        else:
            options[name] = _integer(value, name, 1 if name == "max_cg_iterations" else 0)
    return C, pair_arr, m, w, root, scale, init, options


def _root_alone(C: int, root: int):
    """A graph without edges: (registered, level) with the root alone registered, at level 0."""
    registered = np.zeros(C, dtype=bool)
    registered[root] = True
    return registered, np.where(registered, 0, -1)


def _scatter(values, idx, n: int):
    """(n,) NaN but for ``values`` at ``idx``: a result per used edge as one per pair of the graph."""
    out = np.full(n, np.nan)
    out[idx] = values
    return out
