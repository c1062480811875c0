"""Host glue of the PnP routes: (X, Feature) items as an array, and the logger of their debug line."""
from __future__ import annotations

import logging

import numpy as np

logger = logging.getLogger(__name__)   # one line per call (ransac/_device_route.py)


def item_array(data) -> np.ndarray:
    """(len, 5) float64 {X, Y, Z, u, v} of (X, Feature) items."""
    n = len(data)
    out = np.empty((n, 5), dtype=np.float64)
    if n:
        out[:, :3] = np.array([np.asarray(item[0], dtype=np.float64).reshape(3) for item in data])
        out[:, 3] = np.fromiter((item[1].x for item in data), dtype=np.float64, count=n)
        out[:, 4] = np.fromiter((item[1].y for item in data), dtype=np.float64, count=n)
    return out
