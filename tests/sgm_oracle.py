"""The NumPy definition of the semi-global smoothing of a plane-sweep cost volume, written from the definition and
not from csrc/sfm_sgm.hip.  Every step is an elementwise float64 ``+ - * /`` or ``min`` in the order the definition states, so
the device result is compared with it as bytes (``plane_sweep_oracle.same_bytes``).  Vectorised over the hypotheses and over the
pixels across a direction; an explicit loop along it.  Every term of a ``min`` is finite, so its order does not matter."""
import numpy as np

from plane_sweep_oracle import winners

DIRECTIONS = {8: ((0, 1), (1, 1), (-1, 1), (0, -1), (-1, -1), (1, -1), (1, 0), (-1, 0)), 4: ((0, 1), (0, -1), (1, 0), (-1, 0))}


def unary(volume, invalid_cost):
    """C': the cost where it is finite, else ``invalid_cost``."""
    return np.where(np.isfinite(volume), volume, np.float64(invalid_cost))


def step(c, Lq, p1, p2):
    """L(p, .) from C'(p, .) and L(q, .) of the pixel before, both [D, N]."""
    m = Lq.min(axis=0)
    best = np.minimum(Lq, m + p2)
    best[1:] = np.minimum(best[1:], Lq[:-1] + p1)
    best[:-1] = np.minimum(best[:-1], Lq[1:] + p1)
    return (c + best) - m


def path_costs(C, dx, dy, p1, p2):
    """L_k of one direction for C' [D, H, W]: the predecessor of (x, y) is (x - dx, y - dy); a pixel without one has L = C'."""
    D, H, W = C.shape
    p1, p2 = np.float64(p1), np.float64(p2)
    L = np.empty_like(C)
    if dy != 0:
        xq = np.arange(W) - dx
        inside = (xq >= 0) & (xq < W)
        xq = np.clip(xq, 0, W - 1)
        for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
            if not 0 <= y - dy < H:
                L[:, y] = C[:, y]
            else:
                L[:, y] = np.where(inside, step(C[:, y], L[:, y - dy][:, xq], p1, p2), C[:, y])
    else:
        for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
            if not 0 <= x - dx < W:
                L[:, :, x] = C[:, :, x]
            else:
                L[:, :, x] = step(C[:, :, x], L[:, :, x - dx], p1, p2)
    return L


def aggregate(volume, p1, p2, invalid_cost, paths):
    """S [D, H, W] of one reference: the left fold of L_k in the order of ``DIRECTIONS[paths]``."""
    C = unary(np.asarray(volume, dtype=np.float64), invalid_cost)
    S = None
    for dx, dy in DIRECTIONS[paths]:
        L = path_costs(C, dx, dy, p1, p2)
        S = L if S is None else S + L
    return S


def sgm_aggregate(volume, depths, p1=0.1, p2=0.8, invalid_cost=1.0, paths=8):
    """-> dict(depth [R, H, W], index int32, cost, aggregated [R, D, H, W])."""
    volume = np.asarray(volume, dtype=np.float64)
    R, D, H, W = volume.shape
    depths = np.broadcast_to(np.asarray(depths, dtype=np.float64), (R, D))
    out = dict(depth=np.full((R, H, W), np.nan), index=np.full((R, H, W), -1, dtype=np.int32), cost=np.full((R, H, W), np.nan),
               aggregated=np.empty((R, D, H, W)))
    for r in range(R):
        S = aggregate(volume[r], p1, p2, invalid_cost, paths)
        with np.errstate(all="ignore"):
            valid_depth = np.isfinite(depths[r]) & (depths[r] > 0.0)
        eligible = np.isfinite(volume[r]) & valid_depth[:, None, None]
        out["aggregated"][r] = S
        out["depth"][r], out["index"][r], out["cost"][r] = winners(S, eligible, depths[r])
    return out
