"""The NumPy definition of the semi-global smoothing of a plane-sweep cost volume, written from the definition and
not from csrc/sfm_sgm.hip.  Every step is an elementwise float64 ``+ - * /`` or ``min`` in the order the definition states, so
the device result is compared with it as bytes (``plane_sweep_oracle.same_bytes``).  Vectorised over the hypotheses and over the
pixels across a direction; an explicit loop along it.  Every term of a ``min`` is finite, so its order does not matter."""
import numpy as np

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


def winners(S, eligible, z):
    """-> (depth, index int32, cost) [H, W] of one reference: the eligible hypothesis of lowest S, ties to the lower index, and the
    parabola step of the plane sweep in inverse depth, with S in place of the cost; both neighbours must be eligible."""
    D, H, W = S.shape
    value = np.where(eligible, S, np.nan)
    best, best_cost = np.full((H, W), -1, dtype=np.int32), np.full((H, W), np.nan)
    for d in range(D):
        with np.errstate(all="ignore"):
            better = eligible[d] & ((best < 0) | (value[d] < best_cost))
        best[better] = d
        best_cost[better] = value[d][better]
    has = best >= 0
    at = np.where(has, best, 0)
    with np.errstate(all="ignore"):
        zi = z[at]
        depth = np.where(has, zi, np.nan)
        inner = has & (best > 0) & (best < D - 1)
        before = np.take_along_axis(value, np.clip(at - 1, 0, D - 1)[None], axis=0)[0]
        after = np.take_along_axis(value, np.clip(at + 1, 0, D - 1)[None], axis=0)[0]
        den = (before - best_cost) + (after - best_cost)
        take = inner & np.isfinite(before) & np.isfinite(after) & (den > 0.0)
        o = 0.5 * (before - after) / den
        zj = z[np.clip(np.where(o > 0.0, at + 1, at - 1), 0, D - 1)]
        q = 1.0 / zi + np.abs(o) * (1.0 / zj - 1.0 / zi)
        refined = 1.0 / q
    return np.where(take, refined, depth), best, best_cost


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
