"""The definitions of tests/graph_cg_oracle.py, tests/rotation_averaging_oracle.py and tests/translation_averaging_oracle.py once
more, in vectorised NumPy, for graphs of 10^5 cameras and more where the per-camera loops of those three take minutes
(tests/test_gpu_averaging_edges.py).  The same numbering, statuses, stop rules and counters; what differs is how it is computed:

* Levels: a breadth-first frontier.  In round k a camera without a level that has an active half-edge to the frontier of
  round k - 1 takes level k (a levelled neighbour of a camera still without a level can only be on that frontier), through the
  heaviest such half-edge, the first of equals in its own adjacency order, that is the one with the smallest half-edge index.
* Per-camera sums: ``numpy.bincount`` over the used half-edges of the free cameras sorted by (camera, half-edge), which adds
  every camera's terms in increasing half-edge index from 0.0 as the loops do (``reverse_adjacency``: decreasing index).  With
  ``dtype=numpy.longdouble`` (which bincount does not take) ``numpy.add.reduceat`` over the same order.
* Edge terms, updates and final passes: the operations of the loop oracles on whole arrays.
* The dot products of the conjugate gradients are ``numpy.sum`` as there; the cost is ``numpy.sum`` over the used edges.

``dtype`` is the number format of the system, the conjugate gradients and their scalars (the edge terms stay float64);
``cg_stop_early=1`` returns the iterate before the last one of every solve with unchanged counters.  The two and
``reverse_adjacency`` exist to measure this oracle's own spread.  tests/test_graph_cg_vector_oracle_host.py compares every
result with the loop oracles'.
"""
from __future__ import annotations

import numpy as np

from graph_cg_oracle import BAD_INDEX, CG_FAILED, CONVERGED, MAX_STEPS, STATUS, bad_index  # noqa: F401
from rotation_averaging_oracle import HALF_TURN_COSINE, TINY_SINE


# ---------------------------------------------------------------------------------------------------------------------------
# What both solvers share
# ---------------------------------------------------------------------------------------------------------------------------
def rho(loss, a, e):
    a2 = a * a
    with np.errstate(invalid="ignore", divide="ignore"):
        if loss == "huber":
            return np.where(e <= a2, e, (2.0 * a) * np.sqrt(e) - a2)
        if loss == "cauchy":
            return a2 * np.log1p(e / a2)
    return e


def weight(loss, a, e):
    a2 = a * a
    with np.errstate(invalid="ignore", divide="ignore"):
        if loss == "huber":
            return np.where(e <= a2, 1.0, a / np.sqrt(e))
        if loss == "cauchy":
            return 1.0 / (1.0 + e / a2)
    return np.ones_like(e)


def levels(C, pairs, weights, act, root, place=None):
    """level [C] (-1: unregistered).  ``place(cams, halves, others)`` starts the cameras of one round through their half-edges
    from the cameras at the other ends."""
    flat = np.asarray(pairs, dtype=np.int64).reshape(-1)
    H = len(flat)
    order = np.argsort(flat, kind="stable")                    # the half-edges by camera, increasing index within one
    off = np.concatenate(([0], np.cumsum(np.bincount(flat, minlength=C)))) if H else np.zeros(C + 1, dtype=np.int64)
    level = np.full(C, -1, dtype=np.int64)
    level[root] = 0
    frontier = np.array([root], dtype=np.int64)
    k = 0
    while len(frontier):
        k += 1
        n = off[frontier + 1] - off[frontier]
        at = np.repeat(off[frontier] - np.concatenate(([0], np.cumsum(n)[:-1])), n) + np.arange(int(n.sum()))
        h = order[at] ^ 1                                      # the same edges seen from the other end
        cam = flat[h]
        keep = act[h >> 1] & (level[cam] < 0)
        h, cam = h[keep], cam[keep]
        if not len(h):
            break
        first = np.lexsort((h, -weights[h >> 1], cam))         # by camera, heaviest first, lowest half-edge first
        cam, h = cam[first], h[first]
        lead = np.concatenate(([True], cam[1:] != cam[:-1]))
        frontier, best = cam[lead], h[lead]
        level[frontier] = k
        if place is not None:
            place(frontier, best, flat[best ^ 1])
    return level


class Sums:
    """The used half-edges of the free cameras in the order of the per-camera sums."""

    def __init__(self, C, pairs, used, free, reverse, dtype):
        flat = pairs.reshape(-1)
        h = np.nonzero(np.repeat(used, 2) & free[flat])[0]
        h = h[np.lexsort((-h if reverse else h, flat[h]))]
        self.C, self.dtype = C, dtype
        self.cam, self.other, self.q = flat[h], flat[h ^ 1], h >> 1
        self.sign = np.where(h & 1, 1.0, -1.0)
        count = np.bincount(self.cam, minlength=C)
        self.some = count > 0
        self.start = (np.cumsum(count) - count)[self.some]

    def per_camera(self, terms):
        """[C] or [C,3]: every camera's terms added in order."""
        if terms.ndim == 2:
            return np.stack([self.per_camera(terms[:, k]) for k in range(3)], axis=1)
        if self.dtype == np.float64:
            return np.bincount(self.cam, weights=terms, minlength=self.C)
        out = np.zeros(self.C, dtype=self.dtype)
        if len(terms):
            out[self.some] = np.add.reduceat(terms.astype(self.dtype), self.start)
        return out


def solve_cg(apply, free, d, b, max_cg_iterations, cg_tolerance, cg_stop_early=0):
    """(x, iterations, failed) as tests/graph_cg_oracle.py::solve_cg, in the number format of ``b``."""
    one = b.dtype.type(1.0)
    inv_d = np.where(free, one, 0.0) / np.where(free, d, one)
    x = np.zeros_like(b)
    before = x
    res = b.copy()
    z = res * inv_d[:, None]
    p = z.copy()
    rz, bb = np.sum(res * z), np.sum(b * b)
    tol2 = b.dtype.type(cg_tolerance) * b.dtype.type(cg_tolerance) * bb
    failed = not (np.isfinite(rz) and np.isfinite(bb))
    k = 0
    done = failed or bb <= tol2
    while not done:
        Ap = apply(p)
        pq = np.sum(p * Ap)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            alpha = rz / pq
        if not (pq > 0.0) or not np.isfinite(pq) or not np.isfinite(alpha):
            failed = k == 0 or not np.isfinite(pq) or not np.isfinite(alpha)
            break
        before = x
        x = x + alpha * p
        res = res - alpha * Ap
        z = res * inv_d[:, None]
        rz_new, rr = np.sum(res * z), np.sum(res * res)
        k += 1
        if not (np.isfinite(rz_new) and np.isfinite(rr)):
            failed = True
            break
        done = rr <= tol2 or k == max_cg_iterations
        if not done:
            p = z + (rz_new / rz) * p
        rz = rz_new
    return (before if cg_stop_early else x), k, failed


def iterate(C, pairs, root, level, used, edge_terms, update, final, max_steps, max_cg_iterations, cg_tolerance, step_tolerance,
            min_converged_steps=0, reverse_adjacency=False, dtype=np.float64, cg_stop_early=0):
    """tests/graph_cg_oracle.py::iterate with ``solver="pcg"``; ``update(x, free)`` takes x as float64."""
    reg = level >= 0
    free = reg.copy()
    free[root] = False
    sums = Sums(C, pairs, used, free, reverse_adjacency, dtype)
    status, steps, cg_total, cg_max, initial_cost, at_limit = MAX_STEPS, 0, 0, 0, None, True
    if not free.any():
        status = CONVERGED
    while status == MAX_STEPS and steps < max_steps:
        om, rvec, cost = edge_terms(steps)
        if initial_cost is None:
            initial_cost = float(np.sum(cost[used]))
        with np.errstate(invalid="ignore", over="ignore"):
            omq = om[sums.q].astype(dtype)
            d = sums.per_camera(omq)
            d[free & (d == 0.0)] = 1.0
            b = sums.per_camera(sums.sign[:, None] * (om[sums.q, None] * rvec[sums.q])).astype(dtype)

            def apply(p):
                return sums.per_camera(omq[:, None] * (p[sums.cam] - p[sums.other]))

            x, k, failed = solve_cg(apply, free, d, b, max_cg_iterations, cg_tolerance, cg_stop_early)
        if failed:
            status = CG_FAILED
            break
        cg_total += k
        cg_max = max(cg_max, k)
        at_limit = at_limit and k == max_cg_iterations
        x = x.astype(np.float64)
        update(x, free)
        steps += 1
        if np.max(np.abs(x[free])) <= step_tolerance and steps > min_converged_steps:
            status = CONVERGED
    cost, result = final()
    final_cost = float(np.sum(cost[used]))
    result.update(registered=reg, level=level, rounds=int(level.max()), steps=steps, cg_iterations=cg_total, cg_max=cg_max,
                  cg_at_limit=at_limit and steps > 0 and status != CG_FAILED,
                  initial_cost=final_cost if initial_cost is None else initial_cost, final_cost=final_cost, status=status)
    return result


# ---------------------------------------------------------------------------------------------------------------------------
# Rotation averaging (tests/rotation_averaging_oracle.py)
# ---------------------------------------------------------------------------------------------------------------------------
def mul(A, B):
    """A B per matrix of two stacks [N,3,3], every entry (a0 b0 + a1 b1) + a2 b2."""
    return (A[:, :, 0, None] * B[:, None, 0, :] + A[:, :, 1, None] * B[:, None, 1, :]) + A[:, :, 2, None] * B[:, None, 2, :]


def transposed(A):
    return np.swapaxes(A, 1, 2)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def log_map(D):
    """rotation_averaging_oracle.log_map on a stack [N,3,3] -> [N,3]."""
    n_ = np.arange(len(D))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.stack([0.5 * (D[:, 2, 1] - D[:, 1, 2]), 0.5 * (D[:, 0, 2] - D[:, 2, 0]), 0.5 * (D[:, 1, 0] - D[:, 0, 1])], axis=1)
        s = np.sqrt(dot3(v, v))
        c = np.fmin(1.0, np.fmax(-1.0, 0.5 * (((D[:, 0, 0] + D[:, 1, 1]) + D[:, 2, 2]) - 1.0)))
        theta = np.arctan2(s, c)
        below = v * np.where(s >= TINY_SINE, theta / s, 1.0)[:, None]
        b = np.stack([D[:, 0, 0] - c, D[:, 1, 1] - c, D[:, 2, 2] - c], axis=1)
        k = np.where(b[:, 1] > b[:, 0], 1, 0)
        k = np.where(b[:, 2] > b[n_, k], 2, k)
        col = np.stack([np.where(k == m, b[n_, k], 0.5 * (D[n_, m, k] + D[n_, k, m])) for m in range(3)], axis=1)
        norm = np.sqrt(dot3(col, col))
        g = np.where(dot3(col, v) < 0.0, -1.0, 1.0)
        above = (g * theta)[:, None] * (col / norm[:, None])
        return np.where((c > HALF_TURN_COSINE)[:, None], below, above)


def exp_map(w):
    """rotation_averaging_oracle.exp_map on a stack [N,3] -> [N,3,3]."""
    th2 = dot3(w, w)
    th = np.sqrt(th2)
    small = th < 1e-6
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sin(0.5 * th)
        A = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
        B = np.where(small, 0.5 - th2 / 24.0, 2.0 * s * s / th2)
    W = np.zeros((len(w), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return (np.eye(3)[None] + A[:, None, None] * W) + B[:, None, None] * mul(W, W)


def average_rotations(num_cameras, pairs, relative_rotations, weights=None, root=0, loss="squared", loss_scale=np.radians(1.0),
                      initial_rotations=None, max_steps=50, max_cg_iterations=500, cg_tolerance=1e-6, step_tolerance=1e-8,
                      reverse_adjacency=False, dtype=np.float64, cg_stop_early=0):
    """rotation_averaging_oracle.average_rotations with ``solver="pcg"``; the dict also has ``rounds``, the largest level."""
    C = int(num_cameras)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q = len(pairs)
    rel = np.asarray(relative_rotations, dtype=np.float64).reshape(Q, 3, 3)
    w = np.ones(Q) if weights is None else np.asarray(weights, dtype=np.float64)
    out = dict(R=np.full((C, 3, 3), np.nan), registered=np.zeros(C, dtype=bool), level=np.full(C, -1), residual=np.full(Q, np.nan),
               rounds=0, steps=0, cg_iterations=0, cg_max=0, initial_cost=np.nan, final_cost=np.nan, status=BAD_INDEX)
    if bad_index(C, pairs):
        return out
    with np.errstate(invalid="ignore"):
        act = np.isfinite(w) & (w > 0) & np.all(np.isfinite(rel.reshape(Q, 9)), axis=1)
    R = np.full((C, 3, 3), np.nan)
    R[root] = np.eye(3)

    def place(cams, halves, others):
        Rq = rel[halves >> 1]
        R[cams] = mul(np.where((halves & 1).astype(bool)[:, None, None], Rq, transposed(Rq)), R[others])

    level = levels(C, pairs, w, act, root, place if initial_rotations is None else None)
    reg = level >= 0
    if initial_rotations is not None:
        R = np.array(initial_rotations, dtype=np.float64).reshape(C, 3, 3)
        R[~reg] = np.nan
    used = act & reg[pairs[:, 0]] & reg[pairs[:, 1]]
    uq = np.nonzero(used)[0]
    a = float(loss_scale)

    def edge_terms(step):
        r = np.zeros((Q, 3))
        r[uq] = log_map(mul(transposed(R[pairs[uq, 1]]), mul(rel[uq], R[pairs[uq, 0]])))
        e = dot3(r, r)
        om, cost = np.zeros(Q), np.zeros(Q)
        om[uq] = w[uq] * weight(loss, a, e[uq])
        cost[uq] = w[uq] * rho(loss, a, e[uq])
        return om, r, cost

    def update(x, free):
        f = np.nonzero(free)[0]
        Rf, xf = R[f], x[f]
        y = (Rf[:, :, 0] * xf[:, None, 0] + Rf[:, :, 1] * xf[:, None, 1]) + Rf[:, :, 2] * xf[:, None, 2]
        R[f] = mul(exp_map(y), Rf)

    def final():
        _, r, cost = edge_terms(None)
        with np.errstate(invalid="ignore"):
            return cost, dict(R=R, residual=np.where(used, np.sqrt(dot3(r, r)), np.nan))

    out.update(iterate(C, pairs, root, level, used, edge_terms, update, final, max_steps, max_cg_iterations, cg_tolerance,
                       step_tolerance, reverse_adjacency=reverse_adjacency, dtype=dtype, cg_stop_early=cg_stop_early))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Translation averaging (tests/translation_averaging_oracle.py), world directions given
# ---------------------------------------------------------------------------------------------------------------------------
def average_translations(num_cameras, pairs, directions, weights=None, root=0, loss="squared", loss_scale=np.sin(np.radians(2.0)),
                         initial_positions=None, warmup_steps=10, max_steps=500, max_cg_iterations=500, cg_tolerance=1e-6,
                         step_tolerance=1e-8, reverse_adjacency=False, dtype=np.float64, cg_stop_early=0):
    """translation_averaging_oracle.average_translations with ``solver="pcg"`` and without ``rotations``; the dict also has
    ``rounds``, the largest level."""
    C = int(num_cameras)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q = len(pairs)
    v = np.asarray(directions, dtype=np.float64).reshape(Q, 3)
    w = np.ones(Q) if weights is None else np.asarray(weights, dtype=np.float64)
    out = dict(c=np.full((C, 3), np.nan), registered=np.zeros(C, dtype=bool), level=np.full(C, -1), residual=np.full(Q, np.nan),
               scale=np.full(Q, np.nan), rounds=0, steps=0, cg_iterations=0, cg_max=0, initial_cost=np.nan, final_cost=np.nan,
               status=BAD_INDEX)
    if bad_index(C, pairs):
        return out
    with np.errstate(invalid="ignore"):
        act = np.isfinite(w) & (w > 0) & np.all(np.isfinite(v), axis=1)
    v = np.where(act[:, None], v, 0.0)
    c = np.full((C, 3), np.nan)
    c[root] = 0.0

    def place(cams, halves, others):
        c[cams] = np.where((halves & 1).astype(bool)[:, None], c[others] + v[halves >> 1], c[others] - v[halves >> 1])

    level = levels(C, pairs, w, act, root, place if initial_positions is None else None)
    reg = level >= 0
    if initial_positions is not None:
        c = np.array(initial_positions, dtype=np.float64).reshape(C, 3)
        c[~reg] = np.nan
    used = act & reg[pairs[:, 0]] & reg[pairs[:, 1]]
    a = float(loss_scale)

    def geometry(warm):
        D = np.zeros((Q, 3))
        D[used] = c[pairs[used, 1]] - c[pairs[used, 0]]
        n2, dv = dot3(D, D), dot3(D, v)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if warm:
                d = np.where(used, 1.0, 0.0)
            else:
                d = np.where(used & (n2 != 0.0), np.maximum(dv, 0.0) / np.where(n2 != 0.0, n2, 1.0), 0.0)
            r = np.where(used[:, None], v - d[:, None] * D, 0.0)
            return d, r, dot3(r, r), dv, D

    def terms(step):
        d, r, e, _, _ = geometry(step < warmup_steps)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            om = np.where(used, (w * weight(loss, a, e)) * (d * d), 0.0)
            rd = np.where((used & (d != 0.0))[:, None], r / np.where(d != 0.0, d, 1.0)[:, None], 0.0)
            return om, rd, np.where(used, w * rho(loss, a, e), 0.0)

    def update(x, free):
        c[free] = c[free] + x[free]

    def final():
        d, r, e, dv, D = geometry(False)
        x = np.stack([D[:, 1] * v[:, 2] - D[:, 2] * v[:, 1], D[:, 2] * v[:, 0] - D[:, 0] * v[:, 2],
                      D[:, 0] * v[:, 1] - D[:, 1] * v[:, 0]], axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            cost = np.where(used, w * rho(loss, a, e), 0.0)
            return cost, dict(c=c, residual=np.where(used, np.arctan2(np.sqrt(dot3(x, x)), dv), np.nan),
                              scale=np.where(used, d, np.nan))

    out.update(iterate(C, pairs, root, level, used, terms, update, final, max_steps, max_cg_iterations, cg_tolerance,
                       step_tolerance, min_converged_steps=warmup_steps, reverse_adjacency=reverse_adjacency, dtype=dtype,
                       cg_stop_early=cg_stop_early))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Differences between two results
# ---------------------------------------------------------------------------------------------------------------------------
def rotation_angles(Ra, Rb):
    """The angle in radians of Ra Rb^T per rotation of two stacks [N,3,3]."""
    r = log_map(mul(Ra, transposed(Rb)))
    return np.sqrt(dot3(r, r))


def rotation_spread(a, b):
    """The largest difference of two rotation results (dicts with R and residual): rotations as angles, residuals; radians."""
    reg, used = a["registered"], ~np.isnan(a["residual"])
    assert np.array_equal(reg, b["registered"]) and np.array_equal(used, ~np.isnan(b["residual"]))
    return max(float(np.max(rotation_angles(a["R"][reg], b["R"][reg]))), float(np.max(np.abs(a["residual"][used] - b["residual"][used]))))


def translation_spread(a, b):
    """The largest difference of two translation results (dicts with c, residual and scale)."""
    reg, used = a["registered"], ~np.isnan(a["residual"])
    assert np.array_equal(reg, b["registered"]) and np.array_equal(used, ~np.isnan(b["residual"]))
    return max(float(np.max(np.abs(a["c"][reg] - b["c"][reg]))), float(np.max(np.abs(a["residual"][used] - b["residual"][used]))),
               float(np.max(np.abs(a["scale"][used] - b["scale"][used]))))


# The options of the large runs of tests/test_gpu_averaging_edges.py
LARGE_LIMITS = dict(max_steps=2, step_tolerance=1e-300, cg_tolerance=1e-13, max_cg_iterations=200)
LARGE_SIZES = (4097, 65537, 263000)

# This oracle's own spread on the large cases, measured on the CPU with ``measured_spread`` (rotation: radians; translation:
# tree baselines, radians and 1 / baseline).  tests/test_gpu_averaging_edges.py takes its tolerances from it.
LARGE_SPREAD = {("rotation", 4097, "squared"): 3.11e-16, ("rotation", 4097, "huber"): 6.83e-15,
                ("rotation", 65537, "squared"): 2.10e-15, ("rotation", 65537, "huber"): 4.22e-14,
                ("rotation", 263000, "squared"): 4.60e-15, ("rotation", 263000, "huber"): 5.77e-14,
                ("translation", 4097, "squared"): 3.56e-12, ("translation", 65537, "squared"): 4.15e-11,
                ("translation", 263000, "squared"): 1.15e-10}


def large_run(solver, case, loss="squared", **knobs):
    if solver == "rotation":
        return average_rotations(case["C"], case["pairs"], case["relative"], case["weights"], root=case["root"], loss=loss,
                                 **LARGE_LIMITS, **knobs)
    return average_translations(case["C"], case["pairs"], case["directions"], case["weights"], root=case["root"], loss=loss,
                                warmup_steps=1, **LARGE_LIMITS, **knobs)


# ---------------------------------------------------------------------------------------------------------------------------
# The large graphs of tests/test_gpu_averaging_edges.py
# ---------------------------------------------------------------------------------------------------------------------------
CUT = 700   # the cameras that large_case(263 000) cuts off


def large_graph(cameras, seed, cut=0):
    """A path (c, c + 1) plus two seeded random chords per camera, every edge in random orientation, weights uniform in
    [0.5, 2]; about ten levels deep.  With ``cut`` the ``cut`` cameras before the last one, cameras - 1 - cut .. cameras - 2, are a
    component of their own (a path and chords among themselves) and the last camera closes the path of the others.  Returns
    (pairs [Q,2], weights [Q], the indices of the chords, the generator)."""
    rng = np.random.default_rng(seed)
    main = cameras - cut
    parts, chords, at = [], [], 0
    for lo, n in ((0, main), (main, cut)):
        if n < 2:
            continue
        path = np.stack([np.arange(lo, lo + n - 1), np.arange(lo + 1, lo + n)], axis=1)
        i = rng.integers(lo, lo + n, size=2 * n)
        j = (i - lo + rng.integers(1, n, size=2 * n)) % n + lo          # never i itself
        parts += [path, np.stack([i, j], axis=1)]
        chords.append(at + len(path) + np.arange(2 * n))
        at += len(path) + 2 * n
    pairs = np.concatenate(parts)
    if cut:   # the labels main - 1 and cameras - 1 change places
        a, b = pairs == main - 1, pairs == cameras - 1
        pairs[a], pairs[b] = cameras - 1, main - 1
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    return pairs.astype(np.int64), rng.uniform(0.5, 2.0, size=len(pairs)), np.concatenate(chords), rng


def large_case(solver, cameras, seed=7):
    """The case of tests/test_gpu_averaging_edges.py at ``cameras`` cameras for ``solver`` "rotation" (seeded random true
    rotations, 0.5 degrees of noise per edge) or "translation" (seeded random centres, 0.5 degrees of noise per direction).
    From 262 144 cameras on the root is the last camera, the CUT cameras before it are cut off, and six chords carry the weights
    0 and NaN."""
    big = cameras > 262144
    pairs, w, chords, rng = large_graph(cameras, seed, CUT if big else 0)
    case = dict(C=cameras, pairs=pairs, weights=w, root=cameras - 1 if big else 0)
    if big:
        off = chords[rng.choice(2 * (cameras - CUT), size=6, replace=False)]   # chords of the root's component
        w[off[:3]], w[off[3:]] = 0.0, np.nan
        case["switched_off"] = off
    Q = len(pairs)
    if solver == "rotation":
        axis = rng.normal(size=(cameras, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        truth = exp_map(axis * rng.uniform(0.0, np.pi, size=(cameras, 1)))
        noise = exp_map(rng.normal(size=(Q, 3)) * np.radians(0.5))
        case.update(relative=noise @ truth[pairs[:, 1]] @ transposed(truth[pairs[:, 0]]), truth=truth)
    else:
        centres = rng.normal(size=(cameras, 3)) * 3.0
        v = centres[pairs[:, 1]] - centres[pairs[:, 0]]
        v = v / np.linalg.norm(v, axis=1, keepdims=True) + np.radians(0.5) * rng.normal(size=(Q, 3))
        case.update(directions=v / np.linalg.norm(v, axis=1, keepdims=True), truth=centres)
    return case


def measured_spread(solver, cameras, loss="squared"):
    """The largest difference among the float64 run of ``large_case(solver, cameras)``, its ``longdouble`` run (its
    reversed-adjacency run where ``longdouble`` is not 80-bit) and a run whose every solve stops one CG iteration earlier."""
    case = large_case(solver, cameras)
    base = large_run(solver, case, loss)
    other = dict(dtype=np.longdouble) if np.finfo(np.longdouble).nmant > 52 else dict(reverse_adjacency=True)
    difference = rotation_spread if solver == "rotation" else translation_spread
    return max(difference(base, large_run(solver, case, loss, **knob)) for knob in (other, dict(cg_stop_early=1)))
