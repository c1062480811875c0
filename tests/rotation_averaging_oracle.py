"""Rotation averaging over a view graph: the NumPy definition that csrc/sfm_rotation_averaging.hip follows.

Inputs: C cameras; Q edges (i_q, j_q) with R_q ~ R_j R_i^T, R_c the world -> camera rotation (x_j ~ R_q x_i, the convention
of ``PairPoses.R``); weights w_q; a root; a loss with its scale a in radians; optionally initial rotations.

An edge is *active* iff w_q is finite and > 0 and all nine entries of R_q are finite.  An inactive edge is ignored
everywhere and its residual is NaN.  Parallel edges and either orientation are allowed.

1. Adjacency: half-edge 2q belongs to i_q and 2q + 1 to j_q; a camera's half-edges are taken in increasing index.  An index
   outside 0..C-1 or i_q == j_q gives status BAD_INDEX (every rotation and residual NaN, nothing registered).
2. Levels: level[root] = 0; in round k = 1, 2, ... a camera without a level looks at its active half-edges whose other end
   has a level < k; if there are any it takes level k and, in tree mode, its rotation through the heaviest of them (the first
   of equals): R_c = R_q R_i at the j end, R_q^T R_j at the i end, every entry (a0 b0 + a1 b1) + a2 b2.  R_root = I.  The rounds
   end when one sets nothing.  A camera without a level is unregistered (R = NaN).  With initial rotations the levels are
   the same and the given rotations of registered cameras are kept; the root is held.
3. Steps (at most max_steps): per used edge (active, both ends registered) D = R_j^T (R_q R_i) in this order of products,
   r = log D, e = (r0 r0 + r1 r1) + r2 r2, omega = w rho'(e).  Solve sum_{q at c} omega (x_c - x_other) = sum_{q at c} s (omega r)
   (s = +1 at the j end, -1 at the i end; x_root = 0; the sums in half-edge order) for the free cameras by conjugate
   gradients with the Jacobi preconditioner d_c = sum omega from x = 0, stopping at |r_k| <= cg_tolerance |b|, at
   max_cg_iterations or at a breakdown (p.Ap <= 0: the iterate so far is the step; at k = 0, or any non-finite scalar: status
   CG_FAILED with the rotations of the last completed step).  Then R_c <- exp([R_c x_c]x) R_c (= R_c exp([x_c]x)) by
   Rodrigues, and the step counts.  CONVERGED when max_c |x_c|_inf <= step_tolerance, else MAX_STEPS after max_steps steps.
   No free camera is CONVERGED with 0 steps; max_steps = 0 with a free camera is MAX_STEPS.
4. log D: v = ((D21 - D12) / 2, (D02 - D20) / 2, (D10 - D01) / 2), s = sqrt((v0 v0 + v1 v1) + v2 v2), c = (((D00 + D11) + D22) - 1) / 2
   clamped to [-1, 1], theta = atan2(s, c).  s >= TINY_SINE = 1e-10: r = v (theta / s).  Below it: r = v when c > 0, else
   r = theta (col / |col|) with col the column of (D + I) / 2 whose diagonal entry is largest (the first of equals).
5. Final pass: residual[q] = sqrt(e) in radians for a used edge, NaN otherwise; cost = sum over the used edges of w rho(e)
   (initial_cost at the first linearisation, final_cost at the result; equal without a step).

``solver="pcg"`` is the solve above; ``solver="dense"`` replaces the CG by ``numpy.linalg.solve`` on the assembled
Laplacian (no CG counters, never CG_FAILED).  ``reverse_adjacency=True`` walks every camera's half-edges backwards in the
sums of step 3 (not in the levels): the spread between the two is what the summation order is worth.
"""
from __future__ import annotations

import numpy as np

CONVERGED, MAX_STEPS, CG_FAILED, BAD_INDEX = 0, 1, 2, 3
STATUS = ("converged", "max_steps", "cg_failed", "bad_index")
LOSSES = ("squared", "huber", "cauchy")
TINY_SINE = 1e-10


def mul(A, B):
    """A B, every entry (a0 b0 + a1 b1) + a2 b2."""
    return np.array([[(A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c] for c in range(3)] for r in range(3)])


def log_map(D):
    v = np.array([0.5 * (D[2, 1] - D[1, 2]), 0.5 * (D[0, 2] - D[2, 0]), 0.5 * (D[1, 0] - D[0, 1])])
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = min(1.0, max(-1.0, 0.5 * (((D[0, 0] + D[1, 1]) + D[2, 2]) - 1.0)))
    theta = np.arctan2(s, c)
    if s >= TINY_SINE:
        return v * (theta / s)
    if c > 0.0:
        return v
    b = [0.5 * (D[0, 0] + 1.0), 0.5 * (D[1, 1] + 1.0), 0.5 * (D[2, 2] + 1.0)]
    k = 0
    if b[1] > b[k]:
        k = 1
    if b[2] > b[k]:
        k = 2
    col = np.array([b[k] if m == k else 0.5 * D[m, k] for m in range(3)])
    n = np.sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2])
    return theta * (col / n)


def exp_map(w):
    """exp([w]x) as csrc/sfm_pnp.h's apply_step builds it."""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-6:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        s = np.sin(0.5 * th)
        A, B = np.sin(th) / th, 2.0 * s * s / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return (np.eye(3) + A * W) + B * mul(W, W)


def rho(loss, a, e):
    a2 = a * a
    if loss == "huber":
        return e if e <= a2 else (2.0 * a) * np.sqrt(e) - a2
    if loss == "cauchy":
        return a2 * np.log1p(e / a2)
    return e


def weight(loss, a, e):
    a2 = a * a
    if loss == "huber":
        return 1.0 if e <= a2 else a / np.sqrt(e)
    if loss == "cauchy":
        return 1.0 / (1.0 + e / a2)
    return 1.0


def active_edges(relative, weights):
    w = np.asarray(weights, dtype=np.float64)
    R = np.asarray(relative, dtype=np.float64).reshape(-1, 9)
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0) & np.all(np.isfinite(R), axis=1)


def adjacency(C, pairs):
    """Per camera the half-edges 2q (i end) and 2q + 1 (j end) in increasing index."""
    adj = [[] for _ in range(C)]
    for h, c in enumerate(np.asarray(pairs).reshape(-1)):
        adj[int(c)].append(h)
    return adj


def levels_and_tree(C, pairs, relative, weights, root, tree=True):
    """(level [C] (-1: unregistered), R [C,3,3] of the tree initialisation (NaN where unregistered; only with ``tree``))."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    flat = pairs.reshape(-1)
    act = active_edges(relative, weights)
    adj = adjacency(C, pairs)
    level = np.full(C, -1, dtype=np.int64)
    level[root] = 0
    R = np.full((C, 3, 3), np.nan)
    R[root] = np.eye(3)
    for k in range(1, C):
        new = []
        for c in range(C):
            if level[c] >= 0:
                continue
            best, best_w = -1, 0.0
            for h in adj[c]:
                q = h >> 1
                if not act[q]:
                    continue
                lv = level[flat[h ^ 1]]
                if lv < 0 or lv >= k:
                    continue
                if best < 0 or weights[q] > best_w:
                    best, best_w = h, weights[q]
            if best >= 0:
                new.append((c, best))
        if not new:
            break
        for c, h in new:   # after the scan: no camera of this round sees another of this round
            level[c] = k
            if tree:
                Rq, Ro = np.asarray(relative[h >> 1], dtype=np.float64).reshape(3, 3), R[flat[h ^ 1]]
                R[c] = mul(Rq, Ro) if h & 1 else mul(Rq.T, Ro)
    return level, R


def edge_residuals(pairs, relative, R, used):
    """r_q = log(R_j^T (R_q R_i)) per used edge (zeros elsewhere)."""
    r = np.zeros((len(pairs), 3))
    for q in np.nonzero(used)[0]:
        i, j = pairs[q]
        r[q] = log_map(mul(R[j].T, mul(np.asarray(relative[q], dtype=np.float64).reshape(3, 3), R[i])))
    return r


def average_rotations(num_cameras, pairs, relative_rotations, weights=None, root=0, loss="squared", loss_scale=np.radians(1.0),
                      initial_rotations=None, max_steps=50, max_cg_iterations=500, cg_tolerance=1e-6, step_tolerance=1e-8,
                      solver="pcg", reverse_adjacency=False):
    """The definition.  ``loss_scale`` in radians.  Returns a dict: R [C,3,3], registered [C] bool, level [C], residual [Q]
    (radians), steps, cg_iterations, cg_max, initial_cost, final_cost, status (an index of ``STATUS``)."""
    C = int(num_cameras)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q = len(pairs)
    rel = np.asarray(relative_rotations, dtype=np.float64).reshape(Q, 3, 3)
    w = np.ones(Q) if weights is None else np.asarray(weights, dtype=np.float64)
    out = dict(R=np.full((C, 3, 3), np.nan), registered=np.zeros(C, dtype=bool), level=np.full(C, -1), residual=np.full(Q, np.nan),
               steps=0, cg_iterations=0, cg_max=0, initial_cost=np.nan, final_cost=np.nan, status=BAD_INDEX)
    if Q and (pairs.min() < 0 or pairs.max() >= C or np.any(pairs[:, 0] == pairs[:, 1])):
        return out
    level, R = levels_and_tree(C, pairs, rel, w, root, tree=initial_rotations is None)
    reg = level >= 0
    if initial_rotations is not None:
        R = np.array(initial_rotations, dtype=np.float64).reshape(C, 3, 3)
        R[~reg] = np.nan
    used = active_edges(rel, w) & reg[pairs[:, 0]] & reg[pairs[:, 1]] if Q else np.zeros(0, dtype=bool)
    free = reg.copy()
    free[root] = False
    adj = adjacency(C, pairs)
    if reverse_adjacency:
        adj = [a[::-1] for a in adj]
    flat = pairs.reshape(-1)
    a = float(loss_scale)

    def cost_of(r):
        return float(sum(w[q] * rho(loss, a, (r[q, 0] * r[q, 0] + r[q, 1] * r[q, 1]) + r[q, 2] * r[q, 2])
                         for q in np.nonzero(used)[0]))

    def apply(om, p):
        y = np.zeros((C, 3))
        for c in np.nonzero(free)[0]:
            acc = np.zeros(3)
            for h in adj[c]:
                q = h >> 1
                if used[q]:
                    acc += om[q] * (p[c] - p[flat[h ^ 1]])
            y[c] = acc
        return y

    status, steps, cg_total, cg_max, initial_cost = MAX_STEPS, 0, 0, 0, None
    if not free.any():
        status = CONVERGED
    while status == MAX_STEPS and steps < max_steps:
        r = edge_residuals(pairs, rel, R, used)
        if initial_cost is None:
            initial_cost = cost_of(r)
        om = np.zeros(Q)
        for q in np.nonzero(used)[0]:
            om[q] = w[q] * weight(loss, a, (r[q, 0] * r[q, 0] + r[q, 1] * r[q, 1]) + r[q, 2] * r[q, 2])
        d, b = np.zeros(C), np.zeros((C, 3))
        for c in np.nonzero(free)[0]:
            for h in adj[c]:
                q = h >> 1
                if used[q]:
                    d[c] += om[q]
                    b[c] += (1.0 if h & 1 else -1.0) * (om[q] * r[q])
        if solver == "dense":
            idx = np.nonzero(free)[0]
            slot = np.full(C, -1)
            slot[idx] = np.arange(len(idx))
            L = np.zeros((len(idx), len(idx)))
            for q in np.nonzero(used)[0]:
                si, sj = slot[pairs[q, 0]], slot[pairs[q, 1]]
                for s in (si, sj):
                    if s >= 0:
                        L[s, s] += om[q]
                if si >= 0 and sj >= 0:
                    L[si, sj] -= om[q]
                    L[sj, si] -= om[q]
            x = np.zeros((C, 3))
            x[idx] = np.linalg.solve(L, b[idx])
        else:
            inv_d = np.where(free, 1.0, 0.0) / np.where(free, d, 1.0)
            x = np.zeros((C, 3))
            res = b.copy()
            z = res * inv_d[:, None]
            p = z.copy()
            rz, bb = float(np.sum(res * z)), float(np.sum(b * b))
            tol2 = cg_tolerance * cg_tolerance * bb
            failed = not (np.isfinite(rz) and np.isfinite(bb))
            k = 0
            done = failed or bb <= tol2
            while not done:
                Ap = apply(om, p)
                pq = float(np.sum(p * Ap))
                with np.errstate(divide="ignore", invalid="ignore"):
                    alpha = np.float64(rz) / np.float64(pq)
                if not (pq > 0.0) or not np.isfinite(pq) or not np.isfinite(alpha):
                    failed = k == 0 or not np.isfinite(pq) or not np.isfinite(alpha)
                    break
                x = x + alpha * p
                res = res - alpha * Ap
                z = res * inv_d[:, None]
                rz_new, rr = float(np.sum(res * z)), float(np.sum(res * res))
                k += 1
                if not (np.isfinite(rz_new) and np.isfinite(rr)):
                    failed = True
                    break
                done = rr <= tol2 or k == max_cg_iterations
                if not done:
                    p = z + (rz_new / rz) * p
                rz = rz_new
            if failed:
                status = CG_FAILED
                break
            cg_total += k
            cg_max = max(cg_max, k)
        for c in np.nonzero(free)[0]:
            y = np.array([(R[c][k, 0] * x[c][0] + R[c][k, 1] * x[c][1]) + R[c][k, 2] * x[c][2] for k in range(3)])
            R[c] = mul(exp_map(y), R[c])
        steps += 1
        if np.max(np.abs(x[free])) <= step_tolerance:
            status = CONVERGED
    r = edge_residuals(pairs, rel, R, used)
    final_cost = cost_of(r)
    residual = np.where(used, np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]), np.nan) if Q else np.zeros(0)
    out.update(R=R, registered=reg, level=level, residual=residual, steps=steps, cg_iterations=cg_total, cg_max=cg_max,
               initial_cost=final_cost if initial_cost is None else initial_cost, final_cost=final_cost, status=status)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Synthetic graphs
# ---------------------------------------------------------------------------------------------------------------------------
def rotation_from_vector(v):
    return exp_map(np.asarray(v, dtype=np.float64))


def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return rotation_from_vector(axis * rng.uniform(0.0, max_angle))


def angle_between(Ra, Rb):
    """Angle in radians of Ra Rb^T."""
    return float(np.linalg.norm(log_map(Ra @ Rb.T)))


def make_graph(cameras, chords, seed, noise_deg=0.5, outlier_fraction=0.0, ring=True, max_angle=np.pi):
    """True rotations up to ``max_angle`` from the identity (so up to ~180 degrees apart), a ring (or a chain) plus
    ``chords`` random chords, random edge orientation, Gaussian rotation noise of ``noise_deg`` per axis, and a fraction of
    the chords replaced by random rotations (the ring stays clean, so every camera keeps a clean path).  Returns a dict:
    R_true [C,3,3] with R_true[0] = I, pairs [Q,2], relative [Q,3,3], outlier [Q] bool."""
    rng = np.random.default_rng(seed)
    R_true = np.array([np.eye(3)] + [random_rotation(rng, max_angle) for _ in range(cameras - 1)])
    edges = [(c, c + 1) for c in range(cameras - 1)] + ([(cameras - 1, 0)] if ring and cameras > 2 else [])
    while len(edges) < (cameras if ring and cameras > 2 else cameras - 1) + chords:
        i, j = (int(v) for v in rng.integers(0, cameras, size=2))
        if i != j:
            edges.append((i, j))
    base = len(edges) - chords
    outlier = np.zeros(len(edges), dtype=bool)
    n_out = int(round(outlier_fraction * len(edges)))
    if n_out:
        outlier[base + rng.choice(chords, size=n_out, replace=False)] = True
    pairs, rel = [], []
    for q, (i, j) in enumerate(edges):
        if rng.random() < 0.5:
            i, j = j, i
        Rq = random_rotation(rng) if outlier[q] else \
            rotation_from_vector(rng.normal(size=3) * np.radians(noise_deg)) @ R_true[j] @ R_true[i].T
        pairs.append((i, j))
        rel.append(Rq)
    return dict(R_true=R_true, pairs=np.array(pairs, dtype=np.int64), relative=np.array(rel), outlier=outlier)


def max_error_deg(R, R_true, registered=None):
    """Largest angle in degrees between R[c] and R_true[c] R_true[root]^T-style truth already in the result's gauge."""
    idx = range(len(R)) if registered is None else np.nonzero(registered)[0]
    return float(np.degrees(max(angle_between(R[c], R_true[c]) for c in idx)))


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_rotation_averaging.py (shared with the host test, which measures the oracle's own spread on them)
# ---------------------------------------------------------------------------------------------------------------------------
def noisy_edges(R_true, edges, rng, noise_deg=0.5):
    """pairs and relative rotations of ``edges`` (oriented as given) under ``R_true`` with Gaussian rotation noise."""
    rel = [rotation_from_vector(rng.normal(size=3) * np.radians(noise_deg)) @ R_true[j] @ R_true[i].T for i, j in edges]
    return np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(rel).reshape(-1, 3, 3)


def case_chain(cameras=300, seed=3):
    """A chain 0 - 1 - ... with alternating edge orientation: cameras - 1 level rounds, a tree (every residual can reach 0)."""
    rng = np.random.default_rng(seed)
    R_true = np.array([np.eye(3)] + [random_rotation(rng) for _ in range(cameras - 1)])
    edges = [(c, c + 1) if c % 2 == 0 else (c + 1, c) for c in range(cameras - 1)]
    pairs, rel = noisy_edges(R_true, edges, rng)
    return dict(C=cameras, pairs=pairs, relative=rel, weights=np.ones(len(pairs)), root=0)


def case_hub(ring=700, duplicates=50, seed=4):
    """Camera 0 joined to every camera of a ring 1 .. ring (degree ring + duplicates: longer than a wave and a block), the first
    ``duplicates`` spokes twice (parallel edges, one of them reversed).  The root is on the ring."""
    rng = np.random.default_rng(seed)
    C = ring + 1
    R_true = np.array([np.eye(3)] + [random_rotation(rng) for _ in range(ring)])
    edges = [(1 + c, 1 + (c + 1) % ring) for c in range(ring)] + [(0, 1 + c) if c % 3 else (1 + c, 0) for c in range(ring)]
    edges += [(1 + c, 0) if c % 3 else (0, 1 + c) for c in range(duplicates)]
    pairs, rel = noisy_edges(R_true, edges, rng)
    return dict(C=C, pairs=pairs, relative=rel, weights=rng.uniform(0.5, 2.0, size=len(pairs)), root=5, R_true=R_true)


def case_ring(cameras=1100, chords=2200, seed=5):
    """More free cameras than the one-workgroup kernels have threads: a ring with random chords."""
    g = make_graph(cameras, chords, seed, noise_deg=0.5)
    return dict(C=cameras, pairs=g["pairs"], relative=g["relative"], weights=np.ones(len(g["pairs"])), root=0, R_true=g["R_true"])


def case_losses(seed=1):
    """24 cameras, 104 edges, 20 % of them (all chords) random rotations."""
    g = make_graph(24, 80, seed, noise_deg=0.5, outlier_fraction=0.2)
    return dict(C=24, pairs=g["pairs"], relative=g["relative"], weights=np.ones(104), root=0, R_true=g["R_true"],
                outlier=g["outlier"])


def max_rotation_difference(Ra, Rb, registered=None):
    """Largest angle in radians between corresponding rotations (over the registered cameras)."""
    idx = range(len(Ra)) if registered is None else np.nonzero(registered)[0]
    return max(angle_between(Ra[c], Rb[c]) for c in idx)
