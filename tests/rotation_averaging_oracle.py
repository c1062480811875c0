"""Rotation averaging over a view graph: the NumPy definition that csrc/sfm_rotation_averaging.hip follows.

Inputs: C cameras; Q edges (i_q, j_q) with R_q ~ R_j R_i^T, R_c the world -> camera rotation (x_j ~ R_q x_i, the convention
of ``PairPoses.R``); weights w_q; a root; a loss with its scale a in radians; optionally initial rotations.

An edge is *active* iff w_q is finite and > 0 and all nine entries of R_q are finite.  An inactive edge is ignored
everywhere and its residual is NaN.  Parallel edges and either orientation are allowed.

The adjacency, the level rounds, the system of a step, its solve by conjugate gradients (or ``solver="dense"``), the loop over
the steps with its statuses, the costs and ``reverse_adjacency`` are tests/graph_cg_oracle.py, shared with translation
averaging; its numbering is used here.  What is rotation averaging's own:

1. A bad index gives status BAD_INDEX (every rotation and residual NaN, nothing registered).
2. Levels: in tree mode a camera takes its rotation through its tree edge: R_c = R_q R_i at the j end, R_q^T R_j at the i end,
   every entry (a0 b0 + a1 b1) + a2 b2.  R_root = I.  An unregistered camera has R = NaN.  With initial rotations the levels
   are the same and the given rotations of registered cameras are kept; the root is held.
3. Steps: per used edge D = R_j^T (R_q R_i) in this order of products, r = log D, e = (r0 r0 + r1 r1) + r2 r2,
   omega = w rho'(e), rvec = r and the cost w rho(e).  The update is R_c <- exp([R_c x_c]x) R_c (= R_c exp([x_c]x)) by
   Rodrigues.  min_converged_steps = 0.
4. log D: v = ((D21 - D12) / 2, (D02 - D20) / 2, (D10 - D01) / 2), s = sqrt((v0 v0 + v1 v1) + v2 v2), c = (((D00 + D11) + D22) - 1) / 2
   clamped to [-1, 1], theta = atan2(s, c).  c > HALF_TURN_COSINE = -0.5 (below 120 degrees): r = v (theta / s) for
   s >= TINY_SINE = 1e-10 and r = v below it.  c <= -0.5: the axis from the symmetric part (D + D^T) / 2 = c I + (1 - c) a a^T,
   which stays well conditioned up to the half turn where v vanishes: b_m = D_mm - c, k the largest of them (the first of
   equals), col_k = b_k and col_m = (D_mk + D_km) / 2 otherwise, n = sqrt((col0 col0 + col1 col1) + col2 col2), the sign
   g = -1 when (col0 v0 + col1 v1) + col2 v2 < 0 and +1 otherwise (v = s a; at the half turn itself both signs are logarithms),
   r = (g theta) (col / n).
5. Final pass: residual[q] = sqrt(e) in radians for a used edge, NaN otherwise.
"""
from __future__ import annotations

import numpy as np

from graph_cg_oracle import (BAD_INDEX, CG_FAILED, CONVERGED, LOSSES, MAX_STEPS, STATUS, adjacency, bad_index,  # noqa: F401
                             iterate, levels, rho, weight)

TINY_SINE = 1e-10
HALF_TURN_COSINE = -0.5


def mul(A, B):
    """A B, every entry (a0 b0 + a1 b1) + a2 b2."""
    return np.array([[(A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c] for c in range(3)] for r in range(3)])


def log_map(D):
    v = np.array([0.5 * (D[2, 1] - D[1, 2]), 0.5 * (D[0, 2] - D[2, 0]), 0.5 * (D[1, 0] - D[0, 1])])
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = min(1.0, max(-1.0, 0.5 * (((D[0, 0] + D[1, 1]) + D[2, 2]) - 1.0)))
    theta = np.arctan2(s, c)
    if c > HALF_TURN_COSINE:
        return v * (theta / s) if s >= TINY_SINE else v
    b = [D[0, 0] - c, D[1, 1] - c, D[2, 2] - c]
    k = 0
    if b[1] > b[k]:
        k = 1
    if b[2] > b[k]:
        k = 2
    col = np.array([b[k] if m == k else 0.5 * (D[m, k] + D[k, m]) for m in range(3)])
    n = np.sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2])
    g = -1.0 if (col[0] * v[0] + col[1] * v[1]) + col[2] * v[2] < 0.0 else 1.0
    return (g * theta) * (col / n)


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


def active_edges(relative, weights):
    w = np.asarray(weights, dtype=np.float64)
    R = np.asarray(relative, dtype=np.float64).reshape(-1, 9)
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0) & np.all(np.isfinite(R), axis=1)


def levels_and_tree(C, pairs, relative, weights, root, tree=True):
    """(level [C] (-1: unregistered), R [C,3,3] of the tree initialisation (NaN where unregistered; only with ``tree``))."""
    R = np.full((C, 3, 3), np.nan)
    R[root] = np.eye(3)

    def place(c, h, other):
        Rq = np.asarray(relative[h >> 1], dtype=np.float64).reshape(3, 3)
        R[c] = mul(Rq, R[other]) if h & 1 else mul(Rq.T, R[other])

    return levels(C, pairs, weights, active_edges(relative, weights), root, place if tree else None), R


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
    if bad_index(C, pairs):
        return out
    level, R = levels_and_tree(C, pairs, rel, w, root, tree=initial_rotations is None)
    reg = level >= 0
    if initial_rotations is not None:
        R = np.array(initial_rotations, dtype=np.float64).reshape(C, 3, 3)
        R[~reg] = np.nan
    used = active_edges(rel, w) & reg[pairs[:, 0]] & reg[pairs[:, 1]] if Q else np.zeros(0, dtype=bool)
    a = float(loss_scale)

    def edge_terms(step):
        r = edge_residuals(pairs, rel, R, used)
        om, cost = np.zeros(Q), np.zeros(Q)
        for q in np.nonzero(used)[0]:
            e = (r[q, 0] * r[q, 0] + r[q, 1] * r[q, 1]) + r[q, 2] * r[q, 2]
            om[q] = w[q] * weight(loss, a, e)
            cost[q] = w[q] * rho(loss, a, e)
        return om, r, cost

    def update(x, free):
        for c in np.nonzero(free)[0]:
            y = np.array([(R[c][k, 0] * x[c][0] + R[c][k, 1] * x[c][1]) + R[c][k, 2] * x[c][2] for k in range(3)])
            R[c] = mul(exp_map(y), R[c])

    def final():
        _, r, cost = edge_terms(None)
        e = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        return cost, dict(R=R, residual=np.where(used, np.sqrt(e), np.nan) if Q else np.zeros(0))

    out.update(iterate(C, pairs, root, level, used, edge_terms, update, final, max_steps, max_cg_iterations, cg_tolerance,
                       step_tolerance, solver=solver, reverse_adjacency=reverse_adjacency))
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
