"""Translation averaging over a view graph: the NumPy definition that csrc/sfm_translation_averaging.hip follows.

Inputs: C cameras; Q edges (i_q, j_q), either orientation, parallel edges allowed; per edge a unit world direction
v_q ~ c_j - c_i (c the camera centres) or, with global rotations R_c (world -> camera), the pair's t_q of x_j ~ R_q x_i + t_q;
weights w_q; a root; a loss of csrc/sfm_loss.h whose scale a is a sine; optionally initial positions.

0. World directions from (R, t): u_k = (R_j[0,k] t0 + R_j[1,k] t1) + R_j[2,k] t2, n = sqrt((t0 t0 + t1 t1) + t2 t2), v = -(u / n).
   An edge is *active* iff w_q is finite and > 0 and v_q is finite (with rotations: t_q and the nine entries of R_j are finite
   and n > 0).  An inactive edge is ignored everywhere; its residual and scale are NaN.
1. Adjacency, the levels, the system of a step and its solve, the loop over the steps with its statuses and the costs are
   tests/graph_cg_oracle.py, shared with rotation averaging.  A bad index gives status BAD_INDEX (every position, residual and
   scale NaN, nothing registered).  In tree mode c_root = 0 and a camera takes c_other + v_q through its tree edge at the j
   end, c_other - v_q at the i end: the unit of the result is one tree baseline.  With initial positions the registered
   cameras keep theirs and the root is held.
2. Steps, per used edge: D = c_j - c_i, n2 = (D0 D0 + D1 D1) + D2 D2, dv = (D0 v0 + D1 v1) + D2 v2, the scale
   d = max(dv, 0) / n2 (0 when n2 = 0; 1 in the first warmup_steps steps), r = v - d D, e = (r0 r0 + r1 r1) + r2 r2; the edge
   terms are omega = (w rho'(e)) (d d), rvec = r / d (0 when d = 0) and the cost w rho(e).  A free camera whose every used edge
   has d = 0 has a zero row and takes a zero step.  The update is c <- c + x.  min_converged_steps = warmup_steps: a warm-up
   step does not end the call as CONVERGED.
3. Final pass, with the scale of step 2 (never the warm-up's): residual[q] = atan2(|D x v|, dv) in radians (0..pi; the cross
   product as (D1 v2 - D2 v1, D2 v0 - D0 v2, D0 v1 - D1 v0), its norm sqrt((x0 x0 + x1 x1) + x2 x2)), scale[q] = d.  The
   initial cost is taken with d = 1 when the first step is a warm-up step.

A graph of one edge from the tree start has D = v bit for bit, so n2 = dv, d = 1, r = 0 and the step is exactly zero.  The
dense solve meets a singular matrix when an interior part of the graph is cut off by zero scales.
"""
from __future__ import annotations

import numpy as np

from graph_cg_oracle import (BAD_INDEX, CG_FAILED, CONVERGED, LOSSES, MAX_STEPS, STATUS, adjacency, bad_index,  # noqa: F401
                             iterate, levels, rho, weight)


def world_directions(pairs, t, R):
    """v_q = -(R_j^T t_q) / |t_q| in the stated order of products (NaN where |t_q| = 0 or an input is not finite)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    v = np.zeros((len(pairs), 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for q, (_, j) in enumerate(pairs):
            Rj, tq = R[j], t[q]
            n = np.sqrt((tq[0] * tq[0] + tq[1] * tq[1]) + tq[2] * tq[2])
            for k in range(3):
                v[q, k] = -(((Rj[0, k] * tq[0] + Rj[1, k] * tq[1]) + Rj[2, k] * tq[2]) / n)
    return v


def active_edges(pairs, directions, weights, rotations=None):
    w = np.asarray(weights, dtype=np.float64)
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        act = np.isfinite(w) & (w > 0) & np.all(np.isfinite(d), axis=1)
        if rotations is not None:
            R = np.asarray(rotations, dtype=np.float64).reshape(-1, 9)
            j = np.asarray(pairs).reshape(-1, 2)[:, 1]
            act &= np.all(np.isfinite(R[j]), axis=1) & (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > 0)
    return act


def levels_and_tree(C, pairs, v, weights, act, root, tree=True):
    """(level [C] (-1: unregistered), c [C,3] of the tree start (NaN where unregistered; only with ``tree``))."""
    c = np.full((C, 3), np.nan)
    c[root] = 0.0

    def place(cam, h, other):
        c[cam] = c[other] + v[h >> 1] if h & 1 else c[other] - v[h >> 1]

    return levels(C, pairs, weights, act, root, place if tree else None), c


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def edge_terms(pairs, v, c, used, warm):
    """(d, r, e, dv, D) per edge (zeros where not used)."""
    Q = len(pairs)
    D = np.zeros((Q, 3))
    D[used] = c[pairs[used, 1]] - c[pairs[used, 0]]
    n2, dv = dot3(D, D), dot3(D, v)
    if warm:
        d = np.where(used, 1.0, 0.0)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(used & (n2 != 0.0), np.maximum(dv, 0.0) / np.where(n2 != 0.0, n2, 1.0), 0.0)
    r = np.where(used[:, None], v - d[:, None] * D, 0.0)
    return d, r, dot3(r, r), dv, D


def average_translations(num_cameras, pairs, directions, weights=None, root=0, loss="squared", loss_scale=np.sin(np.radians(2.0)),
                         rotations=None, initial_positions=None, warmup_steps=10, max_steps=500, max_cg_iterations=500,
                         cg_tolerance=1e-6, step_tolerance=1e-8, solver="pcg", reverse_adjacency=False):
    """The definition.  ``loss_scale`` is a sine.  With ``rotations`` [C,3,3] the directions are the pairs' t_q.  Returns a
    dict: c [C,3], registered [C] bool, level [C], residual [Q] (radians), scale [Q], steps, cg_iterations, cg_max,
    initial_cost, final_cost, status (an index of ``STATUS``), v [Q,3] (the world directions used)."""
    C = int(num_cameras)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q = len(pairs)
    dirs = np.asarray(directions, dtype=np.float64).reshape(Q, 3)
    w = np.ones(Q) if weights is None else np.asarray(weights, dtype=np.float64)
    out = dict(c=np.full((C, 3), np.nan), registered=np.zeros(C, dtype=bool), level=np.full(C, -1), residual=np.full(Q, np.nan),
               scale=np.full(Q, np.nan), steps=0, cg_iterations=0, cg_max=0, initial_cost=np.nan, final_cost=np.nan,
               status=BAD_INDEX, v=np.full((Q, 3), np.nan))
    if bad_index(C, pairs):
        return out
    act = active_edges(pairs, dirs, w, rotations) if Q else np.zeros(0, dtype=bool)
    v = dirs if rotations is None else world_directions(pairs, dirs, rotations)
    with np.errstate(invalid="ignore"):
        act = act & np.all(np.isfinite(v), axis=1)
    v = np.where(act[:, None], v, 0.0)
    level, c = levels_and_tree(C, pairs, v, w, act, root, tree=initial_positions is None)
    reg = level >= 0
    if initial_positions is not None:
        c = np.array(initial_positions, dtype=np.float64).reshape(C, 3)
        c[~reg] = np.nan
    used = act & reg[pairs[:, 0]] & reg[pairs[:, 1]] if Q else np.zeros(0, dtype=bool)
    a = float(loss_scale)

    def cost_of(e):
        cost = np.zeros(Q)
        for q in np.nonzero(used)[0]:
            cost[q] = w[q] * rho(loss, a, e[q])
        return cost

    def terms(step):
        d, r, e, _, _ = edge_terms(pairs, v, c, used, step < warmup_steps)
        om, rd = np.zeros(Q), np.zeros((Q, 3))
        for q in np.nonzero(used)[0]:
            om[q] = (w[q] * weight(loss, a, e[q])) * (d[q] * d[q])
            if d[q] != 0.0:
                rd[q] = r[q] / d[q]
        return om, rd, cost_of(e)

    def update(x, free):
        c[free] = c[free] + x[free]

    def final():
        d, r, e, dv, D = edge_terms(pairs, v, c, used, False)
        if not Q:
            return cost_of(e), dict(c=c, v=v, residual=np.zeros(0), scale=np.zeros(0))
        x = np.stack([D[:, 1] * v[:, 2] - D[:, 2] * v[:, 1], D[:, 2] * v[:, 0] - D[:, 0] * v[:, 2],
                      D[:, 0] * v[:, 1] - D[:, 1] * v[:, 0]], axis=1)
        return cost_of(e), dict(c=c, v=v, residual=np.where(used, np.arctan2(np.sqrt(dot3(x, x)), dv), np.nan),
                                scale=np.where(used, d, np.nan))

    out.update(iterate(C, pairs, root, level, used, terms, update, final, max_steps, max_cg_iterations, cg_tolerance,
                       step_tolerance, min_converged_steps=warmup_steps, solver=solver, reverse_adjacency=reverse_adjacency))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Synthetic graphs
# ---------------------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def noisy_directions(centres, edges, rng, noise_deg=0.5):
    """pairs and unit directions c_j - c_i of ``edges`` (oriented as given) with Gaussian noise of ``noise_deg`` per axis."""
    pairs = np.array(edges, dtype=np.int64).reshape(-1, 2)
    v = unit(centres[pairs[:, 1]] - centres[pairs[:, 0]])
    if noise_deg:
        v = unit(v + np.radians(noise_deg) * rng.normal(size=v.shape))
    return pairs, v


def make_graph(cameras, chords, seed, noise_deg=0.5, outlier_fraction=0.0, spread=3.0):
    """Centres N(0, spread^2) with centre 0 at the origin, a ring plus ``chords`` random chords in random orientation, noisy
    unit directions, and a fraction of the edges (all of them chords, so every camera keeps a clean path) replaced by random
    unit vectors.  Returns a dict: centres [C,3], pairs [Q,2], directions [Q,3], outlier [Q] bool."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(cameras, 3)) * spread
    centres[0] = 0.0
    edges = [(k, (k + 1) % cameras) for k in range(cameras)]
    while len(edges) < cameras + chords:
        i, j = (int(x) for x in rng.integers(0, cameras, size=2))
        if i != j:
            edges.append((i, j) if rng.random() < 0.5 else (j, i))
    pairs, v = noisy_directions(centres, edges, rng, noise_deg)
    outlier = np.zeros(len(edges), dtype=bool)
    n_out = int(round(outlier_fraction * len(edges)))
    if n_out:
        outlier[cameras + rng.choice(chords, size=n_out, replace=False)] = True
        v[outlier] = unit(rng.normal(size=(n_out, 3)))
    return dict(centres=centres, pairs=pairs, directions=v, outlier=outlier)


def align(c, truth, registered=None):
    """``c`` scaled and shifted (rotations are taken as given) onto ``truth`` in the least-squares sense."""
    idx = np.arange(len(c)) if registered is None else np.nonzero(registered)[0]
    a, b = c[idx] - c[idx].mean(axis=0), truth[idx] - truth[idx].mean(axis=0)
    s = float(np.sum(a * b) / np.sum(a * a))
    return s * (c - c[idx].mean(axis=0)) + truth[idx].mean(axis=0)


def max_position_error(c, truth, registered=None):
    """Largest distance to the truth after ``align`` (over the registered cameras)."""
    idx = np.arange(len(c)) if registered is None else np.nonzero(registered)[0]
    return float(np.max(np.linalg.norm(align(c, truth, registered)[idx] - truth[idx], axis=1)))


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_translation_averaging.py (shared with the host test, which measures the oracle's own spread on them)
# ---------------------------------------------------------------------------------------------------------------------------
def case_chain(cameras=300, seed=3):
    """A noise-free chain 0 - 1 - ... with alternating edge orientation: cameras - 1 level rounds; no interior distance is
    determined, and the tree start already has every residual 0."""
    rng = np.random.default_rng(seed)
    centres = np.cumsum(unit(rng.normal(size=(cameras, 3))), axis=0)
    centres -= centres[0]
    edges = [(k, k + 1) if k % 2 == 0 else (k + 1, k) for k in range(cameras - 1)]
    pairs, v = noisy_directions(centres, edges, rng, 0.0)
    return dict(C=cameras, pairs=pairs, directions=v, weights=np.ones(len(pairs)), root=0, centres=centres)


def case_hub(ring=700, duplicates=50, seed=4):
    """Camera 0 joined to every camera of a ring 1 .. ring (degree ring + duplicates: longer than a wave and a block), the first
    ``duplicates`` spokes twice (parallel edges, one of them reversed), and random chords that make the ring rigid.  Noisy.
    The root is on the ring."""
    rng = np.random.default_rng(seed)
    C = ring + 1
    centres = rng.normal(size=(C, 3)) * 3.0
    edges = [(1 + k, 1 + (k + 1) % ring) for k in range(ring)] + [(0, 1 + k) if k % 3 else (1 + k, 0) for k in range(ring)]
    edges += [(1 + k, 0) if k % 3 else (0, 1 + k) for k in range(duplicates)]
    pairs, v = noisy_directions(centres, edges, rng)
    return dict(C=C, pairs=pairs, directions=v, weights=rng.uniform(0.5, 2.0, size=len(pairs)), root=5, centres=centres)


def case_ring(cameras=1100, chords=2200, seed=5):
    """More free cameras than the one-workgroup kernels have threads: a noisy ring with random chords."""
    g = make_graph(cameras, chords, seed, noise_deg=0.5)
    return dict(C=cameras, pairs=g["pairs"], directions=g["directions"], weights=np.ones(len(g["pairs"])), root=0,
                centres=g["centres"])


LOSSES_SEED = 1


def case_losses(seed=LOSSES_SEED):
    """24 cameras, 104 edges, 0.5 degrees of noise, 10 % of the edges (all chords) random directions."""
    g = make_graph(24, 80, seed, noise_deg=0.5, outlier_fraction=0.1)
    return dict(C=24, pairs=g["pairs"], directions=g["directions"], weights=np.ones(104), root=0, centres=g["centres"],
                outlier=g["outlier"])


def case_reversed_edge(seed=6, cameras=12, chords=40):
    """A clean, triangle-rich graph with one chord reversed (v -> -v), and the index of that edge."""
    g = make_graph(cameras, chords, seed, noise_deg=0.0)
    q = cameras + 3
    v = g["directions"].copy()
    v[q] = -v[q]
    return dict(C=cameras, pairs=g["pairs"], directions=v, weights=np.ones(len(v)), root=0, centres=g["centres"]), q


def case_reversed_camera(seed=7, cameras=12, chords=40, camera=4):
    """The same kind of graph with every edge at ``camera`` reversed, started next to the truth: all that camera's scales are
    0, its row of the system is zero and it keeps its initial position.  Returns the case (with ``initial``), the camera and
    the mask of its edges."""
    g = make_graph(cameras, chords, seed, noise_deg=0.0)
    at = np.any(g["pairs"] == camera, axis=1)
    v = g["directions"].copy()
    v[at] = -v[at]
    initial = g["centres"] + 0.01 * np.random.default_rng(seed + 100).normal(size=(cameras, 3))
    initial[0] = 0.0
    return dict(C=cameras, pairs=g["pairs"], directions=v, weights=np.ones(len(v)), root=0, centres=g["centres"],
                initial=initial), camera, at


def case_registration(seed=8):
    """Directions from (R, t): the component of the root 3 = {0, 3, 4, 5}, another component {1, 2}, camera 6 only through a
    weight 0, camera 7 only through a NaN t, camera 8 only through t = 0, camera 9 only through an edge that ends (j) at its own
    NaN rotation.  The t are not unit.  Returns a dict with t [Q,3] and R [C,3,3] beside the usual entries."""
    from rotation_averaging_oracle import random_rotation

    rng = np.random.default_rng(seed)
    C = 10
    R = np.array([random_rotation(rng) for _ in range(C)])
    centres = rng.normal(size=(C, 3)) * 3.0
    edges = [(3, 4), (5, 4), (0, 5), (3, 0), (1, 2), (2, 1), (6, 3), (4, 7), (8, 0), (5, 9), (4, 0)]
    pairs = np.array(edges, dtype=np.int64)
    t = np.array([R[j] @ (centres[i] - centres[j]) for i, j in edges])   # |t| is the baseline: the device normalises
    w = np.array([1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.5])
    t[7, 1] = np.nan
    t[8] = 0.0
    R[9] = np.nan
    return dict(C=C, pairs=pairs, t=t, R=R, weights=w, root=3, centres=centres,
                registered=[True, False, False, True, True, True, False, False, False, False],
                level=[1, -1, -1, 0, 1, 2, -1, -1, -1, -1], used=[True] * 4 + [False] * 6 + [True])


# Both sides of a comparison at a fixed step count: neither stops early, and a CG iteration more or less cannot show
FIXED = dict(step_tolerance=1e-300, cg_tolerance=1e-12)
HUBER_SCALE = float(np.sin(np.radians(2.0)))


def comparison_cases():
    """(name, case, options) of every run that tests/test_gpu_translation_averaging.py compares with the oracle at a fixed
    step count; tests/test_translation_averaging_host.py measures the oracle's own spread on the same runs."""
    yield "hub", case_hub(), dict(max_steps=4, warmup_steps=2)
    yield "ring", case_ring(), dict(max_steps=4, warmup_steps=2)
    yield "losses squared", case_losses(), dict(max_steps=20, warmup_steps=5)
    yield "losses huber", case_losses(), dict(loss="huber", loss_scale=HUBER_SCALE, max_steps=20, warmup_steps=5)
    yield "reversed edge", case_reversed_edge()[0], dict(max_steps=30, warmup_steps=0)
    rc = case_reversed_camera()[0]
    yield "reversed camera", rc, dict(max_steps=10, warmup_steps=0, initial_positions=rc["initial"])
    reg = case_registration()
    yield "registration", reg, dict(max_steps=10, warmup_steps=3)


def run_case(case, **options):
    """The oracle on a case dict (``t`` and ``R`` instead of ``directions``: directions from the rotations)."""
    if "t" in case:
        return average_translations(case["C"], case["pairs"], case["t"], case["weights"], root=case["root"], rotations=case["R"],
                                    **options)
    return average_translations(case["C"], case["pairs"], case["directions"], case["weights"], root=case["root"], **options)


def spread(a, b):
    """The largest difference of two oracle results in positions, residuals and scales."""
    used = ~np.isnan(a["residual"])
    assert np.array_equal(used, ~np.isnan(b["residual"])) and np.array_equal(a["registered"], b["registered"])
    reg = a["registered"]
    return max(float(np.max(np.abs(a["c"][reg] - b["c"][reg]))), float(np.max(np.abs(a["residual"][used] - b["residual"][used]))),
               float(np.max(np.abs(a["scale"][used] - b["scale"][used]))))
