"""What the NumPy definitions of the solvers over a view graph share (tests/rotation_averaging_oracle.py, DESIGN.md §6t, and
tests/translation_averaging_oracle.py, §6u), operation by operation what csrc/sfm_graph_cg.h is on the device: the statuses, the
losses, the adjacency, the level rounds, the weighted graph Laplacian system, its dense solve, the conjugate gradients and
the loop over the steps.

1. Adjacency: half-edge 2q belongs to i_q and 2q + 1 to j_q; a camera's half-edges are taken in increasing index.  An index
   outside 0..C-1 or i_q == j_q is a bad index.
2. Levels: level[root] = 0; in round k = 1, 2, ... a camera without a level looks at its active half-edges whose other end
   has a level < k; if there are any it takes level k and is placed through the heaviest of them (the first of equals).
   The rounds end when one sets nothing.  A camera without a level is unregistered.
3. A step: the solver's edge terms give per used edge (active, both ends registered) a weight omega and a 3-vector rvec.
   Solve sum_{q at c} omega (x_c - x_other) = sum_{q at c} s (omega rvec) (s = +1 at the j end, -1 at the i end; x_root = 0;
   the sums in half-edge order) for the free cameras by conjugate gradients with the Jacobi preconditioner d_c = sum omega
   (a free camera with d_c = 0 gets d_c = 1, and with its zero right-hand side a zero step) from x = 0, stopping at
   |r_k| <= cg_tolerance |b|, at max_cg_iterations or at a breakdown (p.Ap <= 0: the iterate so far is the step; at k = 0, or
   any non-finite scalar: status CG_FAILED with the state of the last completed step).  Then the solver's update, and the
   step counts.  CONVERGED when max_c |x_c|_inf <= step_tolerance after a step with index >= min_converged_steps, else
   MAX_STEPS after max_steps steps.  No free camera is CONVERGED with 0 steps; max_steps = 0 with a free camera is MAX_STEPS.
4. The cost is the sum over the used edges, in increasing index, of the solver's per-edge cost: initial_cost at the first
   linearisation, final_cost at the result; equal without a step.

``solver="pcg"`` is the solve above; ``solver="dense"`` replaces the CG by ``numpy.linalg.solve`` on the assembled Laplacian
(a zero diagonal set to 1; least squares for a singular matrix; no CG counters, never CG_FAILED).  ``reverse_adjacency=True``
walks every camera's half-edges backwards in the sums of step 3 (not in the levels): the spread between the two is what the
summation order is worth.
"""
from __future__ import annotations

import numpy as np

CONVERGED, MAX_STEPS, CG_FAILED, BAD_INDEX = 0, 1, 2, 3
STATUS = ("converged", "max_steps", "cg_failed", "bad_index")
LOSSES = ("squared", "huber", "cauchy")


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


def bad_index(C, pairs):
    return bool(len(pairs)) and bool(pairs.min() < 0 or pairs.max() >= C or np.any(pairs[:, 0] == pairs[:, 1]))


def adjacency(C, pairs):
    """Per camera the half-edges 2q (i end) and 2q + 1 (j end) in increasing index."""
    adj = [[] for _ in range(C)]
    for h, c in enumerate(np.asarray(pairs).reshape(-1)):
        adj[int(c)].append(h)
    return adj


def levels(C, pairs, weights, act, root, place=None):
    """level [C] (-1: unregistered).  ``place(c, h, other)`` starts camera c through its half-edge h from the camera at the
    other end, when it takes its level."""
    flat = np.asarray(pairs).reshape(-1)
    adj = adjacency(C, pairs)
    level = np.full(C, -1, dtype=np.int64)
    level[root] = 0
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
            if place is not None:
                place(c, h, flat[h ^ 1])
    return level


def solve_dense(C, pairs, used, free, om, b):
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
    for s in range(len(idx)):
        if L[s, s] == 0.0:
            L[s, s] = 1.0
    x = np.zeros((C, 3))
    try:
        x[idx] = np.linalg.solve(L, b[idx])
    except np.linalg.LinAlgError:
        x[idx] = np.linalg.lstsq(L, b[idx], rcond=None)[0]
    return x


def solve_cg(apply, free, d, b, max_cg_iterations, cg_tolerance):
    """(x, iterations, failed) of the conjugate gradients on ``apply`` (p -> A p)."""
    inv_d = np.where(free, 1.0, 0.0) / np.where(free, d, 1.0)
    x = np.zeros_like(b)
    res = b.copy()
    z = res * inv_d[:, None]
    p = z.copy()
    rz, bb = float(np.sum(res * z)), float(np.sum(b * b))
    tol2 = cg_tolerance * cg_tolerance * bb
    failed = not (np.isfinite(rz) and np.isfinite(bb))
    k = 0
    done = failed or bb <= tol2
    while not done:
        Ap = apply(p)
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
    return x, k, failed


def iterate(C, pairs, root, level, used, edge_terms, update, final, max_steps, max_cg_iterations, cg_tolerance, step_tolerance,
            min_converged_steps=0, solver="pcg", reverse_adjacency=False):
    """The steps of a solver.  ``edge_terms(step)`` -> (omega [Q], rvec [Q,3], cost [Q]) of the linearisation of step ``step``
    (zeros where an edge is not used); ``update(x, free)`` moves the solver's state by the step x [C,3]; ``final()`` -> (cost
    [Q] at the result, a dict of the solver's own per-edge results).  Returns that dict with registered, level, steps,
    cg_iterations, cg_max, cg_at_limit (``solver="pcg"`` and every solve of at least one step ended at ``max_cg_iterations``),
    initial_cost, final_cost and status (an index of ``STATUS``)."""
    reg = level >= 0
    free = reg.copy()
    free[root] = False
    adj = adjacency(C, pairs)
    if reverse_adjacency:
        adj = [a[::-1] for a in adj]
    flat = pairs.reshape(-1)

    def total(cost):
        return float(sum(cost[q] for q in np.nonzero(used)[0]))

    status, steps, cg_total, cg_max, initial_cost = MAX_STEPS, 0, 0, 0, None
    at_limit = solver == "pcg"   # every solve ended at max_cg_iterations: the counters do not depend on rounding
    if not free.any():
        status = CONVERGED
    while status == MAX_STEPS and steps < max_steps:
        om, rvec, cost = edge_terms(steps)
        if initial_cost is None:
            initial_cost = total(cost)
        d, b = np.zeros(C), np.zeros((C, 3))
        for c in np.nonzero(free)[0]:
            for h in adj[c]:
                q = h >> 1
                if used[q]:
                    d[c] += om[q]
                    b[c] += (1.0 if h & 1 else -1.0) * (om[q] * rvec[q])
            if d[c] == 0.0:
                d[c] = 1.0
        if solver == "dense":
            x = solve_dense(C, pairs, used, free, om, b)
        else:
            def apply(p):
                y = np.zeros((C, 3))
                for c in np.nonzero(free)[0]:
                    acc = np.zeros(3)
                    for h in adj[c]:
                        q = h >> 1
                        if used[q]:
                            acc += om[q] * (p[c] - p[flat[h ^ 1]])
                    y[c] = acc
                return y

            x, k, failed = solve_cg(apply, free, d, b, max_cg_iterations, cg_tolerance)
            if failed:
                status = CG_FAILED
                break
            cg_total += k
            cg_max = max(cg_max, k)
            at_limit = at_limit and k == max_cg_iterations
        update(x, free)
        steps += 1
        if np.max(np.abs(x[free])) <= step_tolerance and steps > min_converged_steps:
            status = CONVERGED
    cost, result = final()
    final_cost = total(cost)
    result.update(registered=reg, level=level, steps=steps, cg_iterations=cg_total, cg_max=cg_max,
                  cg_at_limit=at_limit and steps > 0 and status != CG_FAILED,
                  initial_cost=final_cost if initial_cost is None else initial_cost, final_cost=final_cost, status=status)
    return result
