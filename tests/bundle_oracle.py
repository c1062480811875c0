"""NumPy oracle of bundle adjustment (csrc/sfm_bundle.hip, sfm_bundle_adjust): Levenberg-Marquardt over every free
camera and every point with at least two observations, with the LM rules of the PnP refinement (pnp_refine_oracle) and the
gauge rules of DESIGN.md §6h.  Two solvers of the damped normal equations give the same step: ``dense`` builds the whole
matrix (small problems), ``schur`` eliminates the points first, as the device does (about 10^5 points).  Only the
summation order differs from the device."""
import numpy as np

import pnp_refine_oracle

LAMBDA0 = 1e-3
LAMBDA_MAX = 1e16
MIN_DECREASE = 1e-12
MIN_STEP = 1e-12
OK, BAD_START, BAD_INDEX = 0, 1, 2


def residuals(poses, points, cam, pt, uv, K):
    """(e (M,), r (M, 2), Jc (M, 2, 6), Jp (M, 2, 3)) at every observation.  e is sfm_pnp_score's value in its operation
    order (+inf behind the camera); r, Jc and Jp are zero for an observation behind the camera.  Row k of Jc is
    (R X x A_k, A_k) and row k of Jp is A_k R, with A = dr/dc (the rows of pnp_refine_oracle.system)."""
    R = poses[cam, :9].reshape(-1, 3, 3)
    t = poses[cam, 9:]
    X = points[pt]
    r = np.stack([(R[:, k, 0] * X[:, 0] + R[:, k, 1] * X[:, 1]) + R[:, k, 2] * X[:, 2] for k in range(3)], axis=1)
    c = r + t
    p0 = (K[0, 0] * c[:, 0] + K[0, 1] * c[:, 1]) + K[0, 2] * c[:, 2]
    p1 = (K[1, 0] * c[:, 0] + K[1, 1] * c[:, 1]) + K[1, 2] * c[:, 2]
    front = c[:, 2] > 0.0
    c2 = np.where(front, c[:, 2], 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        du = p0 / c[:, 2] - uv[:, 0]
        dv = p1 / c[:, 2] - uv[:, 1]
        e = np.where(front, du * du + dv * dv, np.inf)
    w0, w1 = p0 / c2, p1 / c2
    res = np.where(front[:, None], np.column_stack([w0 - uv[:, 0], w1 - uv[:, 1]]), 0.0)
    ic = np.where(front, 1.0 / c2, 0.0)
    Jc = np.zeros((len(cam), 2, 6))
    Jp = np.zeros((len(cam), 2, 3))
    for row, w in ((0, w0), (1, w1)):
        A = np.column_stack([K[row, 0] * ic, K[row, 1] * ic, (K[row, 2] - w) * ic])
        Jc[:, row, :3] = np.cross(r, A)
        Jc[:, row, 3:] = A
        Jp[:, row] = np.einsum("mk,mkj->mj", A, R)
    return e, res, Jc, Jp


def cost(poses, points, cam, pt, uv, K):
    return float(np.sum(residuals(poses, points, cam, pt, uv, K)[0]))


def inverse3(A):
    """(A^-1 (n, 3, 3), ok (n,)) of symmetric 3 x 3 blocks as point_kernel computes them: the Cholesky factor L (a pivot
    <= 0 or not finite fails that block), then A^-1 = L^-T L^-1, in the device's operation order.  A block with a
    positive pivot is inverted however ill-conditioned it is: a point seen twice by one camera has V_p of rank 2 and V_p*
    of condition about 1 / lambda, and is still a moving point."""
    A = np.asarray(A, dtype=np.float64)
    n = len(A)
    L = np.zeros((n, 3, 3))
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(3):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= (s > 0.0) & np.isfinite(s)
            L[:, j, j] = np.sqrt(np.fmax(s, 0.0))
            for i in range(j + 1, 3):
                x = A[:, i, j].copy()
                for k in range(j):
                    x = x - L[:, i, k] * L[:, j, k]
                L[:, i, j] = x / L[:, j, j]
        Li = np.zeros((n, 3, 3))
        for c in range(3):
            for i in range(c, 3):
                x = np.full(n, 1.0 if i == c else 0.0)
                for k in range(c, i):
                    x = x - L[:, i, k] * Li[:, k, c]
                Li[:, i, c] = x / L[:, i, i]
        inv = np.zeros((n, 3, 3))
        for i in range(3):
            for j in range(i, 3):
                inv[:, i, j] = inv[:, j, i] = (Li[:, 0, i] * Li[:, 0, j] + Li[:, 1, i] * Li[:, 1, j]) + Li[:, 2, i] * Li[:, 2, j]
    return inv, ok


def damped_point_inverses(V, moving, lam):
    """V_p*^-1 = (V_p + lam diag V_p)^-1 of every moving point by ``inverse3`` (zero for held points), or None when one of
    them does not factor: that rejects the step."""
    V = V.copy()
    d = V[:, [0, 1, 2], [0, 1, 2]]
    V[:, [0, 1, 2], [0, 1, 2]] = d + lam * d
    Vi = np.zeros_like(V)
    if moving.any():
        inv, ok = inverse3(V[moving])
        if not ok.all():
            return None
        Vi[moving] = inv
    return Vi


class Problem:
    def __init__(self, K, poses, points, cam, pt, uv, fixed):
        self.K = np.asarray(K, dtype=np.float64).reshape(3, 3)
        self.C, self.P = len(poses), len(points)
        self.cam, self.pt, self.uv = np.asarray(cam), np.asarray(pt), np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        self.fixed = np.zeros(self.C, dtype=bool)
        self.fixed[list(fixed)] = True
        self.free = np.nonzero(~self.fixed)[0]
        self.slot = np.full(self.C, -1)
        self.slot[self.free] = np.arange(len(self.free))
        counts = np.bincount(self.pt, minlength=self.P) if self.P else np.zeros(0, dtype=int)
        self.moving = counts >= 2

    def system(self, poses, points):
        """Gauss-Newton blocks at (poses, points): U (C, 6, 6), gc (C, 6), V (P, 3, 3), gp (P, 3), W (M, 6, 3), cost."""
        e, r, Jc, Jp = residuals(poses, points, self.cam, self.pt, self.uv, self.K)
        U = np.zeros((self.C, 6, 6))
        gc = np.zeros((self.C, 6))
        V = np.zeros((self.P, 3, 3))
        gp = np.zeros((self.P, 3))
        np.add.at(U, self.cam, np.einsum("mki,mkj->mij", Jc, Jc))
        np.add.at(gc, self.cam, np.einsum("mki,mk->mi", Jc, r))
        np.add.at(V, self.pt, np.einsum("mki,mkj->mij", Jp, Jp))
        np.add.at(gp, self.pt, np.einsum("mki,mk->mi", Jp, r))
        W = np.einsum("mki,mkj->mij", Jc, Jp)
        return dict(U=U, gc=gc, V=V, gp=gp, W=W, cost=float(np.sum(e)))

    def solve_dense(self, s, lam):
        """(dc (C, 6), dX (P, 3)) of the whole damped system, or None when it does not factor or the step is not finite."""
        if damped_point_inverses(s["V"], self.moving, lam) is None:   # the device's rule: every V_p* must factor
            return None
        F, mv = len(self.free), np.nonzero(self.moving)[0]
        n = 6 * F + 3 * len(mv)
        pslot = np.full(self.P, -1)
        pslot[mv] = np.arange(len(mv))
        H = np.zeros((n, n))
        b = np.zeros(n)
        for k, c in enumerate(self.free):
            H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = s["U"][c]
            b[6 * k:6 * k + 6] = -s["gc"][c]
        o = 6 * F
        for k, p in enumerate(mv):
            H[o + 3 * k:o + 3 * k + 3, o + 3 * k:o + 3 * k + 3] = s["V"][p]
            b[o + 3 * k:o + 3 * k + 3] = -s["gp"][p]
        for m in range(len(self.cam)):
            a, q = self.slot[self.cam[m]], pslot[self.pt[m]]
            if a >= 0 and q >= 0:
                H[6 * a:6 * a + 6, o + 3 * q:o + 3 * q + 3] += s["W"][m]
                H[o + 3 * q:o + 3 * q + 3, 6 * a:6 * a + 6] += s["W"][m].T
        H[np.diag_indices(n)] += lam * np.diag(H)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(L)):
            return None
        d = np.linalg.solve(L.T, np.linalg.solve(L, b))
        dc = np.zeros((self.C, 6))
        dX = np.zeros((self.P, 3))
        dc[self.free] = d[:o].reshape(F, 6)
        dX[mv] = d[o:].reshape(len(mv), 3)
        return dc, dX

    def solve_schur(self, s, lam):
        """The same step by the Schur complement on the points (vectorised; the device's algorithm)."""
        F, C6 = len(self.free), 6 * len(self.free)
        mv = self.moving
        Vi = damped_point_inverses(s["V"], mv, lam)
        if Vi is None:
            return None
        use = mv[self.pt] & (self.slot[self.cam] >= 0)          # observations that couple a free camera to a moving point
        S = np.zeros((C6, C6))
        rhs = np.zeros(C6)
        for k, c in enumerate(self.free):
            U = s["U"][c].copy()
            U[np.diag_indices(6)] = np.diag(U) + lam * np.diag(U)
            S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = U
            rhs[6 * k:6 * k + 6] = -s["gc"][c]
        obs = np.nonzero(use)[0]
        Y = np.einsum("mij,mjk->mik", s["W"][obs], Vi[self.pt[obs]])          # W V*^-1 (6 x 3)
        a = self.slot[self.cam[obs]]
        np.add.at(rhs.reshape(F, 6) if F else rhs.reshape(0, 6), a, np.einsum("mij,mj->mi", Y, s["gp"][self.pt[obs]]))
        # pairs of observations of the same point: group by point, slot positions up to the longest group
        order = np.argsort(self.pt[obs], kind="stable")
        o_pts = self.pt[obs][order]
        starts = np.searchsorted(o_pts, o_pts, side="left")
        rank = np.arange(len(order)) - starts
        Lmax = int(rank.max()) + 1 if len(order) else 0
        grid = np.full((self.P, max(Lmax, 1)), -1)
        grid[o_pts, rank] = order
        rows = np.arange(6)[:, None] * C6 + np.arange(6)[None, :]
        flat = np.zeros(C6 * C6)
        for i in range(Lmax):
            for j in range(Lmax):
                both = (grid[:, i] >= 0) & (grid[:, j] >= 0)
                gi, gj = grid[both, i], grid[both, j]
                blk = np.einsum("mik,mjk->mij", Y[gi], s["W"][obs][gj])
                base = (6 * a[gi]) * C6 + 6 * a[gj]
                flat += np.bincount((base[:, None, None] + rows[None]).ravel(), weights=blk.ravel(), minlength=C6 * C6)
        S -= flat.reshape(C6, C6)
        try:
            L = np.linalg.cholesky(S) if C6 else np.zeros((0, 0))
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(L)):
            return None
        d = np.linalg.solve(L.T, np.linalg.solve(L, rhs)) if C6 else np.zeros(0)
        dc = np.zeros((self.C, 6))
        dc[self.free] = d.reshape(F, 6)
        # back-substitution: dX_p = V_p*^-1 (-g_p - sum_c W_cp^T dc_c)
        t = -s["gp"].copy()
        np.add.at(t, self.pt[obs], -np.einsum("mij,mi->mj", s["W"][obs], dc[self.cam[obs]]))
        dX = np.where(mv[:, None], np.einsum("pij,pj->pi", Vi, t), 0.0)
        return dc, dX


def centre(pose):
    R = pose[:9].reshape(3, 3)
    return -R.T @ pose[9:]


def adjust(K, poses, points, cam, pt, uv, fixed=(0,), max_steps=50, solver="schur"):
    """-> dict(poses, points, initial_cost, final_cost, steps, accepted, status).  The input arrays are not modified."""
    poses = np.array(poses, dtype=np.float64).reshape(-1, 12)
    points = np.array(points, dtype=np.float64).reshape(-1, 3)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = dict(poses=poses.copy(), points=points.copy(), initial_cost=np.nan, final_cost=np.nan, steps=0, accepted=0,
               status=OK)
    if len(cam) and (cam.min() < 0 or cam.max() >= len(poses) or pt.min() < 0 or pt.max() >= len(points)):
        out["status"] = BAD_INDEX
        return out
    prob = Problem(K, poses, points, cam, pt, uv, fixed)
    solve = prob.solve_schur if solver == "schur" else prob.solve_dense
    s = prob.system(poses, points)
    cur = s["cost"]
    out["initial_cost"] = out["final_cost"] = cur
    if not np.isfinite(cur):
        out["status"] = BAD_START
        return out
    anchor = None
    fixed_idx = np.nonzero(prob.fixed)[0]
    if len(fixed_idx) == 1 and len(prob.free):
        c0 = centre(poses[fixed_idx[0]])
        a = int(prob.free[0])
        anchor = (c0, a, float(np.linalg.norm(centre(poses[a]) - c0)))
    lam, steps, accepted, stop = LAMBDA0, 0, 0, max_steps <= 0
    while not stop:
        steps += 1
        step = solve(s, lam)
        ok = step is not None and np.all(np.isfinite(step[0])) and np.all(np.isfinite(step[1]))
        if not ok:
            lam *= 10.0
        else:
            dc, dX = step
            dn = np.sqrt(np.sum(dc[prob.free] ** 2) + np.sum(dX[prob.moving] ** 2))
            xn = np.sqrt(np.sum(poses[prob.free, 9:] ** 2) + np.sum(points[prob.moving] ** 2))
            if dn <= MIN_STEP * (1.0 + xn):
                stop = True
            else:
                trial = poses.copy()
                for c in prob.free:
                    R, t = pnp_refine_oracle.apply_step(poses[c, :9].reshape(3, 3), poses[c, 9:], dc[c])
                    trial[c] = np.concatenate([R.reshape(9), t])
                tpts = points + dX
                new = cost(trial, tpts, cam, pt, uv, prob.K)
                if np.isfinite(new) and new < cur:
                    stop = cur - new < MIN_DECREASE * cur
                    if anchor is not None:
                        trial, tpts = rescale(trial, tpts, prob.free, *anchor)
                    poses, points, cur = trial, tpts, new
                    lam /= 10.0
                    accepted += 1
                    s = prob.system(poses, points)
                else:
                    lam *= 10.0
        if steps >= max_steps or lam > LAMBDA_MAX:
            stop = True
    out.update(poses=poses, points=points, final_cost=cur, steps=steps, accepted=accepted)
    return out


def rescale(poses, points, free, c0, a, dist):
    """Similarity about the fixed camera's centre c0 that restores |centre(a) - c0| = dist: every point and every free
    camera's centre move by the same factor; rotations and the fixed camera stay."""
    s = dist / float(np.linalg.norm(centre(poses[a]) - c0))
    poses = poses.copy()
    for c in free:
        R = poses[c, :9].reshape(3, 3)
        cc = c0 + s * (centre(poses[c]) - c0)
        poses[c, 9:] = -(R @ cc)
    return poses, c0 + s * (points - c0)
