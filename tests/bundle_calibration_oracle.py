"""NumPy oracle of the calibrating dense bundle adjuster (csrc/sfm_bundle.hip, sfm_bundle_adjust_calibrated; DESIGN.md
§6ab), on top of ``bundle_oracle`` and ``bundle_robust_oracle``.

Up to three intrinsics theta = (f, cx, cy) are shared by all cameras: f = K[0,0], and a step df scales the 2 x 2 block of K
by (f + df) / f; cx = K[0,2] and cy = K[1,2] move additively, free or held together.  With w the projection,

    dw/df = ((w_0 - K02) / K00, (w_1 - K12) / K00)      dw/dcx = (1, 0)      dw/dcy = (0, 1)

are the rows of Jq, times sqrt(w) under a robust loss.  The new blocks of the normal equations are U_qq = sum Jq^T Jq and
g_q = sum Jq^T r over every observation in front of its camera, U_cq = sum Jc^T Jq per camera and W_qp = sum Jq^T Jp per
moving point.  ``dense`` factors the whole damped matrix; ``schur`` eliminates the points first, as the device does, which
leaves the reduced camera system bordered by the q free intrinsics.  Only the summation order differs from the device.

With no free intrinsic every array has a zero-sized border and ``adjust`` computes the bits of ``bundle_oracle.adjust``."""
import numpy as np

import bundle_oracle as bo
import bundle_robust_oracle as bro
import pnp_refine_oracle

NAMES = ("focal", "principal_point")


def free_indices(refine):
    """The indices in (f, cx, cy) of the free intrinsics of a collection of ``NAMES``."""
    refine = tuple(refine)
    assert all(name in NAMES for name in refine) and len(set(refine)) == len(refine), refine
    return np.array(([0] if "focal" in refine else []) + ([1, 2] if "principal_point" in refine else []), dtype=int)


def project(poses, points, cam, pt, K):
    """w (M, 2): the projection of every observation (in front of its camera)."""
    R = poses[cam, :9].reshape(-1, 3, 3)
    c = np.einsum("mij,mj->mi", R, points[pt]) + poses[cam, 9:]
    return (c[:, :2] @ K[:2, :2].T + np.outer(c[:, 2], K[:2, 2])) / c[:, 2:3]


def intrinsic_rows(r, uv, K, front):
    """Jq (M, 2, 3) from the unweighted residual r = w - uv; zero behind the camera."""
    w = r + uv
    Jq = np.zeros((len(r), 2, 3))
    Jq[:, 0, 0] = (w[:, 0] - K[0, 2]) / K[0, 0]
    Jq[:, 1, 0] = (w[:, 1] - K[1, 2]) / K[0, 0]
    Jq[:, 0, 1] = 1.0
    Jq[:, 1, 2] = 1.0
    return Jq * front[:, None, None]


def stepped(K, idx, dq):
    """K after the step dq of the free intrinsics idx, or None where the trial K00 is not finite, is zero or changes
    sign."""
    K = K.copy()
    d = np.zeros(3)
    d[idx] = dq
    if 0 in idx:
        f = K[0, 0] + d[0]
        if not np.isfinite(f) or f == 0.0 or (f < 0.0) != (K[0, 0] < 0.0):
            return None
        ratio = f / K[0, 0]
        K[0, 0] = f
        K[0, 1] *= ratio
        K[1, 0] *= ratio
        K[1, 1] *= ratio
    K[0, 2] += d[1]
    K[1, 2] += d[2]
    return K


class Problem(bro.Problem):
    def __init__(self, K, poses, points, cam, pt, uv, fixed, refine=(), loss="squared", loss_scale=1.0):
        bro.Problem.__init__(self, K, poses, points, cam, pt, uv, fixed, loss, loss_scale)
        self.K = self.K.copy()
        self.idx = free_indices(refine)

    def system(self, poses, points):
        """bundle_robust_oracle's blocks under self.K, plus Uqq (q, q), gq (q,), Ucq (C, 6, q), Wq (P, q, 3; zero for a
        held point) and, for the dense solver, Jq (M, 2, q) beside Jc and Jp (all weighted)."""
        s = bro.Problem.system(self, poses, points)
        e, r, Jc, Jp = bo.residuals(poses, points, self.cam, self.pt, self.uv, self.K)
        sw = np.sqrt(s["w"])
        Jq = intrinsic_rows(r, self.uv, self.K, np.isfinite(e))[:, :, self.idx] * sw[:, None, None]
        r, Jc, Jp = r * sw[:, None], Jc * sw[:, None, None], Jp * sw[:, None, None]
        q = len(self.idx)
        Ucq = np.zeros((self.C, 6, q))
        Wq = np.zeros((self.P, q, 3))
        np.add.at(Ucq, self.cam, np.einsum("mki,mkj->mij", Jc, Jq))
        np.add.at(Wq, self.pt, np.einsum("mki,mkj->mij", Jq, Jp))
        Wq[~self.moving] = 0.0
        s.update(Uqq=np.einsum("mki,mkj->ij", Jq, Jq), gq=np.einsum("mki,mk->i", Jq, r), Ucq=Ucq, Wq=Wq)
        return s

    def solve_dense(self, s, lam):
        """(dc (C, 6), dX (P, 3), dq (q,)) of the whole damped system ordered cameras | intrinsics | points, or None."""
        if bo.damped_point_inverses(s["V"], self.moving, lam) is None:
            return None
        F, q, mv = len(self.free), len(self.idx), np.nonzero(self.moving)[0]
        o, n = 6 * F + q, 6 * F + q + 3 * len(mv)
        pslot = np.full(self.P, -1)
        pslot[mv] = np.arange(len(mv))
        H = np.zeros((n, n))
        b = np.zeros(n)
        for k, c in enumerate(self.free):
            H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = s["U"][c]
            H[6 * k:6 * k + 6, 6 * F:o] = s["Ucq"][c]
            H[6 * F:o, 6 * k:6 * k + 6] = s["Ucq"][c].T
            b[6 * k:6 * k + 6] = -s["gc"][c]
        H[6 * F:o, 6 * F:o] = s["Uqq"]
        b[6 * F:o] = -s["gq"]
        for k, p in enumerate(mv):
            H[o + 3 * k:o + 3 * k + 3, o + 3 * k:o + 3 * k + 3] = s["V"][p]
            H[6 * F:o, o + 3 * k:o + 3 * k + 3] = s["Wq"][p]
            H[o + 3 * k:o + 3 * k + 3, 6 * F:o] = s["Wq"][p].T
            b[o + 3 * k:o + 3 * k + 3] = -s["gp"][p]
        for m in range(len(self.cam)):
            a, k = self.slot[self.cam[m]], pslot[self.pt[m]]
            if a >= 0 and k >= 0:
                H[6 * a:6 * a + 6, o + 3 * k:o + 3 * k + 3] += s["W"][m]
                H[o + 3 * k:o + 3 * k + 3, 6 * a:6 * a + 6] += s["W"][m].T
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
        dc[self.free] = d[:6 * F].reshape(F, 6)
        dX[mv] = d[o:].reshape(len(mv), 3)
        return dc, dX, d[6 * F:o]

    def solve_schur(self, s, lam):
        """The same step by the Schur complement on the points: the reduced camera system of
        ``bundle_oracle.Problem.solve_schur`` (its statements, in its order), bordered by
        S_aq = U_aq - sum_{i in a} W_i V_p*^-1 W_qp^T, S_qq = U_qq* - sum_p W_qp V_p*^-1 W_qp^T and the right-hand side
        -g_q + sum_p W_qp V_p*^-1 g_p; the back-substitution gains -W_qp^T dq."""
        F, C6, q = len(self.free), 6 * len(self.free), len(self.idx)
        mv = self.moving
        Vi = bo.damped_point_inverses(s["V"], mv, lam)
        if Vi is None:
            return None
        use = mv[self.pt] & (self.slot[self.cam] >= 0)
        S = np.zeros((C6, C6))
        rhs = np.zeros(C6)
        for k, c in enumerate(self.free):
            U = s["U"][c].copy()
            U[np.diag_indices(6)] = np.diag(U) + lam * np.diag(U)
            S[6 * k:6 * k + 6, 6 * k:6 * k + 6] = U
            rhs[6 * k:6 * k + 6] = -s["gc"][c]
        obs = np.nonzero(use)[0]
        Y = np.einsum("mij,mjk->mik", s["W"][obs], Vi[self.pt[obs]])
        a = self.slot[self.cam[obs]]
        np.add.at(rhs.reshape(F, 6) if F else rhs.reshape(0, 6), a, np.einsum("mij,mj->mi", Y, s["gp"][self.pt[obs]]))
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
        # the border
        n = C6 + q
        A = np.zeros((n, n))
        y = np.zeros(n)
        A[:C6, :C6] = S
        y[:C6] = rhs
        Yq = np.einsum("pij,pjk->pik", s["Wq"], Vi)                                   # W_qp V*^-1 (q x 3); zero for a held point
        Saq = np.zeros((F, 6, q))
        Saq[:] = s["Ucq"][self.free]
        np.add.at(Saq, a, -np.einsum("mik,mjk->mij", Y, s["Wq"][self.pt[obs]]))
        Uqq = s["Uqq"].copy()
        Uqq[np.diag_indices(q)] = np.diag(Uqq) + lam * np.diag(Uqq)
        A[:C6, C6:] = Saq.reshape(C6, q)
        A[C6:, :C6] = Saq.reshape(C6, q).T
        A[C6:, C6:] = Uqq - np.einsum("pik,pjk->ij", Yq, s["Wq"])
        y[C6:] = -s["gq"] + np.einsum("pik,pk->i", Yq, s["gp"])
        try:
            L = np.linalg.cholesky(A) if n else np.zeros((0, 0))
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(L)):
            return None
        d = np.linalg.solve(L.T, np.linalg.solve(L, y)) if n else np.zeros(0)
        dc = np.zeros((self.C, 6))
        dc[self.free] = d[:C6].reshape(F, 6)
        dq = d[C6:]
        t = -s["gp"].copy()
        np.add.at(t, self.pt[obs], -np.einsum("mij,mi->mj", s["W"][obs], dc[self.cam[obs]]))
        t -= np.einsum("pqj,q->pj", s["Wq"], dq)
        dX = np.where(mv[:, None], np.einsum("pij,pj->pi", Vi, t), 0.0)
        return dc, dX, dq


def adjust(K, poses, points, cam, pt, uv, fixed=(0,), max_steps=50, refine=(), loss="squared", loss_scale=1.0,
           solver="schur"):
    """-> the dict of ``bundle_robust_oracle.adjust`` plus K (3, 3), the refined camera matrix (the input K after a bad
    start or a bad index) and trace, the (cost, trial cost) pairs of the accept tests.  The LM loop is
    bundle_oracle.adjust's, with dq in |delta|, the free intrinsics in |x|, the trial K in the trial cost, and no rescale of
    K."""
    poses, points, cam, pt, uv, out = bro._inputs(poses, points, cam, pt, uv)
    out["K"] = np.array(K, dtype=np.float64).reshape(3, 3)
    out.pop("cg")
    if out["status"] != bo.OK:
        return out
    prob = Problem(K, poses, points, cam, pt, uv, fixed, refine, loss, loss_scale)
    solve = prob.solve_schur if solver == "schur" else prob.solve_dense
    s = prob.system(poses, points)
    cur = s["cost"]
    out["initial_cost"] = out["final_cost"] = cur
    if not np.isfinite(cur):
        out["status"] = bo.BAD_START
        return out
    anchor = None
    fixed_idx = np.nonzero(prob.fixed)[0]
    if len(fixed_idx) == 1 and len(prob.free):
        c0 = bo.centre(poses[fixed_idx[0]])
        a = int(prob.free[0])
        anchor = (c0, a, float(np.linalg.norm(bo.centre(poses[a]) - c0)))
    theta = lambda K: np.array([K[0, 0], K[0, 2], K[1, 2]])[prob.idx]   # noqa: E731
    lam, steps, accepted, stop = bo.LAMBDA0, 0, 0, max_steps <= 0
    trace = []   # (cost, trial cost) of every trial step that reached the accept test
    while not stop:
        steps += 1
        step = solve(s, lam)
        ok = step is not None and all(np.all(np.isfinite(v)) for v in step)
        K_trial = stepped(prob.K, prob.idx, step[2]) if ok else None
        if K_trial is None:
            lam *= 10.0
        else:
            dc, dX, dq = step
            dn = np.sqrt(np.sum(dc[prob.free] ** 2) + np.sum(dX[prob.moving] ** 2) + np.sum(dq ** 2))
            xn = np.sqrt(np.sum(poses[prob.free, 9:] ** 2) + np.sum(points[prob.moving] ** 2) + np.sum(theta(prob.K) ** 2))
            if dn <= bo.MIN_STEP * (1.0 + xn):
                stop = True
            else:
                trial = poses.copy()
                for c in prob.free:
                    R, t = pnp_refine_oracle.apply_step(poses[c, :9].reshape(3, 3), poses[c, 9:], dc[c])
                    trial[c] = np.concatenate([R.reshape(9), t])
                tpts = points + dX
                K_cur, prob.K = prob.K, K_trial
                new = prob.cost(trial, tpts)
                trace.append((cur, new))
                if np.isfinite(new) and new < cur:
                    stop = cur - new < bo.MIN_DECREASE * cur
                    if anchor is not None:
                        trial, tpts = bo.rescale(trial, tpts, prob.free, *anchor)
                    poses, points, cur = trial, tpts, new
                    lam /= 10.0
                    accepted += 1
                    s = prob.system(poses, points)
                else:
                    prob.K = K_cur
                    lam *= 10.0
        if steps >= max_steps or lam > bo.LAMBDA_MAX:
            stop = True
    out.update(poses=poses, points=points, final_cost=cur, steps=steps, accepted=accepted, weights=s["w"], K=prob.K, trace=trace)
    return out
