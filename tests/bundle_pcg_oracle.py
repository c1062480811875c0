"""NumPy oracle of the iterative bundle adjuster (csrc/sfm_bundle_pcg.hip, sfm_bundle_adjust_pcg).

The LM loop, the cost, the damping, the stops, the held points and cameras and the gauge rule are those of
``bundle_oracle.adjust``.  Only the solve of the damped reduced camera system differs: S* dc = b with
S* = U* - W V*^-1 W^T and b = -g_c + W V*^-1 g_p is solved by conjugate gradients preconditioned with S*'s 6 x 6 diagonal
blocks, applied matrix-free (S* is never formed).  PCG starts at 0 and stops at the first of |r_k|^2 <= tol^2 |b|^2,
k = max_iterations, or a breakdown (p^T S* p <= 0 or a non-finite scalar: the iterate reached so far is the step; at
k = 0 the step is rejected).  Back-substitution and everything after it is the Schur solver's.  Only the summation
order differs from the device."""
import numpy as np

import bundle_oracle as bo
import pnp_refine_oracle

CG_TOLERANCE = 0.1
MAX_CG_ITERATIONS = 100


class Problem(bo.Problem):
    def solve_pcg(self, s, lam, tol=CG_TOLERANCE, max_iterations=MAX_CG_ITERATIONS):
        """(dc (C, 6), dX (P, 3), cg iterations), or (None, cg iterations) for a rejected step."""
        F = len(self.free)
        mv = self.moving
        Vi = bo.damped_point_inverses(s["V"], mv, lam)
        if Vi is None:
            return None, 0
        use = mv[self.pt] & (self.slot[self.cam] >= 0)   # observations that couple a free camera to a moving point
        obs = np.nonzero(use)[0]
        W = s["W"][obs]                                     # (n, 6, 3)
        a = self.slot[self.cam[obs]]
        p_of = self.pt[obs]
        Y = np.einsum("mij,mjk->mik", W, Vi[p_of])          # W V*^-1
        Us = s["U"][self.free].copy()
        idx = np.arange(6)
        Us[:, idx, idx] = Us[:, idx, idx] * (1.0 + lam)
        # preconditioner blocks M_c = U*_c - sum_p W_cp V_p*^-1 W_cp^T and b = -g_c + sum W V*^-1 g_p
        Mb = Us.copy()
        np.add.at(Mb, a, -np.einsum("mik,mjk->mij", Y, W))
        b = -s["gc"][self.free].copy()
        np.add.at(b, a, np.einsum("mij,mj->mi", Y, s["gp"][p_of]))
        try:
            Lm = np.linalg.cholesky(Mb) if F else np.zeros((0, 6, 6))
        except np.linalg.LinAlgError:
            return None, 0
        if not np.all(np.isfinite(Lm)):
            return None, 0
        Minv = np.linalg.inv(Mb) if F else np.zeros((0, 6, 6))

        def apply_S(x):
            t = np.zeros((self.P, 3))
            np.add.at(t, p_of, np.einsum("mij,mi->mj", W, x[a]))
            y = np.einsum("pij,pj->pi", Vi, t)
            q = np.einsum("cij,cj->ci", Us, x)
            np.add.at(q, a, -np.einsum("mij,mj->mi", W, y[p_of]))
            return q

        x = np.zeros((F, 6))
        r = b.copy()
        z = np.einsum("cij,cj->ci", Minv, r)
        p = z.copy()
        rho = float(np.sum(r * z))
        bb = float(np.sum(b * b))
        rr = bb
        tol2 = tol * tol * bb
        k = 0
        if not np.isfinite(rho) or not np.isfinite(bb):
            return None, 0
        with np.errstate(all="ignore"):
            while True:
                if rr <= tol2 or k == max_iterations:
                    break
                q = apply_S(p)
                pq = float(np.sum(p * q))
                alpha = rho / pq if pq > 0.0 else np.nan
                if not (pq > 0.0) or not np.isfinite(pq) or not np.isfinite(alpha):
                    if k == 0:
                        return None, 0
                    break
                x = x + alpha * p
                r = r - alpha * q
                k += 1
                z = np.einsum("cij,cj->ci", Minv, r)
                rz = float(np.sum(r * z))
                rr = float(np.sum(r * r))
                if not np.isfinite(rz) or not np.isfinite(rr):
                    break
                beta = rz / rho
                rho = rz
                if rr <= tol2 or k == max_iterations:
                    break
                p = z + beta * p
        dc = np.zeros((self.C, 6))
        dc[self.free] = x
        t = -s["gp"].copy()
        np.add.at(t, p_of, -np.einsum("mij,mi->mj", W, dc[self.cam[obs]]))
        dX = np.where(mv[:, None], np.einsum("pij,pj->pi", Vi, t), 0.0)
        return (dc, dX), k


def adjust_pcg(K, poses, points, cam, pt, uv, fixed=(0,), max_steps=50, max_cg_iterations=MAX_CG_ITERATIONS,
               cg_tolerance=CG_TOLERANCE):
    """bundle_oracle.adjust with the PCG solve -> its dict plus cg (the CG iterations of every trial step, a list),
    cg_iterations (their total) and cg_max (the most in one step)."""
    poses = np.array(poses, dtype=np.float64).reshape(-1, 12)
    points = np.array(points, dtype=np.float64).reshape(-1, 3)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = dict(poses=poses.copy(), points=points.copy(), initial_cost=np.nan, final_cost=np.nan, steps=0, accepted=0,
               status=bo.OK, cg=[], cg_iterations=0, cg_max=0)
    if len(cam) and (cam.min() < 0 or cam.max() >= len(poses) or pt.min() < 0 or pt.max() >= len(points)):
        out["status"] = bo.BAD_INDEX
        return out
    prob = Problem(K, poses, points, cam, pt, uv, fixed)
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
    lam, steps, accepted, stop = bo.LAMBDA0, 0, 0, max_steps <= 0
    cg = []
    while not stop:
        steps += 1
        step, k = prob.solve_pcg(s, lam, cg_tolerance, max_cg_iterations)
        cg.append(k)
        ok = step is not None and np.all(np.isfinite(step[0])) and np.all(np.isfinite(step[1]))
        if not ok:
            lam *= 10.0
        else:
            dc, dX = step
            dn = np.sqrt(np.sum(dc[prob.free] ** 2) + np.sum(dX[prob.moving] ** 2))
            xn = np.sqrt(np.sum(poses[prob.free, 9:] ** 2) + np.sum(points[prob.moving] ** 2))
            if dn <= bo.MIN_STEP * (1.0 + xn):
                stop = True
            else:
                trial = poses.copy()
                for c in prob.free:
                    R, t = pnp_refine_oracle.apply_step(poses[c, :9].reshape(3, 3), poses[c, 9:], dc[c])
                    trial[c] = np.concatenate([R.reshape(9), t])
                tpts = points + dX
                new = bo.cost(trial, tpts, cam, pt, uv, prob.K)
                if np.isfinite(new) and new < cur:
                    stop = cur - new < bo.MIN_DECREASE * cur
                    if anchor is not None:
                        trial, tpts = bo.rescale(trial, tpts, prob.free, *anchor)
                    poses, points, cur = trial, tpts, new
                    lam /= 10.0
                    accepted += 1
                    s = prob.system(poses, points)
                else:
                    lam *= 10.0
        if steps >= max_steps or lam > bo.LAMBDA_MAX:
            stop = True
    out.update(poses=poses, points=points, final_cost=cur, steps=steps, accepted=accepted, cg=cg,
               cg_iterations=int(sum(cg)), cg_max=int(max(cg) if cg else 0))
    return out
