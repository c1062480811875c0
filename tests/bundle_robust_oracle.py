"""NumPy oracle of both bundle adjusters with a robust loss (csrc/sfm_loss.h).

With e an observation's squared reprojection error in px^2 (``bundle_oracle.residuals``), a the scale in pixels and
a2 = a * a, in the device's operation order:

    squared  rho = e                                       w = 1
    huber    rho = e if e <= a2 else (2 a) sqrt(e) - a2    w = 1 if e <= a2 else a / sqrt(e)
    cauchy   rho = a2 log1p(e / a2)                        w = 1 / (1 + e / a2)

The cost is the sum of rho.  The linearisation multiplies r, Jc and Jp of every observation by sqrt(w) at the linearisation
point (iteratively reweighted least squares, first order); the solves are those of ``bundle_oracle.Problem`` and
``bundle_pcg_oracle.Problem`` on the weighted blocks.  The LM loop is ``bundle_oracle.adjust``'s with this cost.  With
``loss="squared"`` every array equals the squared oracles' (x * 1.0 == x)."""
import numpy as np

import bundle_oracle as bo
import bundle_pcg_oracle as bp
import pnp_refine_oracle

LOSSES = ("squared", "huber", "cauchy")


def rho_and_weight(e, loss, scale):
    """(rho(e), w(e) = rho'(e)) elementwise; rho(inf) = inf and w(inf) = 0 for huber and cauchy.  Defined for the scales
    of the contract of csrc/sfm_loss.h (``sfmloss::scale_ok``): a > 0 whose square is a normal finite double, about 1.5e-154
    to 1.3e154.  Outside it a2 is 0 or inf and cauchy's rho is NaN for every e, as the device's would be; every entry point
    refuses such a scale.  Within it rho is +inf where e / a2 overflows."""
    e = np.asarray(e, dtype=np.float64)
    a = float(scale)
    a2 = a * a
    with np.errstate(all="ignore"):
        if loss == "squared":
            return e.copy(), np.ones_like(e)
        if loss == "huber":
            small = e <= a2
            root = np.sqrt(e)
            return np.where(small, e, (2.0 * a) * root - a2), np.where(small, 1.0, a / np.where(small, 1.0, root))
        if loss == "cauchy":
            return a2 * np.log1p(e / a2), 1.0 / (1.0 + e / a2)
    raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")


class _Robust:
    """The cost and the weighted Gauss-Newton blocks; mixed into both Problem classes."""

    def set_loss(self, loss, scale):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        self.loss, self.scale = loss, float(scale)

    def cost(self, poses, points):
        e = bo.residuals(poses, points, self.cam, self.pt, self.uv, self.K)[0]
        return float(np.sum(rho_and_weight(e, self.loss, self.scale)[0]))

    def system(self, poses, points):
        """bundle_oracle.Problem.system on sqrt(w) r, sqrt(w) Jc, sqrt(w) Jp; cost = sum rho; w (M,) beside them."""
        e, r, Jc, Jp = bo.residuals(poses, points, self.cam, self.pt, self.uv, self.K)
        f, w = rho_and_weight(e, self.loss, self.scale)
        sw = np.sqrt(w)   # 0 behind the camera, where r, Jc and Jp are 0 already
        r = r * sw[:, None]
        Jc = Jc * sw[:, None, None]
        Jp = Jp * sw[:, None, None]
        U = np.zeros((self.C, 6, 6))
        gc = np.zeros((self.C, 6))
        V = np.zeros((self.P, 3, 3))
        gp = np.zeros((self.P, 3))
        np.add.at(U, self.cam, np.einsum("mki,mkj->mij", Jc, Jc))
        np.add.at(gc, self.cam, np.einsum("mki,mk->mi", Jc, r))
        np.add.at(V, self.pt, np.einsum("mki,mkj->mij", Jp, Jp))
        np.add.at(gp, self.pt, np.einsum("mki,mk->mi", Jp, r))
        W = np.einsum("mki,mkj->mij", Jc, Jp)
        return dict(U=U, gc=gc, V=V, gp=gp, W=W, cost=float(np.sum(f)), w=w)


class Problem(_Robust, bo.Problem):
    def __init__(self, K, poses, points, cam, pt, uv, fixed, loss="squared", loss_scale=1.0):
        bo.Problem.__init__(self, K, poses, points, cam, pt, uv, fixed)
        self.set_loss(loss, loss_scale)


class PcgProblem(_Robust, bp.Problem):
    def __init__(self, K, poses, points, cam, pt, uv, fixed, loss="squared", loss_scale=1.0):
        bp.Problem.__init__(self, K, poses, points, cam, pt, uv, fixed)
        self.set_loss(loss, loss_scale)


def _lm(prob, solve, poses, points, max_steps, out):
    """The LM loop of bundle_oracle.adjust on prob.cost / prob.system; ``solve(s, lam)`` -> (step or None, cg count)."""
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
        step, k = solve(s, lam)
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
                new = prob.cost(trial, tpts)
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
    out.update(poses=poses, points=points, final_cost=cur, steps=steps, accepted=accepted, cg=cg, weights=s["w"])
    return out


def _inputs(poses, points, cam, pt, uv):
    poses = np.array(poses, dtype=np.float64).reshape(-1, 12)
    points = np.array(points, dtype=np.float64).reshape(-1, 3)
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = dict(poses=poses.copy(), points=points.copy(), initial_cost=np.nan, final_cost=np.nan, steps=0, accepted=0,
               status=bo.OK, cg=[])
    if len(cam) and (cam.min() < 0 or cam.max() >= len(poses) or pt.min() < 0 or pt.max() >= len(points)):
        out["status"] = bo.BAD_INDEX
    return poses, points, cam, pt, uv, out


def adjust(K, poses, points, cam, pt, uv, fixed=(0,), max_steps=50, loss="squared", loss_scale=1.0, solver="schur"):
    """bundle_oracle.adjust on the sum of rho -> its dict, plus weights (M,), the w of the last linearisation."""
    poses, points, cam, pt, uv, out = _inputs(poses, points, cam, pt, uv)
    if out["status"] != bo.OK:
        return out
    prob = Problem(K, poses, points, cam, pt, uv, fixed, loss, loss_scale)
    solve = prob.solve_schur if solver == "schur" else prob.solve_dense
    out = _lm(prob, lambda s, lam: (solve(s, lam), 0), poses, points, max_steps, out)
    out.pop("cg")
    return out


def adjust_pcg(K, poses, points, cam, pt, uv, fixed=(0,), max_steps=50, max_cg_iterations=bp.MAX_CG_ITERATIONS,
               cg_tolerance=bp.CG_TOLERANCE, loss="squared", loss_scale=1.0):
    """bundle_pcg_oracle.adjust_pcg on the sum of rho -> its dict (cg, cg_iterations, cg_max), plus weights."""
    poses, points, cam, pt, uv, out = _inputs(poses, points, cam, pt, uv)
    out.update(cg_iterations=0, cg_max=0)
    if out["status"] != bo.OK:
        return out
    prob = PcgProblem(K, poses, points, cam, pt, uv, fixed, loss, loss_scale)
    out = _lm(prob, lambda s, lam: prob.solve_pcg(s, lam, cg_tolerance, max_cg_iterations), poses, points, max_steps, out)
    out.update(cg_iterations=int(sum(out["cg"])), cg_max=int(max(out["cg"]) if out["cg"] else 0))
    return out


def rotation_error(poses, poses_true):
    """The largest angle (rad) between a pose's rotation and the true one."""
    worst = 0.0
    for a, b in zip(np.asarray(poses).reshape(-1, 12), np.asarray(poses_true).reshape(-1, 12)):
        c = (np.trace(a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T) - 1.0) / 2.0
        worst = max(worst, float(np.arccos(np.clip(c, -1.0, 1.0))))
    return worst
