"""The pose, track and bundle kernels on the MI355X at the cameras and worlds of tests/geometry_cases.py: every camera
(zero skew, skew, all six entries of rows 0 and 1, 8k pixels, normalised coordinates) times worlds that are turned, scaled
by 1e3 and 1e-3, and moved 2e4 scene sizes away.  Each kernel is compared with its oracle (checked against the truth in
tests/test_geometry_cases_host.py) under the checks and tolerances of its own parity test, with the truth on noise-free
data, and with itself under the change of world (equivariance).  Sizes are small: correctness here does not depend on size.

Rules for the numbers:
  * lengths are compared in the world's own unit: "1e-9 * max(1, |t|)" at world ``id`` reads 1e-9 * max(s, |t'|) at scale s;
    the bundle results are mapped back to the original frame and unit and compared with the unchanged absolute tolerances;
  * truth, noise-free: ten times the oracle's own error on that input plus the kernel's parity tolerance;
  * ``far`` is ill-conditioned by construction and the device and the oracle use different stable algorithms: there the
    device's error against the truth may be at most ten times the oracle's on the same input;
  * equivariance, device against device: one-shot kernels to their parity tolerance, iterative ones on the final cost."""
import random

import numpy as np
import pytest
import torch

import bundle_oracle as bo
import bundle_pcg_oracle as pco
import geometry_cases as gc
import p3p_oracle as p3o
import pnp_oracle as po
import pnp_refine_oracle as ro
import tracks_oracle as to
from structure_from_motion_amd import device
from structure_from_motion_amd._native import AGG_RMS
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.pnp import pnp

pytestmark = pytest.mark.gpu

CAMERAS = list(gc.CAMERAS)
SCORE_WORLDS = ("id", "turned", "large", "far")
FIT_TOL = 1e-9          # test_gpu_pnp.py::test_fit_parity, test_gpu_p3p.py::_fit_parity
SUM_TOL = 1e-13         # test_gpu_pnp.py::test_score_parity
MIN_ANGLE = np.radians(1.0)
MAX_ERROR = 16.0        # px^2 at the bench camera's pixel unit
# test_gpu_tracks.py's constants
POINT_TOL = 1e-9
VALUE_TOL = 1e-9
REFINED_POINT_TOL = 1e-6
REFINED_ERROR_TOL = 1e-5
COST_TOL = 1e-9
STATUS_BAND = 1e-6
# In a world whose unit is not the scene's size (``large``, ``small``) the columns of the oracle's unconditioned A differ by
# the factor s, and LAPACK's SVD returns the null vector less accurately: against inverse iteration on A^T A in extended
# precision the oracle's linear estimate is off by 1.9e-14 relative at ``id``, 2.7e-13 at ``large`` and 1.9e-12 at ``small``
# (0.5 px noise), while the device's streamed QR keeps 3e-15 against the truth in all three.  The point parity (worst
# 4.9e-12) stays far inside POINT_TOL, but e is about 400 times as sensitive as the point (2 r f / z at r of a few pixels):
# 7 times that at wide8k's focal length): measured worst error parity 2.7e-8 (wide8k/small), 2.2e-9 (wide8k/large), 1.8e-9
# (affine/small) against 8.8e-11 at s = 1; each point's cost still agrees to 3.4e-10 (COST_TOL).  One order of margin.
SCALED_VALUE_TOL = 3e-7
# test_gpu_bundle.py / test_gpu_bundle_pcg.py (random graphs): the device and the oracle take the same LM path
POSE_TOL = 1e-10
BUNDLE_POINT_TOL = 1e-10
# Near convergence a trial step is accepted or rejected, and the run stopped, on a decrease of the size of the rounding of
# the cost, so two summation orders can end a rejected trial or a last small step apart.  The oracle against itself with
# the observations permuted (nothing but the summation order changes) does so at wide8k/id (10 steps against 11) and
# affine/turned (10 against 8), with the same accepted count and the costs equal to 2e-15, and then differs by
# 3.6e-10 / 1.3e-8 and 4.6e-12 / 1.8e-10 (poses / points) — the very gaps the device shows against the oracle there
# (3.7e-10 / 1.4e-8 and 4.2e-12 / 1.7e-10); where the step counts agree it agrees to 3e-15 / 5e-14.  So where the step counts
# of device and oracle differ, the estimates are held to the size of such a last step with one order of margin, and the
# final cost to the unchanged 1e-9.
LAST_STEP_POSE_TOL = 5e-9
LAST_STEP_POINT_TOL = 2e-7


@pytest.fixture(scope="module")
def dev(native_lib):
    return device.require_gpu()


def _length(world, t):
    return max(gc.WORLDS[world][0], float(np.max(np.abs(t))))


def _items(pts):
    return [(row[:3].copy(), Feature(float(row[3]), float(row[4]))) for row in pts]


def _table(n, h, seed):
    return device.pyshuffle_table(n, h, random.Random(seed), advance=False)[0]


def _fit(pts, S, K, solver):
    n, h = pts.shape[0], S.shape[0]
    fit = device.p3p_fit if solver == "p3p" else device.pnp_fit
    model, flags = fit(device.to_device(pts).reshape(1, n, 5), device.to_device(S, torch.int32).reshape(1, h, 8), K)
    return model.cpu().numpy()[0], flags.cpu().numpy()[0]


def _pose_gap(world, model, R, t):
    """(max |R - R_ref|, max |t - t_ref| / world length) of a model row."""
    return gc.rotation_gap(model[:9].reshape(3, 3), R), float(np.max(np.abs(model[9:] - t))) / _length(world, t)


def _worst(*values):
    """The largest value; NaN if any is NaN (so that a model of NaNs fails the bound it is held to)."""
    return float(np.max(values))


# ---- DLT fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
def test_dlt_fit(dev, camera):
    K = gc.CAMERAS[camera]
    n, h = 400, 1000
    noisy = gc.pnp_case(camera, n, 21, 0.3, 0.5)
    clean = gc.pnp_case(camera, n, 22, 0.0, 0.0)
    S = _table(n, h, 5)
    for world in gc.ALL_WORLDS:
        # parity on noisy pixels with outliers (test_fit_parity's checks)
        pts, _, _ = gc.pnp_to(world, *noisy)
        model, flags = _fit(pts, S, K, "dlt")
        checked, worst = 0, [0.0, 0.0]
        ratios = np.zeros(h)
        for k in range(h):
            idx = S[k, :6]
            R_o, t_o, ratios[k] = po.fit(pts[idx, :3], pts[idx, 3:], K)
            assert flags[k] == (0 if ratios[k] >= po.DEGENERATE_FLOOR else 1), (world, k)
            if ratios[k] < 1e-3 or not np.all(np.isfinite(model[k])):
                continue
            gap = _pose_gap(world, model[k], R_o, t_o)
            worst = [_worst(a, b) for a, b in zip(worst, gap)]
            checked += 1
        assert checked > h // 2
        # truth on noise-free pixels
        ptc, R, t = gc.pnp_to(world, *clean)
        mc, _ = _fit(ptc, S[:200], K, "dlt")
        dev_err, orc_err, truth_checked = 0.0, 0.0, 0
        for k in range(200):
            idx = S[k, :6]
            R_o, t_o, ratio = po.fit(ptc[idx, :3], ptc[idx, 3:], K)
            if ratio < 1e-3:
                continue
            truth_checked += 1
            dev_err = _worst(dev_err, *_pose_gap(world, mc[k], R, t))
            orc_err = _worst(orc_err, *_pose_gap(world, np.concatenate([R_o.reshape(9), t_o]), R, t))
        assert truth_checked > 100
        # equivariance, device against device: the models at this world, mapped back, against the models at ``id``.  The DLT's
        # t = p4 / mean(S) follows a move of the world origin only as far as M / mean(S) is a rotation — exactly on noise-free
        # pixels, not on noisy ones — so with noise t is compared in the worlds that keep the origin.
        back, back_c = gc.poses_back(world, model), gc.poses_back(world, mc)
        if world == "id":
            base, base_c, base_use = back, back_c, ratios >= 1e-3
        use = base_use & (ratios >= 1e-3) & np.all(np.isfinite(model), axis=1)
        eq_R = float(np.max(np.abs(back[use, :9] - base[use, :9])))
        eq_t = 0.0
        if not np.any(gc.WORLDS[world][2]):
            eq_t = float(np.max(np.abs(back[use, 9:] - base[use, 9:]) / np.maximum(1.0, np.abs(base[use, 9:]).max(axis=1))[:, None]))
        fine = np.array([po.fit(clean[0][S[k, :6], :3], clean[0][S[k, :6], 3:], K)[2] >= 1e-3 for k in range(200)])
        eq_R = max(eq_R, float(np.max(np.abs(back_c[fine, :9] - base_c[fine, :9]))))
        eq_t = max(eq_t, float(np.max(np.abs(back_c[fine, 9:] - base_c[fine, 9:]) /
                                      np.maximum(1.0, np.abs(base_c[fine, 9:]).max(axis=1))[:, None])))
        print(f"dlt fit {camera}/{world}: parity R {worst[0]:.2e} t {worst[1]:.2e} of {checked}; truth device {dev_err:.2e} "
              f"oracle {orc_err:.2e}; equivariance R {eq_R:.2e} t {eq_t:.2e}")
        if world == "far":
            # Measured (all cameras): device 3.33e-10, oracle 3.32e-10 .. 3.33e-10 — both the rounding of pixels that were
            # projected from coordinates of 2e4, not the solver (P3P: 1.20e-10 for both).
            assert dev_err <= 10.0 * orc_err
        else:
            assert worst[0] <= FIT_TOL and worst[1] <= FIT_TOL
            assert dev_err <= 10.0 * orc_err + FIT_TOL
            assert eq_R <= FIT_TOL and eq_t <= FIT_TOL


# ---- P3P fit -----------------------------------------------------------------------------------------------------------
def _p3p_host(items, S_row, K):
    """test_gpu_p3p.py::_host_fit: (model (12,), flag, near tie of item 3)."""
    sample = [items[i] for i in S_row[:4]]
    try:
        R, t = pnp.p3p_model_fitter(sample, K)
    except pnp.PnPCalculationError:
        return np.full(12, np.nan), 1, False
    es = sorted(pnp.calculate_reprojection_score(c, sample[3], K) for c in pnp.p3p_candidates(sample, K))
    near = len(es) > 1 and np.isfinite(es[0]) and es[1] - es[0] <= 1e-9 * max(abs(es[0]), 1e-300)
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t)]), 0, near


@pytest.mark.parametrize("camera", CAMERAS)
def test_p3p_fit(dev, camera):
    """test_fit_parity_pyshuffle's checks over the five worlds of one camera, 5 x 800 = 4 000 samples: its bounds for 20 000
    samples (2 no-solution mismatches, 20 near ties, 40 ill-conditioned samples beyond 1e-9, more than 100 no-solution
    samples) are a fifth here."""
    K = gc.CAMERAS[camera]
    n, h = 400, 800
    noisy = gc.pnp_case(camera, n, 31, 0.3, 0.5)
    clean = gc.pnp_case(camera, n, 32, 0.0, 0.0)
    S = _table(n, h, 6)
    nan_mismatch = near = beyond = nans = 0
    base = None
    for world in gc.ALL_WORLDS:
        pts, _, _ = gc.pnp_to(world, *noisy)
        items = _items(pts)
        model, flags = _fit(pts, S, K, "p3p")
        nans += int(np.isnan(model[:, 0]).sum())
        compared = np.zeros(h, dtype=bool)
        for k in range(h):
            ref, flag, tie = _p3p_host(items, S[k], K)
            assert flags[k] == flag, (world, k)
            if flag:
                continue
            if np.isnan(ref[0]) != np.isnan(model[k, 0]):
                nan_mismatch += 1
                continue
            if np.isnan(ref[0]):
                continue
            if tie:
                near += 1
                continue
            compared[k] = True
            if not _worst(*_pose_gap(world, model[k], ref[:9].reshape(3, 3), ref[9:])) <= FIT_TOL:
                beyond += 1
                compared[k] = False
        # truth on noise-free pixels: well-conditioned samples only (po.condition is that of the problem at ``id``)
        ptc, R, t = gc.pnp_to(world, *clean)
        mc, _ = _fit(ptc, S[:200], K, "p3p")
        itc = _items(ptc)
        dev_err = orc_err = 0.0
        for k in range(200):
            if p3o.condition(clean[0][S[k, :4], :3], clean[1], clean[2]) > 1e5:
                continue
            ref, _, _ = _p3p_host(itc, S[k], K)
            dev_err = _worst(dev_err, *_pose_gap(world, mc[k], R, t))
            orc_err = _worst(orc_err, *_pose_gap(world, ref, R, t))
        back = gc.poses_back(world, model)
        if world == "id":
            base, base_ok = back, compared
        use = compared & base_ok
        eq = np.abs(back[use] - base[use])
        scale = np.maximum(1.0, np.abs(base[use, 9:]).max(axis=1))
        eq_far = int(np.count_nonzero((eq[:, :9].max(axis=1) > FIT_TOL) | (eq[:, 9:].max(axis=1) > FIT_TOL * scale)))
        print(f"p3p fit {camera}/{world}: truth device {dev_err:.2e} host {orc_err:.2e}; equivariance beyond 1e-9: {eq_far} of "
              f"{int(use.sum())}; so far no-solution {nans}, mismatches {nan_mismatch}, near ties {near}, beyond {beyond}")
        if world == "far":
            assert dev_err <= 10.0 * orc_err
        else:
            assert dev_err <= 10.0 * orc_err + FIT_TOL
            # the ill-conditioned samples (the danger cylinder) are the same rare ones as in the parity count
            assert eq_far <= 8
    assert nans > 20 and nan_mismatch <= 1 and near <= 4 and beyond <= 8, (nans, nan_mismatch, near, beyond)


# ---- score, mask and the whole pass ---------------------------------------------------------------------------------------
def _oracle_sums(pts, model, S, K, thr, sample):
    """test_gpu_pnp.py::_oracle_sums with a sample of 4 or 6: the device's summation order."""
    h = model.shape[0]
    cnt = np.zeros(h, dtype=np.int32)
    s1, s2 = np.zeros(h), np.zeros(h)
    errs = []
    for k in range(h):
        e = po.score_values(model[k, :9].reshape(3, 3), model[k, 9:], K, pts)
        errs.append(e)
        with np.errstate(invalid="ignore"):
            passed = e <= thr
        a1 = np.cumsum(e[passed])[-1] if passed.any() else 0.0
        a2 = np.cumsum(e[passed] * e[passed])[-1] if passed.any() else 0.0
        c = int(np.count_nonzero(passed))
        for i in S[k, :sample]:
            if e[i] <= thr:
                c -= 1
            else:
                with np.errstate(over="ignore", invalid="ignore"):
                    a1 += e[i]
                    a2 += e[i] * e[i]
        cnt[k], s1[k], s2[k] = c, a1, a2
    return cnt, s1, s2, errs


def _close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    finite = np.isfinite(a) & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(same | (finite & (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))))))


@pytest.mark.parametrize("solver,sample", [("dlt", 6), ("p3p", 4)])
@pytest.mark.parametrize("camera", CAMERAS)
def test_score_mask_and_pass(dev, camera, solver, sample):
    """The contract of test_score_parity (counts equal, sums to 1e-13, the thresholds 0, inf, nan, 1e300) and of the pass:
    the winner and its mask are those the reference's rule picks from the oracle's scores of the same models."""
    K = gc.CAMERAS[camera]
    n, h, min_extra = 700, 200, 20
    base = gc.pnp_case(camera, n, 41, 0.3, 0.02)   # test_gpu_pnp.py::_pair_data's noise: a six-point DLT is minimal
    winners = {}
    for world in SCORE_WORLDS:
        pts, _, _ = gc.pnp_to(world, *base)
        far_side = np.random.default_rng(n).random(n) < 0.05       # a few points mirrored through the world origin
        pts[far_side, :3] = 2.0 * gc.WORLDS[world][2] - pts[far_side, :3]
        pts_d = device.to_device(pts).reshape(1, n, 5)
        ws = device.PnPWorkspace(1, n, h, dev)
        thr4 = gc.threshold(camera, 4.0)
        ws.run(pts_d, K, thr4, min_extra, AGG_RMS, philox=(77, 0, 1), solver=solver)
        S = ws.S[0].cpu().numpy()
        assert np.array_equal(S, device.sample_philox(77, 0, h, n).cpu().numpy()[0])
        model, flags = ws.model[0].cpu().numpy(), ws.flags[0].cpu().numpy()
        S_d, model_d = ws.S, ws.model
        for thr in (thr4, 1e300, 0.0, float("nan"), float("inf")):
            cnt, s1, s2 = (a.cpu().numpy()[0] for a in device.pnp_score(pts_d, model_d, S_d, K, thr, sample_size=sample))
            c_o, s1_o, s2_o, errs = _oracle_sums(pts, model, S, K, thr, sample)
            assert np.array_equal(cnt, c_o), (world, thr, np.nonzero(cnt != c_o)[0][:5])
            assert _close(s1, s1_o, SUM_TOL) and _close(s2, s2_o, SUM_TOL), (world, thr)
        # the pass: strict <, earliest first, NaN never, among unflagged hypotheses with enough survivors
        c_o, s1_o, s2_o, errs = _oracle_sums(pts, model, S, K, thr4, sample)
        best, best_err = -1, np.inf
        for k in range(h):
            if flags[k] or c_o[k] < min_extra:
                continue
            err = np.sqrt(s2_o[k] / (c_o[k] + sample))
            if err < best_err:
                best, best_err = k, err
        out = ws.outcome(0)
        winners[world] = best
        assert out.best_h == best, (world, out.best_h, best)
        result = device.select_best(ws.cnt, ws.s1, ws.s2, ws.flags, min_extra, AGG_RMS, sample_size=sample)
        mask = device.pnp_inlier_mask(pts_d, model_d, S_d, K, result, thr4, sample_size=sample)[0].cpu().numpy()
        if best < 0:
            # no hypothesis gathers min_extra inliers: no winner on the device either, and an empty mask
            assert out.mask is None and not mask.any() and not ws.mask.any(), world
            print(f"score/mask/pass {camera}/{world}/{solver}: no winner (most extra inliers {int(c_o.max())})")
            continue
        assert abs(out.error - best_err) <= 1e-12 * best_err
        with np.errstate(invalid="ignore"):
            ref_mask = (errs[best] <= thr4).astype(np.uint8)
        ref_mask[S[best, :sample]] = 2
        assert np.array_equal(out.mask, ref_mask), world
        assert np.array_equal(mask, ref_mask), world
        print(f"score/mask/pass {camera}/{world}/{solver}: winner {best}, {int(c_o[best])} extra inliers, error {best_err:.4g}")
    # The DLT's t does not follow a move of the world origin on noisy pixels: at ``far`` 0.02 px of noise put
    # every six-point fit off by more than the gate, and the pass has no winner.  Where the origin stays, and with P3P
    # everywhere, it has one.
    assert winners["id"] >= 0 and winners["large"] >= 0
    assert solver == "dlt" or min(winners.values()) >= 0


# ---- refinement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
def test_pnp_refine(dev, camera):
    """test_gpu_pnp_refine.py::test_parity_with_oracle's checks (rms, two rounds), and one round ends no higher than the true
    pose on the winner's inliers; the final cost is the same in every world.  The winner, its mask and its error come from
    one DLT pass at ``id`` and are carried to each world, so that every world refines the same problem (the DLT's own t
    does not follow a move of the origin on noisy pixels)."""
    K = gc.CAMERAS[camera]
    thr = gc.threshold(camera, 4.0)
    n, h = 2000, 400   # test_parity_with_oracle's sizes: at 0.5 px few six-point fits gather ten extra inliers
    base = gc.pnp_case(camera, n, 101, 0.3, 0.5)
    ws = device.PnPWorkspace(1, n, h, dev)
    ws.run(device.to_device(base[0]).reshape(1, n, 5), K, thr, 10, AGG_RMS, philox=(5, 0, 1000))
    rec = device.read_select(ws.result)[0]
    assert rec.best_h >= 0
    winner = ws.model[0, rec.best_h].cpu().numpy()
    mask_in, err = ws.mask[0].cpu().numpy(), float(rec.best_err)
    err_d = torch.tensor([err], dtype=torch.float64, device=dev)
    costs = {}
    for world in gc.ITERATIVE_WORLDS:
        view, R_true, t_true = gc.pnp_to(world, *base)
        pts = device.to_device(view).reshape(1, n, 5)
        m = gc.poses_to(world, winner)
        R0, t0 = m[:9].reshape(3, 3), m[9:]
        model_d = device.to_device(m).reshape(1, 12)
        model, mask, info = device.pnp_refine(pts, model_d, ws.mask, err_d, K, thr, AGG_RMS, 2, 20)
        model, mask, info = model.cpu().numpy()[0], mask.cpu().numpy()[0], device.read_pnp_refine_info(info)[0]
        ref = ro.refine(view, R0, t0, K, mask_in, err, thr, AGG_RMS, rounds=2, max_steps=20)
        gap = _pose_gap(world, model, ref["R"], ref["t"])
        assert gap[0] <= 1e-9 and gap[1] <= 1e-9, (world, gap)
        assert info.accepted == ref["accepted"] and info.accepted >= 1, (world, info)
        e = po.score_values(ref["R"], ref["t"], K, view)
        with np.errstate(invalid="ignore"):
            borderline = np.abs(e - thr) <= 1e-9 * thr
        assert np.array_equal(mask[~borderline], ref["mask"][~borderline]), world
        assert abs(info.count - ref["count"]) <= int(np.count_nonzero(borderline)), world
        if not borderline.any():
            assert info.count == ref["count"]
            assert abs(info.error - ref["error"]) <= 1e-9 * abs(ref["error"]), world
        one, _, info1 = device.pnp_refine(pts, model_d, ws.mask, err_d, K, thr, AGG_RMS, 1, 20)
        one = one.cpu().numpy()[0]
        inl = view[mask_in != 0]
        final = ro.cost(one[:9].reshape(3, 3), one[9:], K, inl)
        truth = ro.cost(R_true, t_true, K, inl)
        costs[world] = (final, device.read_pnp_refine_info(info1)[0].lm_steps)
        print(f"pnp refine {camera}/{world}: parity R {gap[0]:.2e} t {gap[1]:.2e}; one round: cost {final:.9g} in "
              f"{costs[world][1]} steps, true pose {truth:.9g}, {len(inl)} inliers")
        assert final <= truth, world
    for world in gc.ITERATIVE_WORLDS[1:]:
        assert abs(costs[world][0] - costs["id"][0]) <= 1e-9 * costs["id"][0], (world, costs)


# ---- bundle adjustment -----------------------------------------------------------------------------------------------------
def _bundle(pr, pcg):
    call = device.bundle_adjust_pcg if pcg else device.bundle_adjust
    out = call(device.to_device(pr["poses"]), device.to_device(pr["points"]),
               device.to_device(pr["camera_indices"], dtype=torch.int32), device.to_device(pr["point_indices"], dtype=torch.int32),
               device.to_device(pr["pixels"]), pr["K"], (0,), 50)
    read = device.read_bundle_pcg_info if pcg else device.read_bundle_info
    return out[0].cpu().numpy(), out[1].cpu().numpy(), read(out[2])


@pytest.mark.parametrize("pcg", [False, True], ids=["dense", "pcg"])
@pytest.mark.parametrize("camera", CAMERAS)
def test_bundle_adjust(dev, camera, pcg):
    """The checks of test_gpu_bundle.py / test_gpu_bundle_pcg.py::test_parity_with_oracle (random graph).  The estimates are
    mapped back to the original frame and unit before their absolute tolerances are applied."""
    base = gc.bundle_case(camera, 8, 1000, 12)
    costs = {}
    for world in gc.ITERATIVE_WORLDS:
        pr = gc.problem_to(world, base)
        poses, points, info = _bundle(pr, pcg)
        args = (pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])
        ref = pco.adjust_pcg(*args) if pcg else bo.adjust(*args)
        assert info.status == ref["status"] == 0
        assert info.accepted == ref["accepted"] and info.accepted >= 3, (world, info, ref["accepted"], ref["steps"])
        same_path = info.steps == ref["steps"]
        if pcg and same_path:
            assert info.cg_iterations == ref["cg_iterations"] and info.cg_max == ref["cg_max"], (world, info, ref["cg"])
        assert abs(info.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
        assert abs(info.final_cost - ref["final_cost"]) <= 1e-9 * ref["final_cost"], (world, info.final_cost, ref["final_cost"])
        assert info.final_cost < 0.01 * info.initial_cost
        pose_gap = float(np.max(np.abs(gc.poses_back(world, poses) - gc.poses_back(world, ref["poses"]))))
        point_gap = float(np.max(np.abs(gc.points_back(world, points) - gc.points_back(world, ref["points"]))))
        truth = bo.cost(pr["poses_true"], pr["points_true"], pr["camera_indices"], pr["point_indices"], pr["pixels"], pr["K"])
        costs[world] = (info.final_cost, info.steps)
        print(f"bundle {'pcg' if pcg else 'dense'} {camera}/{world}: pose gap {pose_gap:.2e}, point gap {point_gap:.2e}, cost "
              f"{info.initial_cost:.6g} -> {info.final_cost:.9g} in {info.steps} steps, {info.accepted} accepted (oracle "
              f"{ref['steps']} steps; true parameters {truth:.6g})")
        if same_path:
            assert pose_gap <= POSE_TOL and point_gap <= BUNDLE_POINT_TOL, world
        else:
            assert pose_gap <= LAST_STEP_POSE_TOL and point_gap <= LAST_STEP_POINT_TOL, world
        assert info.final_cost <= truth
    for world in gc.ITERATIVE_WORLDS[1:]:
        assert abs(costs[world][0] - costs["id"][0]) <= 1e-9 * costs["id"][0], (world, costs)


# ---- track triangulation ---------------------------------------------------------------------------------------------------
def _tracks(pr, refine, min_angle, max_error):
    X, status, err, angle, info = device.triangulate_tracks(
        device.to_device(pr["poses"]), device.to_device(pr["cam"], dtype=torch.int32), device.to_device(pr["pt"], dtype=torch.int32),
        device.to_device(pr["uv"]), pr["P"], pr["K"], 2, min_angle, max_error, refine)
    return dict(points=X.cpu().numpy(), status=status.cpu().numpy(), obs_error=err.cpu().numpy(), angle=angle.cpu().numpy(),
                info=device.read_tracks_info(info))


def _rel(points, ref):
    return np.max(np.abs(points - ref), axis=1) / np.linalg.norm(ref, axis=1)


@pytest.mark.parametrize("refine", [0, 10])
@pytest.mark.parametrize("camera", CAMERAS)
def test_triangulate_tracks(dev, camera, refine):
    max_error = gc.threshold(camera, MAX_ERROR)
    P = 1500
    noisy = gc.tracks_case(camera, 6, P, 2, noise_px=0.5, outliers=0.1)
    clean = gc.tracks_case(camera, 6, P, 3, noise_px=0.0)
    base = None
    for world in (gc.ALL_WORLDS if refine == 0 else gc.ITERATIVE_WORLDS):
        # truth on noise-free pixels
        pc = gc.problem_to(world, clean)
        got_c = _tracks(pc, refine, 0.0, np.inf)
        ref_c = to.triangulate(pc["K"], pc["poses"], pc["cam"], pc["pt"], pc["uv"], P, refine_steps=refine)
        assert np.all(got_c["status"] == to.OK)
        dev_err, orc_err = _rel(got_c["points"], pc["points_true"]).max(), _rel(ref_c["points"], pc["points_true"]).max()
        if world == "far":
            # Measured (refine 0, all cameras): device 1.9e-15 .. 2.7e-15, oracle 1.2e-11 .. 2.3e-11 relative to |X'| = 2.3e4:
            # the streamed Givens QR of the device loses fewer digits to the offset than the SVD of the unconditioned A.
            print(f"tracks {camera}/far refine 0: truth device {dev_err:.2e} oracle {orc_err:.2e}")
            assert dev_err <= 10.0 * orc_err
            continue
        assert dev_err <= 10.0 * orc_err + (REFINED_POINT_TOL if refine else POINT_TOL)
        # parity (test_gpu_tracks.py::test_parity_with_oracle)
        pr = gc.problem_to(world, noisy)
        got = _tracks(pr, refine, MIN_ANGLE, max_error)
        ref = to.triangulate(pr["K"], pr["poses"], pr["cam"], pr["pt"], pr["uv"], P, min_angle=MIN_ANGLE, max_error=max_error,
                             refine_steps=refine)
        assert got["info"].status == 0
        max_e = np.full(P, np.nan)
        ok_e = ~np.isnan(ref["obs_error"])
        np.fmax.at(max_e, pr["pt"][ok_e], ref["obs_error"][ok_e])
        near = (np.abs(ref["angle"] - MIN_ANGLE) <= STATUS_BAND * MIN_ANGLE) | (np.abs(max_e - max_error) <= STATUS_BAND * max_error)
        differ = got["status"] != ref["status"]
        assert not np.any(differ & ~near), (world, np.nonzero(differ & ~near)[0][:10])
        assert np.count_nonzero(differ) <= max(2, P // 1000)
        assert got["info"].points_ok == np.count_nonzero(got["status"] == to.OK)
        steps = (got["info"].max_refine_steps_taken, ref["info"]["max_refine_steps_taken"])
        same = ~differ
        assert np.array_equal(np.isnan(got["points"][same]), np.isnan(ref["points"][same]))
        wide = same & (ref["angle"] >= MIN_ANGLE)
        dp = _rel(got["points"][wide], ref["points"][wide])
        da = np.abs(got["angle"][wide] - ref["angle"][wide])
        obs = wide[pr["pt"]] & np.isfinite(ref["obs_error"])
        unit = gc.PIXEL_UNIT[camera] ** 2   # "relative above 1 px^2", in the camera's pixel unit
        de = np.abs(got["obs_error"][obs] - ref["obs_error"][obs]) / np.maximum(unit, np.abs(ref["obs_error"][obs]))
        cost_got = np.bincount(pr["pt"][obs], weights=got["obs_error"][obs], minlength=P)[wide]
        cost_ref = np.bincount(pr["pt"][obs], weights=ref["obs_error"][obs], minlength=P)[wide]
        dc = np.abs(cost_got - cost_ref) / np.maximum(unit, cost_ref)
        # equivariance, device against device.  The linear estimate minimises |A v| over |v| = 1 of the homogeneous point,
        # which a move of the origin or a change of unit does not keep: it follows the world exactly on noise-free pixels only
        # (the oracle moves by 1e-6 .. 4e-5 relative at 0.5 px).  The refined estimate, the minimum of the reprojection
        # error, does follow on noisy pixels.
        eq_got = got if refine else got_c
        back = gc.points_back(world, eq_got["points"])
        if world == "id":
            base = dict(eq_got, points=back)
        both = (eq_got["status"] == to.OK) & (base["status"] == to.OK)
        flips = int(np.count_nonzero(eq_got["status"] != base["status"]))
        eq = _rel(back[both], base["points"][both]).max()
        print(f"tracks {camera}/{world} refine {refine}: truth device {dev_err:.2e} oracle {orc_err:.2e}; parity points "
              f"{dp.max():.3g}, angle {da.max():.3g}, error {de.max():.3g}, point cost {dc.max():.3g}, status differences "
              f"{np.count_nonzero(differ)}, steps {steps[0]} / {steps[1]}; equivariance points {eq:.3g}, status flips {flips}")
        if refine == 0:
            error_tol = VALUE_TOL if gc.WORLDS[world][0] == 1.0 else SCALED_VALUE_TOL
            assert dp.max() <= POINT_TOL and da.max() <= VALUE_TOL and de.max() <= error_tol
        else:
            assert steps[0] == steps[1]
            assert dp.max() <= REFINED_POINT_TOL and da.max() <= REFINED_POINT_TOL and de.max() <= REFINED_ERROR_TOL
        assert dc.max() <= COST_TOL
        assert np.array_equal(np.isnan(got["obs_error"]), np.isnan(ref["obs_error"]))
        assert np.array_equal(np.isinf(got["obs_error"]), np.isinf(ref["obs_error"]))
        assert flips <= max(2, P // 1000)
        assert eq <= (REFINED_POINT_TOL if refine else POINT_TOL)


# ---- two-view DLT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
def test_two_view_triangulate(dev, camera):
    """device.triangulate takes P = K [R | t]: against tracks_oracle.triangulate_pair_dlt with P built from each camera, to
    the 1e-9 relative of test_gpu_tracks.py::test_two_view_tracks_match_device_triangulate."""
    K = gc.CAMERAS[camera]
    for noise in (1.0, 0.0):
        sc = gc.tracks_case(camera, 6, 400, 5, noise_px=noise)
        for world in gc.ALL_WORLDS:
            pr = gc.problem_to(world, sc)
            keep = np.isin(pr["cam"], (1, 4))
            cam, pt, uv = pr["cam"][keep], pr["pt"][keep], pr["uv"][keep]
            both = np.nonzero(np.bincount(pt, minlength=400) == 2)[0]
            assert len(both) > 200
            a = np.array([uv[(pt == p) & (cam == 1)][0] for p in both])
            b = np.array([uv[(pt == p) & (cam == 4)][0] for p in both])
            Pm = [K @ np.hstack([pr["poses"][c, :9].reshape(3, 3), pr["poses"][c, 9:, None]]) for c in (1, 4)]
            X = device.triangulate(device.to_device(np.hstack([a, b])), device.to_device(Pm[0].reshape(12)),
                                   device.to_device(Pm[1].reshape(12))).cpu().numpy()
            ref = np.array([to.triangulate_pair_dlt(K, pr["poses"][1], pr["poses"][4], xa, xb) for xa, xb in zip(a, b)])
            parity = _rel(X, ref).max()
            truth = pr["points_true"][both]
            dev_err, orc_err = _rel(X, truth).max(), _rel(ref, truth).max()
            print(f"two-view {camera}/{world} noise {noise}: parity {parity:.3g}, truth device {dev_err:.3g} oracle {orc_err:.3g}")
            if world != "far":
                assert parity <= 1e-9
            if noise == 0.0:
                # far, measured (all cameras): device 1.2e-15 .. 2.6e-15, oracle 6.6e-12 .. 8.8e-12
                assert dev_err <= 10.0 * orc_err + (0.0 if world == "far" else 1e-9)
