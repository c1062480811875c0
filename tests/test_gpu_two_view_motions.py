"""The two-view kernels on the family of relative motions in tests/motion_cases.py: five-point and eight-point fits, SED
scoring, essential decomposition, the cheirality vote, triangulation, the batched pipeline and the public route, each
against the host definition or the CPU oracle that tests/test_two_view_motions_host.py checks on the same motions."""
import functools
import itertools
import random

import numpy as np
import pytest
import torch

import motion_cases as mc
from oracle import sfm_oracle as orc
from structure_from_motion_amd import device
from structure_from_motion_amd._native import AGG_RMS, ScoreOptions
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.epipolar import epipolar_ransac as er
from structure_from_motion_amd.epipolar import five_point as fp
from structure_from_motion_amd.feature_matching.matching import Match
from test_gpu_five_point import _fit_parity
from test_gpu_parity import _oracle_pair, pose_sets_equal

pytestmark = pytest.mark.gpu

motions = pytest.mark.parametrize("motion", mc.NAMES)


@functools.lru_cache(maxsize=None)
def _scene(motion, n, seed, noise_px=0.0, outliers=0.0):
    return mc.scene(motion, n, seed, noise_px, outliers)


def _truth_gap(E, Et):
    return np.minimum(np.abs(E - Et).max(axis=-1), np.abs(E + Et).max(axis=-1))


# ---- five point ------------------------------------------------------------------------------------------------------
@motions
@pytest.mark.parametrize("n", [6, 200])
def test_five_point_fit_philox(motion, n):
    sc = _scene(motion, 200, 1)
    corr_np = np.ascontiguousarray(sc["corr"][:n])
    corr = device.to_device(corr_np).reshape(1, n, 4)
    S = torch.empty((1, 1000, 8), dtype=torch.int32, device=corr.device)
    E, flags = device.five_point_fit(corr, S, philox=(99, 0, 1))
    E, flags, S = E.cpu().numpy()[0], flags.cpu().numpy()[0], S.cpu().numpy()[0]
    assert not flags.any()
    _fit_parity(corr_np, S, E, flags, either_sign=True)
    Et = mc.true_essential(sc["R"], sc["t"])
    with np.errstate(invalid="ignore"):
        pick = np.where(np.isnan(E[:, 0]), np.inf, _truth_gap(E, Et))
    print(f"{motion} n={n}: item 5 picks the true E on {np.mean(pick <= 1e-6):.3f}")
    if n == 200:   # at n = 6 every sample is the same six items in another order: no population to take a share of
        assert np.mean(pick <= 1e-6) >= 0.98


@motions
def test_five_point_candidates_and_recall(motion):
    sc = _scene(motion, 200, 1)
    n = 200
    corr = device.to_device(sc["corr"]).reshape(1, n, 4)
    table = device.PyShuffleTable(n, 1000, random.Random(4), advance=False)
    S = device.to_device(table.S, dtype=torch.int32).reshape(1, 1000, 8)
    E, flags = device.five_point_fit(corr, S)
    _fit_parity(sc["corr"], table.S, E.cpu().numpy()[0], flags.cpu().numpy()[0], either_sign=True)
    out, count = device.five_point_candidates(corr, S)
    out, count = out.cpu().numpy()[0], count.cpu().numpy()[0]
    cands, cnt_host = fp.candidates_corr(sc["corr"], table.S)
    # the rule of test_gpu_five_point.test_candidates_match_host, in either sign (mc.unit_gap): counts equal on 99 %, and
    # every sample with equal counts within 1e-6 (measured on an MI355X: counts equal on 1.000, candidates within 1e-6 on
    # 1.0000 of the samples, on every motion)
    agree = count == cnt_host
    print(f"{motion}: candidate counts equal the host's on {np.mean(agree):.3f}")
    assert np.mean(agree) >= 0.99
    for h in np.nonzero(agree)[0]:
        if cnt_host[h] > 0:
            assert _truth_gap(out[h, :count[h]], cands[h, :count[h]]).max() <= 1e-6, h
    # the device's own recall: the floors of test_two_view_motions_host.test_five_point_recall
    Et = mc.true_essential(sc["R"], sc["t"])
    assert (count >= 0).all()
    err = np.min(np.where(np.isnan(out[:, :, 0]), np.inf, _truth_gap(out, Et)), axis=1)
    print(f"{motion}: within 1e-9 {np.mean(err <= 1e-9):.3f}, within 1e-6 {np.mean(err <= 1e-6):.3f}")
    assert np.mean(err <= 1e-9) >= 0.94
    assert np.mean(err <= 1e-6) >= 0.98


# ---- eight point -----------------------------------------------------------------------------------------------------
@motions
@pytest.mark.parametrize("noise_px", [0.0, 0.5])
@pytest.mark.parametrize("outliers", [0.0, 0.3])
def test_eight_point_fit(motion, noise_px, outliers):
    """Device (Jacobi) against the oracle (LAPACK) in mc.unit form: E / E[2][2] itself has an arbitrary scale where
    E[2][2] = 0.

    ``outliers=0.3`` is the population of test_gpu_parity's fit tests, most samples holding an outlier or two; there the
    median gap to the oracle is at most 1e-12, as in those tests (measured 2e-14 .. 4e-13).

    With ``outliers=0.0`` every sample lies on one E and is as ill-conditioned as a fit gets, and the median of 1e-12 is NOT
    met against the oracle, with or without noise, on any motion, bench included.  Measured on an MI355X
    (``pytest tests/test_gpu_two_view_motions.py -m gpu -s -k eight_point``): median gap 3.4e-12 .. 2.0e-11 without noise
    (4.5e-12 on bench, 1.1e-11 on tz, 2.0e-11 on turn170) and 1.7e-12 .. 1.2e-11 at 0.5 px (1.9e-12 on bench).  The gap is
    the oracle's error, not the device's: against a 40-digit evaluation of the same algorithm (oracle/fit_mp.py) LAPACK's
    eigen-solve of the squared 9 x 9 matrix is off by a median of 1.4e-12 .. 2.6e-11 over 40 evenly spaced hypotheses
    (1e-8 .. 2e-5 on the worst twelve) and the device by 3.8e-15 .. 2.9e-14 (at most 2e-11 on the worst twelve).  So on
    this population the device is held to the 40-digit fit with the same 1e-12 median, over 40 evenly spaced hypotheses,
    and its gap to the oracle to 1e-12 plus three times the oracle's own median error on those 40.

    Before the fit left E as it is for an E[2][2] of exactly 0, 2 to 12 of the 500 noise-free fits of tgen, pan_tx, ty,
    tilt_ty, roll10_tx, tx, roll90_tx and roll90_tgen were inf and NaN on the device where the oracle's, whose E[2][2] was
    1e-16 instead, were finite."""
    from oracle.fit_mp import fit_eight_point_mp

    n, h = 200, 500
    corr = _scene(motion, n, 1, noise_px, outliers)["corr"]
    S = orc.philox_sample_table(7, 0, h, n)
    E_ref, deg_ref, _ = orc.fit_hypotheses(corr, S)
    E, flags = device.fit_eight_point(device.to_device(corr).reshape(1, n, 4), device.to_device(S, torch.int32).reshape(1, h, 8))
    E = E.cpu().numpy()[0].reshape(h, 3, 3)
    ok = ~deg_ref & np.isfinite(E_ref).all(axis=(1, 2))
    lost = np.nonzero(ok & ~np.isfinite(E).all(axis=(1, 2)))[0]
    both = ok & np.isfinite(E).all(axis=(1, 2))
    gap = np.zeros(h)
    gap[both] = mc.unit_gap(E[both], E_ref[both])
    print(f"{motion} {noise_px} px {outliers}: unit gap max {gap.max():.1e} median {np.median(gap[both]):.1e}, |E| median "
          f"{np.median(np.abs(E_ref[ok]).max(axis=(1, 2))):.1e}, device not finite on {len(lost)}")
    for i in lost[:3]:
        print("    not finite:", i, E[i].reshape(9), "oracle", E_ref[i].reshape(9))
    # the twelve worst against a 40-digit evaluation of the same algorithm (assert_fits_agree's tie-break, in unit form)
    worst = np.argsort(gap)[-12:]
    dev_err, lap_err = [], []
    even = np.arange(0, h, h // 40)[:40] if outliers == 0.0 else np.arange(0, h, h // 12)[:12]
    for i in np.concatenate([worst, even]):
        pts = corr[S[i]]
        truth, _ = fit_eight_point_mp(pts[:, 0:2], pts[:, 2:4])
        dev_err.append(float(mc.unit_gap(E[i], truth)))
        lap_err.append(float(mc.unit_gap(E_ref[i], truth)))
    dev_err, lap_err = np.array(dev_err), np.array(lap_err)
    print(f"    against 40 digits: device median {np.median(dev_err):.1e} max {dev_err.max():.1e}, LAPACK median "
          f"{np.median(lap_err):.1e} max {lap_err.max():.1e}")
    np.testing.assert_array_equal(flags.cpu().numpy()[0] != 0, deg_ref)
    assert len(lost) == 0, lost[:10]
    if outliers > 0.0:
        assert np.median(gap[both]) <= 1e-12
    else:
        dev_even, lap_even = np.median(dev_err[12:]), np.median(lap_err[12:])
        print(f"    40 evenly spaced against 40 digits: device median {dev_even:.1e}, LAPACK median {lap_even:.1e}")
        assert dev_even <= 1e-12
        assert np.median(gap[both]) <= 1e-12 + 3.0 * lap_even
    assert (gap > 1e-6).sum() <= 12
    for k, i in enumerate(worst):
        if gap[i] > 1e-6:   # the two double-precision routes disagree: the device is right
            assert dev_err[k] <= 1e-9 and dev_err[k] <= lap_err[k], (int(i), gap[i], dev_err[k], lap_err[k])
    assert np.median(dev_err) <= 3.0 * np.median(lap_err) + 1e-14
    assert dev_err.max() <= 10.0 * lap_err.max() + 1e-13


# ---- scoring ---------------------------------------------------------------------------------------------------------
@motions
@pytest.mark.parametrize("thr", [1.5e-6, 2e-5])
@pytest.mark.parametrize("kernel", [None, "matrix"])
def test_score_with_the_oracles_E(motion, thr, kernel):
    """The oracle's fits of the noise-free scene (|E| about 1e13 .. 1e19 where E[2][2] = 0) scored on the same points with
    noise and 25 % outliers: counts bit-equal, sums to the summation order."""
    n, h = 1000, 130
    clean = _scene(motion, n, 3)["corr"]
    corr = _scene(motion, n, 3, 0.5, 0.25)["corr"]
    S = orc.philox_sample_table(11, 0, h, n)
    E_ref, _, _ = orc.fit_hypotheses(clean, S)
    cnt_ref, s1_ref, s2_ref = orc.score_hypotheses(corr, E_ref, S, thr)
    options = None if kernel is None else ScoreOptions(kernel=kernel)
    cnt, s1, s2 = device.score_sed(device.to_device(corr).reshape(1, n, 4), device.to_device(E_ref.reshape(1, h, 9)),
                                   device.to_device(S, torch.int32).reshape(1, h, 8), thr, options=options)
    np.testing.assert_array_equal(cnt.cpu().numpy()[0], cnt_ref)
    for got, want in ((s1.cpu().numpy()[0], s1_ref), (s2.cpu().numpy()[0], s2_ref)):
        both_nan = np.isnan(got) & np.isnan(want)
        np.testing.assert_allclose(got[~both_nan], want[~both_nan], rtol=1e-13, atol=0)


# ---- decomposition ---------------------------------------------------------------------------------------------------
def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


@motions
def test_decompose_essential(motion):
    """[t]x R as it is, times 1e16, times 1e-16, and as the oracle fits it from exact data (E / E[2][2], of magnitude
    1e12 .. 1e19 where E[2][2] = 0).  Exact zeros, zero columns and tied singular values are in these matrices."""
    sc = _scene(motion, 200, 1)
    raw = _skew(sc["t"]) @ sc["R"]
    S = mc.samples(200, 20, 8, 3)
    E_fit, flagged, _ = orc.fit_hypotheses(sc["corr"], S)
    fitted = E_fit[~flagged & np.isfinite(E_fit).all(axis=(1, 2))][0]
    forms = {"raw": raw, "times 1e16": raw * 1e16, "times 1e-16": raw * 1e-16, "fitted": fitted}
    poses, status = device.decompose_essential(device.to_device(np.stack([f.reshape(9) for f in forms.values()])))
    poses, status = poses.cpu().numpy(), status.cpu().numpy()
    for k, (name, form) in enumerate(forms.items()):
        assert status[k] == 0, (name, np.abs(form).max())
        # the pose does not depend on the scale of E; recover_all_r_t's absolute sigma_3 test does
        R1, R2, t1 = orc.recover_all_r_t(mc.unit(form) if name == "fitted" else raw)
        assert pose_sets_equal(poses[k], R1, R2, t1, 1e-10), name
        for p in poses[k]:
            R = p[:9].reshape(3, 3)
            np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-13)
            assert abs(np.linalg.det(R) - 1.0) <= 1e-13 and abs(np.linalg.norm(p[9:]) - 1.0) <= 1e-13


# ---- cheirality vote -------------------------------------------------------------------------------------------------
@motions
def test_cheirality(motion):
    sc = _scene(motion, 1000, 5, 0.5, 0.25)
    R1, R2, t1 = orc.recover_all_r_t(_skew(sc["t"]) @ sc["R"])
    candidates = list(itertools.product([R1, R2], [t1, -t1]))
    poses = np.array([np.concatenate([R.reshape(9), t]) for R, t in candidates])
    got = device.cheirality(device.to_device(sc["corr"]), device.to_device(poses), 50.0).cpu().numpy()
    for c, (R, t) in enumerate(candidates):
        want = orc.cheirality_pass(sc["corr"], R, t)
        mism = np.nonzero(got[c].astype(bool) != want)[0]
        assert len(mism) == 0, (c, mism[:10])


# ---- triangulation ---------------------------------------------------------------------------------------------------
@motions
def test_triangulate(motion):
    """The rules of test_gpu_parity.test_triangulate_random_geometries: every point a minimiser of |A x|, the
    well-conditioned ones equal to the SVD's.  In forward motion the points near the epipole have no parallax and fall
    out by that rule."""
    n = 1200
    sc = _scene(motion, n, 5, 0.5, 0.25)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = sc["R"], sc["t"]
    K_ext = np.hstack((sc["K"], np.zeros((3, 1))))
    P1, P2 = K_ext @ np.eye(4), K_ext @ T
    corr = orc.pack_correspondences(sc["pix_a"], sc["pix_b"])
    got = device.triangulate(device.to_device(corr), device.to_device(P1.reshape(12)), device.to_device(P2.reshape(12))).cpu().numpy()
    A = orc.dlt_matrix(corr, P1[:3], P2[:3])
    _, sv, vt = np.linalg.svd(A)
    x = np.column_stack([got, np.ones(n)])
    finite = np.all(np.isfinite(x), axis=1)
    assert finite.mean() > 0.999
    xn = x[finite] / np.linalg.norm(x[finite], axis=1, keepdims=True)
    residual = np.linalg.norm(np.einsum("nij,nj->ni", A[finite], xn), axis=1)
    assert np.max(np.abs(residual - sv[finite, 3]) / sv[finite, 0]) <= 1e-9
    want = orc.triangulate_points(sc["pix_a"], sc["pix_b"], sc["K"], T)
    well = finite & (sv[:, 3] < 1e-3 * sv[:, 2]) & (np.abs(vt[:, 3, 3]) > 1e-6)
    print(f"{motion}: {well.sum()} of {n} points well-conditioned")
    assert well.sum() >= 0.05 * n    # the comparison is not empty: a tenth of the inliers even in forward motion
    assert np.max(np.abs(got[well] - want[well]) / np.linalg.norm(want[well], axis=1, keepdims=True)) <= 1e-9


# ---- the whole path --------------------------------------------------------------------------------------------------
def test_batched_pipeline_one_motion_per_pair():
    """test_gpu_parity.test_batched_two_view_pipeline with one motion per pair, E compared in mc.unit form."""
    from structure_from_motion_amd import batched

    B, n, h, thr, min_extra = len(mc.NAMES), 1200, 400, 1.5e-6, 10
    scenes = [_scene(motion, n, 50 + b, 0.5, 0.25) for b, motion in enumerate(mc.NAMES)]
    K = scenes[0]["K"]
    pipe = batched.TwoViewBatch(B, n, h)
    pipe.run(device.to_device(np.stack([s["pix_a"] for s in scenes])), device.to_device(np.stack([s["pix_b"] for s in scenes])),
             K, seed=70, thr=thr, min_extra=min_extra, aggregation=AGG_RMS)
    results = pipe.results()
    for b, (motion, res) in enumerate(zip(mc.NAMES, results)):
        ref, order, R, t, mask, votes, pts = _oracle_pair(scenes[b]["pix_a"], scenes[b]["pix_b"], K, 70 + b, h, thr, min_extra)
        assert not ref["degenerate"].any(), motion
        assert res.status == batched.OK, (motion, res.status)
        assert res.best_h == ref["best"], motion
        assert mc.unit_gap(res.E, ref["E"]) <= 1e-6, motion
        np.testing.assert_array_equal(res.inlier_order, order)
        assert sorted(res.votes.tolist()) == sorted(votes), motion
        np.testing.assert_allclose(res.R, R, atol=1e-6)
        np.testing.assert_allclose(res.t, t, atol=1e-6)
        np.testing.assert_array_equal(res.pose_mask, mask)
        assert np.max(np.abs(res.points - pts) / np.linalg.norm(pts, axis=1, keepdims=True)) <= 1e-6, motion


# The rotation gap (mc.rotation_gap_of) of the same call through ransac._host_loop on the CPU, per motion and solver:
# the output of ``PYTHONPATH=. python tests/motion_cases.py`` (mc.host_route, mc.ROUTE).  One motion is left out: on turn170
# the host loop itself fails.  Its winner keeps 31 (five point) and 82 (eight point) of about 210 true inliers and is 0.080
# and 0.063 off the true rotation, where every other motion keeps 191 to 209 and is 0.001 to 0.06 off.  A bound of that size
# would check nothing; the batched pipeline test above covers turn170 against the oracle.
HOST_ROUTE_GAP = {
    ("bench", "five_point"): 0.001690902405235839,   # 205 inliers
    ("bench", "eight_point"): 0.017939419092637132,   # 194 inliers
    ("tgen", "five_point"): 0.0010840803292153816,   # 206 inliers
    ("tgen", "eight_point"): 0.009638151915008553,   # 194 inliers
    ("pan_tx", "five_point"): 0.014443828859726587,   # 209 inliers
    ("pan_tx", "eight_point"): 0.025090308828736058,   # 203 inliers
    ("gen_tx", "five_point"): 0.0025310538521116227,   # 208 inliers
    ("gen_tx", "eight_point"): 0.012356650768535801,   # 200 inliers
    ("ty", "five_point"): 0.014100620201730309,   # 206 inliers
    ("ty", "eight_point"): 0.03272678487378898,   # 195 inliers
    ("tilt_ty", "five_point"): 0.011011783491918212,   # 206 inliers
    ("tilt_ty", "eight_point"): 0.06025250319860038,   # 191 inliers
    ("roll10_tx", "five_point"): 0.002637888274686519,   # 207 inliers
    ("roll10_tx", "eight_point"): 0.019069511020120715,   # 202 inliers
    ("tz", "five_point"): 0.001892108068472412,   # 208 inliers
    ("tz", "eight_point"): 0.004659598361306251,   # 207 inliers
    ("gen_tz", "five_point"): 0.0034182282512234957,   # 205 inliers
    ("gen_tz", "eight_point"): 0.0013918465950938652,   # 205 inliers
    ("roll180_tx", "five_point"): 0.007024114494020329,   # 206 inliers
    ("roll180_tx", "eight_point"): 0.03290191155300108,   # 200 inliers
    ("roll15_tz", "five_point"): 0.0035553230371952863,   # 206 inliers
    ("roll15_tz", "eight_point"): 0.008077528721916659,   # 206 inliers
    ("tx", "five_point"): 0.0015531470248420173,   # 208 inliers
    ("tx", "eight_point"): 0.015863603025228525,   # 203 inliers
    ("roll90_tx", "five_point"): 0.0028276191143899528,   # 206 inliers
    ("roll90_tx", "eight_point"): 0.012723525366058483,   # 209 inliers
    ("roll90_tgen", "five_point"): 0.003156581688706852,   # 207 inliers
    ("roll90_tgen", "eight_point"): 0.013417807725729234,   # 206 inliers
}


@pytest.mark.parametrize("motion", [m for m in mc.NAMES if m != "turn170"])
@pytest.mark.parametrize("solver", ["five_point", "eight_point"])
def test_public_route(motion, solver):
    """estimate_essential_mat_with_ransac at 30 % outliers and 0.5 px: the rotation is as close to the truth as the host
    loop's, give or take the 1e-6 by which the two fits may differ."""
    r = mc.ROUTE
    sc = _scene(motion, r["n"], r["scene_seed"], r["noise_px"], r["outlier_fraction"])
    fa = [Feature(float(x), float(y)) for x, y in sc["pix_a"]]
    fb = [Feature(float(x), float(y)) for x, y in sc["pix_b"]]
    matches = [Match(a_index=i, b_index=i) for i in range(len(fa))]
    random.seed(r["shuffle_seed"])
    E, inliers = er.estimate_essential_mat_with_ransac(sc["K"], fa, fb, matches, r["threshold"],
                                                       min_num_extra_inliers=r["min_extra"], max_iterations=r["iterations"],
                                                       solver=solver)
    gap = mc.rotation_gap_of(E, sc["R"])
    print(f"{motion} {solver}: rotation gap {gap!r} with {len(inliers)} inliers, host loop {HOST_ROUTE_GAP[motion, solver]!r}")
    assert gap <= HOST_ROUTE_GAP[motion, solver] + 1e-6
