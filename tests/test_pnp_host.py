"""PnP estimator, host side: the NumPy oracle, the host scorer, input validation and the RANSAC routing (no GPU)."""
import random
from functools import partial

import numpy as np
import pytest

import pnp_oracle as orc
from structure_from_motion_amd import synthetic
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.feature_matching.matching import Match
from structure_from_motion_amd.pnp import pnp
from structure_from_motion_amd.ransac import ransac

K = synthetic.BENCH_K


def _items(pts):
    return [(row[:3].copy(), Feature(float(row[3]), float(row[4]))) for row in pts]


def test_oracle_recovers_exact_pose_from_six_points():
    pts, R, t = orc.scene(6, seed=1, K=K, outlier_fraction=0.0, noise_px=0.0)
    R_est, t_est, ratio = orc.fit(pts[:, :3], pts[:, 3:], K)
    assert ratio > 1e-6
    assert np.allclose(R_est, R, atol=1e-9) and np.allclose(t_est, t, atol=1e-9)
    assert abs(np.linalg.det(R_est) - 1.0) < 1e-12


def test_public_host_fitter_matches_oracle():
    pts, R, t = orc.scene(6, seed=2, K=K, outlier_fraction=0.0, noise_px=0.3)
    R_o, t_o, _ = orc.fit(pts[:, :3], pts[:, 3:], K)
    R_h, t_h = pnp.pnp_model_fitter(_items(pts), camera_matrix=K)
    assert np.allclose(R_h, R_o, atol=1e-12) and np.allclose(t_h, t_o, atol=1e-12)
    with pytest.raises(ValueError):
        pnp.pnp_model_fitter(_items(pts)[:5], camera_matrix=K)


@pytest.mark.parametrize("shape", ["coplanar", "collinear"])
def test_coplanar_and_collinear_samples_are_flagged(shape):
    rng = np.random.default_rng(3)
    X = np.column_stack([rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6), np.full(6, 5.0)])
    if shape == "collinear":
        X[:, 1] = 0.3 * X[:, 0]
    R, t = orc.random_pose(rng)
    uvw = (X @ R.T + t) @ K.T
    uv = uvw[:, :2] / uvw[:, 2:3]
    assert orc.fit(X, uv, K)[2] < orc.DEGENERATE_FLOOR
    with pytest.raises(pnp.PnPCalculationError):
        pnp.pnp_model_fitter(_items(np.column_stack([X, uv])), camera_matrix=K)


def test_scorer_infinite_behind_camera_and_bitwise_order():
    R, t = np.eye(3), np.zeros(3)
    assert pnp.calculate_reprojection_score((R, t), (np.array([0.1, 0.2, -3.0]), Feature(300.0, 200.0)), K) == np.inf
    assert pnp.calculate_reprojection_score((R, t), (np.array([0.1, 0.2, 0.0]), Feature(300.0, 200.0)), K) == np.inf
    pts, R, t = orc.scene(200, seed=4, K=K)
    vec = orc.score_values(R, t, K, pts)
    for row, e in zip(pts, vec):
        got = pnp.calculate_reprojection_score((R, t), (row[:3], Feature(row[3], row[4])), camera_matrix=K)
        assert got == orc.score_one(R, t, K, row[:3], row[3], row[4]) == e


def test_input_validation():
    pts, _, _ = orc.scene(20, seed=5, K=K)
    points = [row[:3] for row in pts]
    feats = [Feature(row[3], row[4]) for row in pts]
    with pytest.raises(ValueError, match="six"):
        pnp.estimate_pose_pnp_with_ransac(K, points, feats, [Match(i, i) for i in range(5)], 4.0)
    with pytest.raises(ValueError, match="3x3"):
        pnp.estimate_pose_pnp_with_ransac(K[:2], points, feats, [Match(i, i) for i in range(20)], 4.0)
    K_bad = K.copy()
    K_bad[2, 2] = 2.0
    with pytest.raises(ValueError, match="row 2"):
        pnp.estimate_pose_pnp_with_ransac(K_bad, points, feats, [Match(i, i) for i in range(20)], 4.0)


def test_routing():
    fit = partial(pnp.pnp_model_fitter, camera_matrix=K)
    score = partial(pnp.calculate_reprojection_score, camera_matrix=K)
    spec = ransac._device_spec(fit, score, 6)
    assert isinstance(spec, ransac.DeviceSpec) and spec.solver == "dlt" and np.array_equal(spec.camera_matrix, K)
    assert ransac._device_spec(fit, score, 7) is None
    assert ransac._device_spec(fit, score, 8) is None
    assert ransac._device_spec(fit, partial(pnp.calculate_reprojection_score, camera_matrix=2 * K), 6) is None
    assert ransac._device_spec(partial(orc.fitter, camera_matrix=K), partial(orc.scorer, camera_matrix=K), 6) is None
    assert ransac._device_spec(fit, partial(orc.scorer, camera_matrix=K), 6) is None


def test_untagged_callables_take_host_loop(monkeypatch):
    """Untagged callables (and a tagged pair with another sample size) run _host_loop and never touch the device."""
    from structure_from_motion_amd.ransac import _device_route

    def no_device(*args, **kwargs):
        raise AssertionError("device route taken")

    monkeypatch.setattr(_device_route, "ransac_on_device", no_device)
    pts, R, t = orc.scene(60, seed=6, K=K, outlier_fraction=0.2, noise_px=0.2)
    items = _items(pts)
    random.seed(3)
    model, inliers = ransac.fit_with_ransac(items, 6, partial(orc.fitter, camera_matrix=K),
                                            partial(orc.scorer, camera_matrix=K), 4.0, max_iterations=50)
    random.seed(3)
    ref = ransac._host_loop(items, 6, partial(orc.fitter, camera_matrix=K), partial(orc.scorer, camera_matrix=K), 4.0, 0,
                            ransac.ErrorAggregationMethod.RMS, 50)
    assert np.array_equal(model[0], ref[0][0]) and len(inliers) == len(ref[1])
    assert np.allclose(model[0], R, atol=0.05)
    with pytest.raises(ValueError, match="Six"):   # tagged pair, 7 items per sample: host loop, fitter refuses
        ransac.fit_with_ransac(items, 7, partial(pnp.pnp_model_fitter, camera_matrix=K),
                               partial(pnp.calculate_reprojection_score, camera_matrix=K), 4.0, max_iterations=5)
