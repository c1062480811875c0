"""Host tests of the five-point solver (structure_from_motion_amd/epipolar/five_point.py) against the action-matrix oracle,
and of the routing of estimate_essential_mat_with_ransac(solver="five_point").  No GPU needed."""
import random
from functools import partial

import numpy as np
import pytest

import five_point_oracle as orc
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.epipolar import epipolar_ransac as er
from structure_from_motion_amd.epipolar import five_point as fp
from structure_from_motion_amd.epipolar.eight_point import EightPointCalculationError
from structure_from_motion_amd.feature_matching.matching import Match
from structure_from_motion_amd.ransac import ransac


def _rotation(w):
    th = np.linalg.norm(w)
    k = w / th
    W = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * W + (1.0 - np.cos(th)) * (W @ W)


def samples(m, seed, planar=False):
    """m noise-free six-item samples: (a (m,6,2), b (m,6,2), true E (m,9))."""
    rng = np.random.default_rng(seed)
    A, B, Es = [], [], []
    for _ in range(m):
        R = _rotation(rng.normal(size=3) * 0.2)
        t = rng.normal(size=3)
        X = rng.uniform(-1.0, 1.0, (6, 3))
        if planar:
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            nrm *= np.sign(nrm[2])
            X[:, 2] = (5.0 * nrm[2] - nrm[0] * X[:, 0] - nrm[1] * X[:, 1]) / max(nrm[2], 0.5)
        else:
            X[:, 2] += 5.0
        Y = X @ R.T + t
        A.append(X[:, :2] / X[:, 2:])
        B.append(Y[:, :2] / Y[:, 2:])
        Es.append(orc.true_essential(R, t))
    return np.array(A), np.array(B), np.array(Es)


def _residuals(E, a, b):
    """Max over the candidates of |b^T E a| on the five items, |det E| and the trace constraint (E normalised to sqrt 2)."""
    E = E.reshape(3, 3)
    ah = np.column_stack([a, np.ones(len(a))])
    bh = np.column_stack([b, np.ones(len(b))])
    epi = np.max(np.abs(np.einsum("ij,jk,ik->i", bh, E, ah)))
    trace = np.max(np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E))
    return epi, abs(np.linalg.det(E)), trace


@pytest.mark.parametrize("planar", [False, True])
def test_true_essential_is_a_candidate(planar):
    a, b, Et = samples(1000, 1 + planar, planar)
    cands, count, degenerate, _ = fp.solve(a[:, :5], b[:, :5])
    assert not degenerate.any()
    err = np.nanmin(np.abs(cands - Et[:, None, :]).max(axis=2), axis=1)
    # measured over these 1000 samples: 95 % (planar) to 99 % (general) within 1e-9, 98.8 % / 99.5 % within 1e-6; the rest
    # are samples with nearly coincident roots of the degree-10 polynomial, where the polished root loses digits
    assert np.mean(err <= 1e-9) >= 0.94
    assert np.mean(err <= 1e-6) >= 0.98


@pytest.mark.parametrize("planar", [False, True])
def test_candidate_counts_match_the_oracle(planar):
    a, b, _ = samples(300, 11 + planar, planar)
    cands, count, _, _ = fp.solve(a[:, :5], b[:, :5])
    agree = close = 0
    for i in range(len(a)):
        ref = orc.solve(a[i, :5], b[i, :5])
        agree += len(ref) == count[i]
        if len(ref) == count[i]:
            d = max(np.min(np.abs(cands[i, :count[i]] - e).max(axis=1)) for e in ref) if ref else 0.0
            close += d <= 1e-6
    # counts agree on every sample but a near-double root or two; the candidates of 97 % of the samples agree to 1e-6
    assert agree >= 0.99 * len(a)
    assert close >= 0.97 * len(a)


def test_candidates_satisfy_the_constraints():
    a, b, _ = samples(2000, 21)
    cands, count, _, _ = fp.solve(a[:, :5], b[:, :5])
    r = np.array([_residuals(cands[i, k], a[i, :5], b[i, :5]) for i in range(len(a)) for k in range(count[i])])
    # epipolar residual, |det E| and the trace constraint of E with ||E||_F = sqrt(2).  Measured over these 2000 samples
    # (9792 candidates): the epipolar residual is at rounding level for every candidate (max 4e-15, the null basis is
    # orthonormal); det and trace have medians 3e-16 / 5e-16 and 98.3 % of the candidates are within 1e-10 / 1e-9; the tail
    # (at most 5e-3) comes from roots of nearly double multiplicity, where Newton's method converges slowly
    assert np.max(r[:, 0]) <= 1e-13
    assert np.mean(np.all(r <= [1e-10, 1e-10, 1e-9], axis=1)) >= 0.98


def test_candidates_come_in_ascending_root_order_and_normalised():
    a, b, _ = samples(200, 31)
    cands, count, _, _ = fp.solve(a[:, :5], b[:, :5])
    for i in range(len(a)):
        for k in range(count[i]):
            e = cands[i, k]
            assert abs(np.linalg.norm(e) - np.sqrt(2.0)) <= 1e-12
            assert e[np.argmax(np.abs(e))] > 0


def test_collinear_and_duplicate_samples_are_flagged_coplanar_not():
    a, b, _ = samples(50, 41)
    col_a, col_b = a.copy(), b.copy()
    s = np.linspace(-0.3, 0.3, 6)
    col_a[:, :, 0], col_a[:, :, 1] = s, 0.5 * s + 0.1          # 3-D points on a line: collinear in both images
    col_b[:, :, 0], col_b[:, :, 1] = 0.9 * s + 0.05, -0.2 * s
    _, _, deg, _ = fp.solve(col_a[:, :5], col_b[:, :5])
    assert deg.all()
    dup_a, dup_b = a.copy(), b.copy()
    dup_a[:, 1], dup_b[:, 1] = dup_a[:, 0], dup_b[:, 0]
    _, _, deg, _ = fp.solve(dup_a[:, :5], dup_b[:, :5])
    assert deg.all()
    pa, pb, _ = samples(50, 42, planar=True)
    _, _, deg, _ = fp.solve(pa[:, :5], pb[:, :5])
    assert not deg.any()
    with pytest.raises(fp.FivePointCalculationError):
        fp.five_point(col_a[0], col_b[0])
    assert issubclass(fp.FivePointCalculationError, EightPointCalculationError)


def test_no_solution_gives_nan_and_is_never_selected():
    # search random correspondences for samples without any real solution
    rng = np.random.default_rng(51)
    a = rng.uniform(-0.5, 0.5, (400, 6, 2))
    b = rng.uniform(-0.5, 0.5, (400, 6, 2))
    _, count, deg, E = fp.solve(a[:, :5], b[:, :5], np.concatenate([a[:, 5], b[:, 5]], axis=1))
    none = np.nonzero((count == 0) & ~deg)[0]
    assert len(none) > 0
    assert np.isnan(E[none]).all()
    i = none[0]
    pairs = [(Feature(*a[i, k]), Feature(*b[i, k])) for k in range(6)]
    K = np.eye(3)
    model = er.five_point_model_fitter(pairs, K)
    assert np.isnan(model).all()
    # the host RANSAC loop: a NaN model neither gates nor wins
    random.seed(3)
    def sed(e, pair):
        return float(fp.sed_value(np.ravel(e), pair[0].x, pair[0].y, pair[1].x, pair[1].y))

    got, inl = ransac._host_loop(pairs, 6, lambda s: np.full((3, 3), np.nan), sed, 1e-3, 0, ransac.ErrorAggregationMethod.RMS, 5)
    assert got is None and inl == []


def test_routing_and_argument_errors():
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    fit = partial(er.five_point_model_fitter, camera_matrix=K)
    score = partial(er.calculate_sed_inlier_score, camera_matrix=K)
    spec = ransac._device_spec(fit, score, 6)
    assert isinstance(spec, ransac.DeviceSpec) and spec.solver == "five_point" and np.array_equal(spec.camera_matrix, K)
    assert ransac._device_spec(fit, score, 8) is None
    assert ransac._device_spec(fit, partial(er.calculate_sed_inlier_score, camera_matrix=2 * K), 6) is None
    eight = ransac._device_spec(partial(er.eight_point_model_fitter, camera_matrix=K), score, 8)
    assert isinstance(eight, ransac.DeviceSpec) and eight.solver == "eight_point" and np.array_equal(eight.camera_matrix, K)
    feats = [Feature(float(i), float(i * i % 7)) for i in range(5)]
    matches = [Match(a_index=i, b_index=i) for i in range(5)]
    with pytest.raises(ValueError, match="solver"):
        er.estimate_essential_mat_with_ransac(K, feats, feats, matches, 1e-3, solver="seven_point")
    with pytest.raises(ValueError, match="Six feature pairs"):
        er.estimate_essential_mat_with_ransac(K, feats, feats, matches, 1e-3, solver="five_point")
    from lib.epipolar.epipolar_ransac import five_point_model_fitter

    assert five_point_model_fitter is er.five_point_model_fitter


def test_host_fitter_picks_the_true_solution():
    a, b, Et = samples(200, 61)
    item5 = np.concatenate([a[:, 5], b[:, 5]], axis=1)
    _, _, _, E = fp.solve(a[:, :5], b[:, :5], item5)
    err = np.abs(E - Et).max(axis=1)
    assert np.mean(err <= 1e-8) >= 0.98


def test_local_optimisation_is_refused_for_five_point(monkeypatch):
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    feats = [Feature(float(i), float(i * i % 7)) for i in range(10)]
    matches = [Match(a_index=i, b_index=i) for i in range(10)]
    monkeypatch.setenv("SFM_LOCAL_OPTIMIZATION", "2")
    # raised before any device work: this test runs without a GPU
    with pytest.raises(ValueError, match="SFM_LOCAL_OPTIMIZATION"):
        er.estimate_essential_mat_with_ransac(K, feats, feats, matches, 1e-3, solver="five_point")
