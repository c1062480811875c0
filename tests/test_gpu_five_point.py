"""The five-point essential-matrix path on the GPU: device fit vs the host definition, candidates, six-item scoring,
selection and mask, the public route, heavy outliers and planar scenes."""
import random

import numpy as np
import pytest
import torch

from structure_from_motion_amd import device, synthetic
from structure_from_motion_amd._native import AGG_MEAN, AGG_RMS, AGG_SQUARE, AGG_SUM
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.epipolar import epipolar_ransac as er
from structure_from_motion_amd.epipolar import five_point as fp
from structure_from_motion_amd.epipolar.eight_point import EightPointCalculationError
from structure_from_motion_amd.feature_matching.matching import Match
from structure_from_motion_amd.ransac import ransac

pytestmark = pytest.mark.gpu


def _scene(n=400, seed=6, outliers=0.3, noise=0.5):
    pa, pb, K, R, t, is_out = synthetic.two_view_scene(n, seed=seed, outlier_fraction=outliers, noise_px=noise)
    corr = device.normalize_correspondences(device.to_device(pa), device.to_device(pb), K)
    return pa, pb, K, R, t, is_out, corr


def _item5_sed(E, corr_np, S):
    q = corr_np[S[:, 5]]
    return fp.sed_value([E[:, i] for i in range(9)], q[:, 0], q[:, 1], q[:, 2], q[:, 3])


def _fit_parity(corr_np, S, E_dev, flags_dev, either_sign=False):
    """``either_sign``: E and -E count as equal.  Where the two largest-magnitude entries of E tie (every pure translation:
    [t]x is antisymmetric), rounding decides which of them the solver makes positive, and the SED is the same for both."""
    def gap(a, b):
        d = np.abs(a - b).max(-1)
        return np.minimum(d, np.abs(a + b).max(-1)) if either_sign else d

    E_host, flags_host = fp.fit_corr(corr_np, S)
    assert np.array_equal(flags_dev, flags_host)
    ok = flags_host == 0
    both_nan = np.isnan(E_dev).all(1) & np.isnan(E_host).all(1)
    diff = gap(E_dev, E_host)
    same = both_nan | (diff <= 1e-9)
    # Near-tie rule: where the picks differ, the device pick is a host candidate (to 1e-6) and the two picks' SEDs on item 5
    # tie to within what the candidates' own error moves them (1e-6 relative, or 1e-12 absolute near zero)
    cands, _ = fp.candidates_corr(corr_np, S)
    sed_dev, sed_host = _item5_sed(E_dev, corr_np, S), _item5_sed(E_host, corr_np, S)
    for h in np.nonzero(ok & ~same)[0]:
        d = np.nanmin(gap(cands[h], E_dev[h]))
        assert d <= 1e-6, (h, d)
        assert abs(sed_dev[h] - sed_host[h]) <= 1e-6 * max(sed_dev[h], sed_host[h]) + 1e-12, (h, sed_dev[h], sed_host[h])
    assert np.mean(same[ok]) >= 0.99


def test_fit_parity_pyshuffle():
    *_, corr = _scene()
    n = corr.shape[0]
    table = device.PyShuffleTable(n, 2000, random.Random(4), advance=False)
    S = device.to_device(table.S, dtype=torch.int32).reshape(1, 2000, 8)
    E, flags = device.five_point_fit(corr.reshape(1, n, 4), S)
    _fit_parity(corr.cpu().numpy(), table.S, E.cpu().numpy()[0], flags.cpu().numpy()[0])


@pytest.mark.parametrize("n", [6, 7, 300])
def test_fit_parity_philox(n):
    *_, corr = _scene(n=max(n, 8))
    corr = corr[:n].contiguous()
    S = torch.empty((1, 1000, 8), dtype=torch.int32, device=corr.device)
    E, flags = device.five_point_fit(corr.reshape(1, n, 4), S, philox=(99, 0, 1))
    S_np = S.cpu().numpy()[0]
    if n >= 8:
        assert np.array_equal(S_np, device.sample_philox(99, 0, 1000, n).cpu().numpy()[0])
    else:
        assert (S_np[:, n:] == -1).all()
    _fit_parity(corr.cpu().numpy(), S_np, E.cpu().numpy()[0], flags.cpu().numpy()[0])


def test_candidates_match_host():
    *_, corr = _scene()
    n = corr.shape[0]
    table = device.PyShuffleTable(n, 500, random.Random(8), advance=False)
    S = device.to_device(table.S, dtype=torch.int32).reshape(1, 500, 8)
    out, count = device.five_point_candidates(corr.reshape(1, n, 4), S)
    cands, cnt_host = fp.candidates_corr(corr.cpu().numpy(), table.S)
    count = count.cpu().numpy()[0]
    out = out.cpu().numpy()[0]
    assert np.mean(count == cnt_host) >= 0.99
    for h in np.nonzero(count == cnt_host)[0]:
        if cnt_host[h] > 0:
            assert np.abs(out[h, :count[h]] - cands[h, :count[h]]).max() <= 1e-6


def _host_scores(corr_np, E, S, thr, k=6):
    H = E.shape[0]
    cnt = np.zeros(H, np.int64)
    s1 = np.zeros(H)
    s2 = np.zeros(H)
    for h in range(H):
        sed = fp.sed_value(list(E[h]), corr_np[:, 0], corr_np[:, 1], corr_np[:, 2], corr_np[:, 3])
        in_sample = np.zeros(len(corr_np), bool)
        in_sample[S[h, :k]] = True
        ok = (sed <= thr) & ~in_sample
        cnt[h] = ok.sum()
        s1[h] = sed[ok].sum() + sed[in_sample].sum()
        s2[h] = (sed[ok] ** 2).sum() + (sed[in_sample] ** 2).sum()
    return cnt, s1, s2


def test_score_select_mask_six_items():
    *_, corr = _scene(n=500)
    n, H, thr = corr.shape[0], 300, 2e-5
    table = device.PyShuffleTable(n, H, random.Random(2), advance=False)
    S = device.to_device(table.S, dtype=torch.int32).reshape(1, H, 8)
    E, flags = device.five_point_fit(corr.reshape(1, n, 4), S)
    cnt, s1, s2 = device.score_sed(corr.reshape(1, n, 4), E, S, thr, sample_size=6)
    corr_np, E_np = corr.cpu().numpy(), E.cpu().numpy()[0]
    c_ref, s1_ref, s2_ref = _host_scores(corr_np, E_np, table.S, thr)
    assert np.array_equal(cnt.cpu().numpy()[0], c_ref)
    fin = np.isfinite(s1_ref)
    assert np.allclose(s1.cpu().numpy()[0][fin], s1_ref[fin], rtol=1e-12, atol=0)
    for agg in (AGG_SUM, AGG_SQUARE, AGG_MEAN, AGG_RMS):
        res = device.select_best(cnt, s1, s2, flags, 10, agg, sample_size=6)
        rec = device.read_select(res)[0]
        err = {AGG_SUM: s1_ref, AGG_SQUARE: s2_ref, AGG_MEAN: s1_ref / (c_ref + 6),
               AGG_RMS: np.sqrt(s2_ref / (c_ref + 6))}[agg]
        gated = (c_ref >= 10) & (flags.cpu().numpy()[0] == 0) & np.isfinite(err)
        best = int(np.argmin(np.where(gated, err, np.inf))) if gated.any() else -1
        if best >= 0 and rec.best_h != best:   # summation-order ties only
            assert abs(err[rec.best_h] - err[best]) <= 1e-12 * abs(err[best])
        else:
            assert rec.best_h == best
        mask = device.inlier_mask(corr.reshape(1, n, 4), E, S, res, thr, sample_size=6).cpu().numpy()[0]
        if rec.best_h >= 0:
            h = rec.best_h
            assert (mask[table.S[h, :6]] == 2).all() and (mask == 2).sum() == 6
            assert (mask == 1).sum() == c_ref[h]


def _features(pix):
    return [Feature(float(x), float(y)) for x, y in pix]


def test_public_route_equals_host_loop():
    pa, pb, K, R, t, is_out, _ = _scene(n=200)
    fa, fb = _features(pa), _features(pb)
    matches = [Match(a_index=i, b_index=i) for i in range(len(fa))]
    random.seed(5)
    E_dev, inl_dev = er.estimate_essential_mat_with_ransac(K, fa, fb, matches, 2e-5, min_num_extra_inliers=20,
                                                           max_iterations=200, solver="five_point")
    random.seed(5)
    from functools import partial

    pairs = [(fa[i], fb[i]) for i in range(len(fa))]
    E_host, inl_host = ransac._host_loop(pairs, 6, partial(er.five_point_model_fitter, camera_matrix=K),
                                         partial(er.calculate_sed_inlier_score, camera_matrix=K), 2e-5, 20,
                                         ransac.ErrorAggregationMethod.RMS, 200)
    assert np.abs(E_dev - E_host).max() <= 1e-9
    assert [(p[0].x, p[0].y) for p in inl_dev] == [(p[0].x, p[0].y) for p in inl_host]


def _rotation_error(E, corr_in, R_true):
    poses, status = device.decompose_essential(device.to_device(np.asarray(E).reshape(1, 9)))
    best = np.inf
    for p in poses.cpu().numpy()[0]:
        Rp = p[:9].reshape(3, 3)
        c = (np.trace(Rp.T @ R_true) - 1.0) / 2.0
        best = min(best, float(np.arccos(np.clip(c, -1.0, 1.0))))
    return best


def test_heavy_outliers():
    pa, pb, K, R, t, is_out, corr = _scene(n=2000, seed=3, outliers=0.7, noise=0.3)
    fa, fb = _features(pa), _features(pb)
    matches = [Match(a_index=i, b_index=i) for i in range(len(fa))]
    results = {}
    for solver in ("five_point", "eight_point"):
        random.seed(11)
        try:
            E, inl = er.estimate_essential_mat_with_ransac(K, fa, fb, matches, 1e-6, min_num_extra_inliers=300,
                                                           max_iterations=6000, solver=solver)
            results[solver] = _rotation_error(E, None, R)
        except ValueError:
            results[solver] = None
    # measured on an MI355X: five point 0.043 rad (the unrefined model of a noisy minimal sample); eight point finds no
    # hypothesis with 300 extra inliers in the same 6000 and raises ValueError
    print("rotation error at 70 % outliers, 6000 hypotheses:", results)
    assert results["five_point"] is not None and results["five_point"] <= 0.1


def test_planar_scene():
    pa, pb, K, R, t, is_out, plane = synthetic.planar_two_view_scene(600, seed=2, outlier_fraction=0.0, noise_px=0.0)
    fa, fb = _features(pa), _features(pb)
    matches = [Match(a_index=i, b_index=i) for i in range(len(fa))]
    random.seed(1)
    with pytest.raises(EightPointCalculationError):
        er.estimate_essential_mat_with_ransac(K, fa, fb, matches, 1e-8, max_iterations=100)
    random.seed(1)
    E, inl = er.estimate_essential_mat_with_ransac(K, fa, fb, matches, 1e-8, max_iterations=100, solver="five_point")
    corr = device.normalize_correspondences(device.to_device(pa), device.to_device(pb), K)
    sed = device.sed_values(corr, device.to_device(E.reshape(9))).cpu().numpy()
    assert np.max(sed) <= 1e-18
    pa, pb, K, R, t, is_out, plane = synthetic.planar_two_view_scene(1000, seed=4, outlier_fraction=0.3, noise_px=0.5)
    fa, fb = _features(pa), _features(pb)
    random.seed(2)
    E, inl = er.estimate_essential_mat_with_ransac(K, fa, fb, [Match(a_index=i, b_index=i) for i in range(len(fa))], 2e-5,
                                                   max_iterations=500, solver="five_point")
    kept = {(p[0].x, p[0].y) for p in inl}
    true_in = [(fa[i].x, fa[i].y) for i in np.nonzero(~is_out)[0]]
    assert np.mean([p in kept for p in true_in]) >= 0.95


def test_batch_equals_single():
    corrs = []
    for seed in (1, 2, 3):
        *_, corr = _scene(n=300, seed=seed)
        corrs.append(corr)
    C = torch.stack(corrs)
    ws = device.RansacWorkspace(3, 300, 400)
    ws.run(C, 2e-5, 10, AGG_RMS, philox=(7, 0, 1), solver="five_point")
    for b in range(3):
        one = device.RansacWorkspace(1, 300, 400)
        one.run(C[b:b + 1].contiguous(), 2e-5, 10, AGG_RMS, philox=(7 + b, 0, 1), solver="five_point")
        o1, ob = one.outcome(0), ws.outcome(b)
        assert o1.best_h == ob.best_h and np.array_equal(o1.mask, ob.mask)
        assert np.array_equal(np.nan_to_num(o1.E), np.nan_to_num(ob.E)) and len(ob.sample) == 6


def _buffers(ws):
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (ws.S, ws.E, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask)]


def test_eight_point_run_unchanged():
    # an eight-point pass, a five-point pass on the same buffers, the eight-point pass again: bit for bit the first one, and the
    # same winner, E and mask as the separate eight-point calls
    *_, corr = _scene(n=500)
    c = corr.reshape(1, 500, 4)
    ws = device.RansacWorkspace(1, 500, 1000)
    ws.run(c, 2e-5, 10, AGG_RMS, philox=(3, 0, 1))
    first = _buffers(ws)
    ws.run(c, 2e-5, 10, AGG_RMS, philox=(3, 0, 1), solver="five_point")
    five = _buffers(ws)
    assert ws.outcome(0).sample.shape == (6,)
    ws.run(c, 2e-5, 10, AGG_RMS, philox=(3, 0, 1))
    again = _buffers(ws)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert not np.array_equal(first[1], five[1])   # the five-point pass did write the buffers in between
    assert len(ws.outcome(0).sample) == 8
    S = first[0]
    E, flags = device.fit_eight_point(c, device.to_device(S, dtype=torch.int32))
    cnt, s1, s2 = device.score_sed(c, E, device.to_device(S, dtype=torch.int32), 2e-5, exact_only=True)
    res = device.select_best(cnt, s1, s2, flags, 10, AGG_RMS)
    mask = device.inlier_mask(c, E, device.to_device(S, dtype=torch.int32), res, 2e-5)
    rec, rec_ws = device.read_select(res)[0], device.read_select(ws.result)[0]
    assert rec.best_h == rec_ws.best_h and rec.best_cnt == rec_ws.best_cnt
    assert np.array_equal(E.cpu().numpy(), first[1]) and np.array_equal(mask.cpu().numpy(), first[7])


def test_nan_models_never_gate_nor_win():
    *_, corr = _scene(n=400)
    n, H, thr = 400, 256, 2e-5
    c = corr.reshape(1, n, 4)
    S = device.sample_philox(12, 0, H, n)
    E, flags = device.five_point_fit(c, S)
    E[0, ::2] = float("nan")              # every other hypothesis: the model of a sample without a real solution
    flags.zero_()
    cnt, s1, s2 = device.score_sed(c, E, S, thr, sample_size=6)
    assert (cnt.cpu().numpy()[0, ::2] == 0).all()
    for agg in (AGG_SUM, AGG_SQUARE, AGG_MEAN, AGG_RMS):
        rec = device.read_select(device.select_best(cnt, s1, s2, flags, 0, agg, sample_size=6))[0]
        assert rec.best_h >= 0 and rec.best_h % 2 == 1, (agg, rec.best_h)
    E[0, 1::2] = float("nan")             # nothing but NaN models: no winner, an all-zero mask
    cnt, s1, s2 = device.score_sed(c, E, S, thr, sample_size=6)
    for agg in (AGG_SUM, AGG_SQUARE, AGG_MEAN, AGG_RMS):
        res = device.select_best(cnt, s1, s2, flags, 0, agg, sample_size=6)
        assert device.read_select(res)[0].best_h == -1
        assert not device.inlier_mask(c, E, S, res, thr, sample_size=6).cpu().numpy().any()


@pytest.mark.parametrize("n", [6, 7])
def test_public_route_philox_small_n(n, monkeypatch):
    pa, pb, K, R, t, is_out, _ = _scene(n=8, outliers=0.0, noise=0.0)
    fa, fb = _features(pa[:n]), _features(pb[:n])
    monkeypatch.setenv("SFM_SAMPLER", "philox")
    monkeypatch.setenv("SFM_SEED", "17")
    E, inl = er.estimate_essential_mat_with_ransac(K, fa, fb, [Match(a_index=i, b_index=i) for i in range(n)], 1e-8,
                                                   max_iterations=50, solver="five_point")
    assert len(inl) >= 6 and not np.isnan(E).any()
    keep = [i for i in range(n) if (fa[i].x, fa[i].y) in {(p[0].x, p[0].y) for p in inl}]
    corr = device.normalize_correspondences(device.to_device(pa[keep]), device.to_device(pb[keep]), K)
    assert np.max(device.sed_values(corr, device.to_device(E.reshape(9))).cpu().numpy()) <= 1e-18


def test_five_point_ops_opcheck():
    from structure_from_motion_amd import ops

    op = ops.load()
    *_, corr = _scene(n=300)
    c = corr.reshape(1, 300, 4)
    S = device.sample_philox(4, 0, 64, 300)
    torch.library.opcheck(op.five_point_fit.default, (c, S))
    E, flags = op.five_point_fit(c, S)
    torch.library.opcheck(op.five_point_fit_.default, (c, S, torch.empty_like(E), torch.empty_like(flags)),
                          test_utils=("test_schema", "test_faketensor"))
    ws = device.RansacWorkspace(1, 300, 64)
    args = (c, 5, 1, True, 0, 2e-5, 10.0, AGG_RMS, ws.S, ws.E, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask)
    torch.library.opcheck(op.five_point_ransac_pass_.default, args, test_utils=("test_schema", "test_faketensor"))
    assert "five_point_fit" in ops.FUNCTIONAL_OPS and "five_point_fit_" in ops.INPLACE_OPS
    assert "five_point_ransac_pass_" in ops.INPLACE_OPS


def test_multi_view_app_with_five_point_seed():
    from apps import sfm_multi_view

    eight = sfm_multi_view.run(pnp_solver="p3p")
    five = sfm_multi_view.run(pnp_solver="p3p", e_solver="five_point")
    print("max rotation error: eight point", max(eight["rotation_error_rad"].values()), "five point",
          max(five["rotation_error_rad"].values()))
    assert five["views_registered"] == 8 == eight["views_registered"]
    assert max(five["rotation_error_rad"].values()) <= max(eight["rotation_error_rad"].values()) + 2e-3
    assert max(five["translation_error"].values()) <= max(eight["translation_error"].values()) + 2e-2


def test_three_view_app_with_five_point_seed():
    from apps import sfm_three_view

    eight = sfm_three_view.run()
    five = sfm_three_view.run(e_solver="five_point")
    print("three-view app R2 / R3 error: eight point", eight["R2_error_rad"], eight["R3_error_rad"], "five point",
          five["R2_error_rad"], five["R3_error_rad"])
    assert five["R2_error_rad"] <= eight["R2_error_rad"] + 1e-3
    assert five["R3_error_rad"] <= eight["R3_error_rad"] + 1e-3


def test_bad_sample_size_is_refused():
    *_, corr = _scene(n=100)
    S = torch.zeros((1, 4, 8), dtype=torch.int32, device=corr.device)
    E = torch.zeros((1, 4, 9), dtype=torch.float64, device=corr.device)
    with pytest.raises(Exception):
        device.score_sed(corr.reshape(1, 100, 4), E, S, 1e-5, sample_size=7)
    with pytest.raises(ValueError):
        device.RansacWorkspace(1, 100, 4).run(corr.reshape(1, 100, 4), 1e-5, 0, AGG_RMS, solver="four_point")
