"""PnP estimator on the MI355X: fit, score, route, batch and end-to-end parity with the NumPy oracle (tests/pnp_oracle.py)."""
import random
from functools import partial

import numpy as np
import pytest
import torch

import pnp_oracle as orc
from structure_from_motion_amd import synthetic
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.feature_matching.matching import Match

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
AGG = {"sum": 0, "square": 1, "mean": 2, "rms": 3}


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _with_behind(pts, fraction, seed):
    """Move a fraction of the points behind camera 1 (and so, for these poses, behind the new view too)."""
    rng = np.random.default_rng(seed)
    pts = pts.copy()
    back = rng.random(len(pts)) < fraction
    pts[back, 2] = -pts[back, 2]
    return pts


def _tables(n, h, seed):
    from structure_from_motion_amd import device

    return device.pyshuffle_table(n, h, random.Random(seed), advance=False)[0]


def _device_fit(pts, S):
    from structure_from_motion_amd import device

    n, h = pts.shape[0], S.shape[0]
    model, flags = device.pnp_fit(device.to_device(pts).reshape(1, n, 5), device.to_device(S, torch.int32).reshape(1, h, 8), K)
    return model.cpu().numpy()[0], flags.cpu().numpy()[0]


def test_fit_parity(dev):
    pts, _, _ = orc.scene(2000, seed=21, K=K, outlier_fraction=0.3, noise_px=0.5)
    h = 20_000
    S = _tables(2000, h, 5)
    model, flags = _device_fit(pts, S)
    checked = 0
    for k in range(h):
        idx = S[k, :6]
        R_o, t_o, ratio = orc.fit(pts[idx, :3], pts[idx, 3:], K)
        assert flags[k] == (0 if ratio >= orc.DEGENERATE_FLOOR else 1), k
        M_cond = np.linalg.svd(R_o, compute_uv=False)
        if ratio < 1e-3 or not np.all(np.isfinite(model[k])):
            continue
        R, t = model[k, :9].reshape(3, 3), model[k, 9:]
        assert np.max(np.abs(R - R_o)) <= 1e-9, (k, np.max(np.abs(R - R_o)))
        assert np.max(np.abs(t - t_o)) <= 1e-9 * max(1.0, np.max(np.abs(t_o))), k
        assert M_cond.min() > 0
        checked += 1
    assert checked > h // 2


def test_fit_flags_coplanar(dev):
    rng = np.random.default_rng(8)
    pts, _, _ = orc.scene(64, seed=22, K=K, outlier_fraction=0.0, noise_px=0.0)
    pts[:6, 2] = 5.0   # the first six points on one plane
    S = np.tile(np.arange(8, dtype=np.int32), (4, 1))
    S[1, :6] = rng.permutation(np.arange(6, 64))[:6]
    _, flags = _device_fit(pts, S)
    assert flags.tolist() == [1, 0, 1, 1]


def _oracle_sums(pts, model, S, thr, sample=6):
    """(cnt, s1, s2) with the device's summation order: survivors and passing sample points in index order, then the sample
    points (the first ``sample`` entries of a row of S) that did not pass, in sample order."""
    h = model.shape[0]
    cnt = np.zeros(h, dtype=np.int32)
    s1, s2 = np.zeros(h), np.zeros(h)
    for k in range(h):
        e = orc.score_values(model[k, :9].reshape(3, 3), model[k, 9:], K, pts)
        with np.errstate(invalid="ignore"):
            passed = e <= thr
        smp = S[k, :sample]
        a1 = np.cumsum(e[passed])[-1] if passed.any() else 0.0
        a2 = np.cumsum(e[passed] * e[passed])[-1] if passed.any() else 0.0
        c = int(np.count_nonzero(passed))
        for i in smp:
            if e[i] <= thr:
                c -= 1
            else:
                with np.errstate(over="ignore", invalid="ignore"):
                    a1 += e[i]
                    a2 += e[i] * e[i]
        cnt[k], s1[k], s2[k] = c, a1, a2
    return cnt, s1, s2


def _close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    finite = np.isfinite(a) & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        ok = same | (finite & (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))))
    return bool(np.all(ok))


@pytest.mark.parametrize("n", [6, 7, 63, 64, 65, 1000, 50_000])
def test_score_parity(dev, n):
    from structure_from_motion_amd import device

    pts, _, _ = orc.scene(n, seed=30 + n % 97, K=K, outlier_fraction=0.3, noise_px=0.5)
    pts = _with_behind(pts, 0.05, n)
    h = 40 if n >= 50_000 else 300
    S = _tables(n, h, n)
    model, _ = _device_fit(pts, S)
    pts_d = device.to_device(pts).reshape(1, n, 5)
    S_d = device.to_device(S, torch.int32).reshape(1, h, 8)
    model_d = device.to_device(model).reshape(1, h, 12)
    for thr in (4.0, 1e300, 0.0, float("nan"), float("inf")):
        cnt, s1, s2 = (a.cpu().numpy()[0] for a in device.pnp_score(pts_d, model_d, S_d, K, thr))
        c_o, s1_o, s2_o = _oracle_sums(pts, model, S, thr)
        assert np.array_equal(cnt, c_o), (thr, np.nonzero(cnt != c_o)[0][:5])
        assert _close(s1, s1_o, 1e-13) and _close(s2, s2_o, 1e-13), thr


TILE, BLOCK = 512, 256   # kScoreTile and kScoreBlock of csrc/sfm_minimal_score.h


@pytest.mark.parametrize("sample", [4, 6])
@pytest.mark.parametrize("h", [1, BLOCK - 1, BLOCK + 1])
@pytest.mark.parametrize("n", ["sample", TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_score_mask_at_tile_and_block_edges(dev, n, h, sample):
    """The scorer and the mask at their own edges, with two different scenes in one call (so the b * n * 5 item stride and
    b * h_count are exercised): one point set that is exactly the sample, one point short of a tile, a full tile, one point
    into the second tile and into the third; one hypothesis, one lane short of a block and one lane into the second.  The
    device's own models on both sides: cnt exact, s1 and s2 within 1e-13 relative (the values are the oracle's bit for bit,
    only the summation order differs), the mask byte-equal to the host rule for the selected winner, all zero over a buffer
    of 7s for a record without a winner, and count 0 everywhere under a NaN threshold."""
    from structure_from_motion_amd import device

    n = sample if n == "sample" else n
    thr = 4.0
    outliers = 0.0 if n == sample else 0.3
    pts = np.stack([orc.scene(n, seed=80 + 2 * (n % 89) + b, K=K, outlier_fraction=outliers, noise_px=0.02)[0] for b in range(2)])
    if n > sample:   # (where every sample is the whole point set, a point behind the camera would leave no winner)
        pts = np.stack([_with_behind(pts[b], 0.05, n + b) for b in range(2)])
    S = np.zeros((2, h, 8), dtype=np.int32)
    for b in range(2):
        rng = np.random.default_rng(1000 * n + 10 * h + b)
        S[b, :, :sample] = np.array([rng.choice(n, sample, replace=False) for _ in range(h)])
    pts_d, S_d = device.to_device(pts), device.to_device(S, torch.int32)
    model_d, flags_d = (device.p3p_fit if sample == 4 else device.pnp_fit)(pts_d, S_d, K)
    model = model_d.cpu().numpy()
    cnt_d, s1_d, s2_d = device.pnp_score(pts_d, model_d, S_d, K, thr, sample_size=sample)
    cnt, s1, s2 = cnt_d.cpu().numpy(), s1_d.cpu().numpy(), s2_d.cpu().numpy()
    for b in range(2):
        c_o, s1_o, s2_o = _oracle_sums(pts[b], model[b], S[b], thr, sample)
        assert np.array_equal(cnt[b], c_o), (b, np.nonzero(cnt[b] != c_o)[0][:5])
        assert _close(s1[b], s1_o, 1e-13) and _close(s2[b], s2_o, 1e-13), b
    min_extra = 0 if n == sample else 10
    result = device.select_best(cnt_d, s1_d, s2_d, flags_d, min_extra, AGG["rms"], sample_size=sample)
    rec = device.read_select(result)
    mask = device.pnp_inlier_mask(pts_d, model_d, S_d, K, result, thr, sample_size=sample).cpu().numpy()
    for b in range(2):
        best = rec[b].best_h
        assert best >= 0 or h == 1, (b, h)
        expected = np.zeros(n, dtype=np.uint8)
        if best >= 0:
            e = orc.score_values(model[b, best, :9].reshape(3, 3), model[b, best, 9:], K, pts[b])
            with np.errstate(invalid="ignore"):
                expected[e <= thr] = 1
            expected[S[b, best, :sample]] = 2
        assert np.array_equal(mask[b], expected), (b, np.nonzero(mask[b] != expected)[0][:5])
    nothing = device.select_best(cnt_d, s1_d, s2_d, flags_d, n + 1, AGG["rms"], sample_size=sample)
    assert all(r.best_h == -1 for r in device.read_select(nothing))
    filled = torch.full((2, n), 7, dtype=torch.uint8, device=pts_d.device)
    device.pnp_inlier_mask(pts_d, model_d, S_d, K, nothing, thr, out=filled, sample_size=sample)
    assert not filled.any()
    assert not device.pnp_score(pts_d, model_d, S_d, K, float("nan"), sample_size=sample)[0].any()


def _pair_data(n, seed, outliers=0.3):
    pts, R, t = orc.scene(n, seed=seed, K=K, outlier_fraction=outliers, noise_px=0.02)   # (a six-point DLT is minimal)
    points = [row[:3].copy() for row in pts]
    feats = [Feature(float(row[3]), float(row[4])) for row in pts]
    return pts, points, feats, R, t


@pytest.mark.parametrize("method", ["sum", "square", "mean", "rms"])
def test_route_parity_pyshuffle(dev, method):
    from structure_from_motion_amd.pnp import pnp
    from structure_from_motion_amd.ransac import ransac

    _, points, feats, R_true, _ = _pair_data(300, seed=41)
    matches = [Match(i, i) for i in range(300)]
    agg = ransac.ErrorAggregationMethod(method)
    for seed in (1, 2):
        random.seed(seed)
        R, t, inliers = pnp.estimate_pose_pnp_with_ransac(K, points, feats, matches, 4.0, min_num_extra_inliers=20,
                                                          error_aggregation_method=agg, max_iterations=150)
        after_device = random.getstate()
        random.seed(seed)
        items = [(points[i], feats[i]) for i in range(300)]
        model, ref = ransac._host_loop(items, 6, partial(orc.fitter, camera_matrix=K), partial(orc.scorer, camera_matrix=K),
                                       4.0, 20, agg, 150)
        assert random.getstate() == after_device   # the global stream advanced exactly as the reference's loop
        assert np.max(np.abs(R - model[0])) <= 1e-9 and np.max(np.abs(t - model[1])) <= 1e-9
        assert len(inliers) == len(ref)
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(inliers, ref))
        assert np.allclose(R, R_true, atol=0.02)


@pytest.mark.parametrize("method", ["sum", "rms"])
def test_route_parity_philox(dev, method, monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.pnp import pnp
    from structure_from_motion_amd.ransac import ransac

    n, h, thr, min_extra = 300, 150, 4.0, 20
    pts, points, feats, _, _ = _pair_data(n, seed=43)
    monkeypatch.setenv("SFM_SAMPLER", "philox")
    monkeypatch.setenv("SFM_SEED", "77")
    R, t, inliers = pnp.estimate_pose_pnp_with_ransac(K, points, feats, [Match(i, i) for i in range(n)], thr,
                                                      min_num_extra_inliers=min_extra,
                                                      error_aggregation_method=ransac.ErrorAggregationMethod(method),
                                                      max_iterations=h)
    S = device.sample_philox(77, 0, h, n).cpu().numpy()[0]
    best, best_err = -1, np.inf
    for k in range(h):
        R_o, t_o, ratio = orc.fit(pts[S[k, :6], :3], pts[S[k, :6], 3:], K)
        e = orc.score_values(R_o, t_o, K, pts)
        sample = np.zeros(n, dtype=bool)
        sample[S[k, :6]] = True
        surv = ~sample & (e <= thr)
        if np.count_nonzero(surv) < min_extra:
            continue
        errs = e[sample | surv]
        err = errs.sum() if method == "sum" else np.sqrt(np.mean(errs * errs))
        if err < best_err:
            best, best_err, best_model, best_order = k, err, (R_o, t_o), np.concatenate([S[k, :6], np.nonzero(surv)[0]])
    assert best >= 0
    assert np.max(np.abs(R - best_model[0])) <= 1e-9 and np.max(np.abs(t - best_model[1])) <= 1e-9
    assert [float(f.x) for _, f in inliers] == [feats[i].x for i in best_order]


def test_batch_equals_single_calls(dev):
    from structure_from_motion_amd import device

    n, h = 500, 256
    views = [orc.scene(n, seed=50 + b, K=K, noise_px=0.02)[0] for b in range(3)]
    tables = [_tables(n, h, 60 + b) for b in range(3)]
    ws = device.PnPWorkspace(3, n, h, dev)
    ws.S.copy_(device.to_device(np.stack(tables), torch.int32))
    ws.run(device.to_device(np.stack(views)), K, 4.0, 10, AGG["rms"])
    for b in range(3):
        one = device.PnPWorkspace(1, n, h, dev)
        one.S.copy_(device.to_device(tables[b], torch.int32).reshape(1, h, 8))
        one.run(device.to_device(views[b]).reshape(1, n, 5), K, 4.0, 10, AGG["rms"])
        for name in ("model", "flags", "cnt", "s1", "s2", "result", "mask"):
            assert torch.equal(getattr(ws, name)[b], getattr(one, name)[0]), (b, name)
        assert one.outcome(0).best_h >= 0
    # philox sampling in the fit launch: view b draws from seed + b * stride
    ws.run(device.to_device(np.stack(views)), K, 4.0, 10, AGG["rms"], philox=(9, 0, 1000))
    for b in range(3):
        assert torch.equal(ws.S[b], device.sample_philox(9 + 1000 * b, 0, h, n)[0])


def test_ops_opcheck(dev):
    from structure_from_motion_amd import device, ops

    op = ops.load()
    n, h = 300, 64
    pts = device.to_device(orc.scene(n, seed=70, K=K)[0]).reshape(1, n, 5)
    S = device.sample_philox(3, 0, h, n)
    Kl = [float(v) for v in K.reshape(9)]
    model, flags = op.pnp_fit(pts, S, Kl)
    torch.library.opcheck(op.pnp_fit.default, (pts, S, Kl))
    torch.library.opcheck(op.pnp_score.default, (pts, model, S, Kl, 4.0))
    torch.library.opcheck(op.pnp_score_.default, (pts, model, S, Kl, 4.0, torch.empty_like(flags), torch.empty_like(model[..., 0]),
                                                  torch.empty_like(model[..., 0])), test_utils=("test_schema", "test_faketensor"))


def test_three_view_end_to_end(dev):
    from apps import sfm_three_view

    out = sfm_three_view.run(n=400, seed=11, outlier_fraction=0.3, noise_px=0.0)
    assert out["R3_error_rad"] < 1e-3, out
    assert out["t3_error"] < 1e-3, out
    assert out["pnp_inliers"] >= 0.6 * out["triangulated"]
