"""Homography RANSAC and the two-view model choice on the MI355X against the NumPy definition (tests/homography_oracle.py):
fit, score, selection, mask, the Philox route, the public route, the model choice, and the other passes left untouched."""
import random

import numpy as np
import pytest
import torch

import homography_oracle as ho
from structure_from_motion_amd import synthetic
from structure_from_motion_amd.feature_matching.matching import Match

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
THR = 2e-5
TILE = 512   # kScoreTile of csrc/sfm_minimal_score.h


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _tables(n, h, seed):
    from structure_from_motion_amd import device

    return device.PyShuffleTable(n, h, random.Random(seed), advance=False).S


def _upload(corr, S):
    """corr (B, n, 4), S (B, h, 8) -> device tensors."""
    from structure_from_motion_amd import device

    return device.to_device(corr), device.to_device(S, torch.int32)


@pytest.mark.parametrize("motion", ["plane_bench", "bench"])
def test_fit_parity(dev, motion):
    """Flags equal the oracle's; per unflagged sample max |H_dev - H_ref| <= max(1e-9, 1e-13 / (sigma_8 / sigma_1)): rounding
    1e-16 times an unconditioning factor of at most about 1e3, divided by the gap of the null vector (1e-9 is the project's
    P3P parity bound); up to sign where |det H_ref| <= 1e-9.  20 000 shuffle samples plus the two hand-made ones: the last
    64-lane block of the fit launch is partial."""
    from structure_from_motion_amd import device

    n, h = 2000, 20_000
    sc = ho.motion_scene(motion, n, 21, 0.5, 0.3)
    corr = np.vstack([sc["corr"], ho.COLLINEAR_A, ho.REPEATED])
    S = np.zeros((h + 2, 8), dtype=np.int32)
    S[:h] = _tables(n, h, 5)
    S[h, :4] = n + np.arange(4)
    S[h + 1, :4] = n + 4 + np.arange(4)
    assert (h + 2) % 64 != 0
    c, s = _upload(corr[None], S[None])
    H_dev, flags_dev = (t.cpu().numpy()[0] for t in device.homography_fit(c, s))
    H_ref, flags_ref, ratio = ho.fit(corr, S)
    assert flags_ref[h] == 0 and flags_ref[h + 1] == 1
    assert np.array_equal(flags_dev, flags_ref), np.nonzero(flags_dev != flags_ref)[0][:10]
    ok = flags_ref == 0
    print(f"{motion}: ratio min {np.nanmin(ratio[ok]):.3g}, 1st percentile {np.percentile(ratio[ok], 1):.3g}, flagged {int((~ok).sum())}")
    bound = np.maximum(1e-9, 1e-13 / ratio[ok])
    plain = np.max(np.abs(H_dev[ok] - H_ref[ok]), axis=1)
    flipped = np.max(np.abs(H_dev[ok] + H_ref[ok]), axis=1)
    gap = np.where(np.abs(ho.det(H_ref[ok])) <= 1e-9, np.minimum(plain, flipped), plain)
    worst = int(np.argmax(gap / bound))
    print(f"{motion}: worst gap / bound {gap[worst] / bound[worst]:.3g} (gap {gap[worst]:.3g}, ratio {ratio[ok][worst]:.3g})")
    assert (gap <= bound).all(), (gap[worst], bound[worst])
    assert np.all(ho.det(H_dev[ok]) >= 0.0)
    assert np.abs(np.sqrt(np.sum(H_dev[ok] ** 2, axis=1)) - 1.0).max() <= 1e-14


def _score_case(n, h, seed):
    """Two different scenes (outlier-free at n = 4, where every sample is the whole data set) and distinct samples."""
    outliers = 0.0 if n == 4 else 0.3
    corr = np.stack([ho.motion_scene("plane_bench", n, seed, 0.5, outliers)["corr"],
                     ho.motion_scene("pan10", n, seed + 1, 0.5, outliers)["corr"]])
    S = np.zeros((2, h, 8), dtype=np.int32)
    for b in range(2):
        rng = np.random.default_rng(1000 * seed + b)
        S[b, :, :4] = np.array([rng.choice(n, 4, replace=False) for _ in range(h)])
    return corr, S


def _through_infinity(corr, S):
    """For each entry a model (9,) that maps sample item 3 of hypothesis 0 through the line at infinity: p2 = -1 there."""
    out = []
    for b in range(corr.shape[0]):
        xa, ya = corr[b, S[b, 0, 3], :2]
        H = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -2.0 * xa / (xa * xa + ya * ya), -2.0 * ya / (xa * xa + ya * ya), 1.0])
        out.append(H / np.linalg.norm(H))
    return np.stack(out)


@pytest.mark.parametrize("h", [1, 255, 257])
@pytest.mark.parametrize("n", [4, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_score_selection_mask(dev, n, h):
    """The device's own H on both sides: cnt exact, s1 and s2 within 1e-13 relative (the values are the definition's bit for
    bit, only the summation order differs: n eps at most), the selection equal to the host rule for the four aggregation
    methods, the mask byte-equal, and all zero when nothing qualifies."""
    from structure_from_motion_amd import device

    corr, S = _score_case(n, h, 3 + n % 7)
    c, s = _upload(corr, S)
    H_t, flags_t = device.homography_fit(c, s)
    H_t[:, 0] = device.to_device(_through_infinity(corr, S))   # hypothesis 0: a sample item with e = +inf
    H = H_t.cpu().numpy()
    flags = flags_t.cpu().numpy()
    cnt_t, s1_t, s2_t = device.homography_score(c, H_t, s, THR)
    cnt, s1, s2 = cnt_t.cpu().numpy(), s1_t.cpu().numpy(), s2_t.cpu().numpy()
    min_extra = 0 if n == 4 else 10
    for b in range(2):
        cnt_ref, s1_ref, s2_ref = ho.score_table(corr[b], H[b], S[b], THR)
        assert np.isinf(s1_ref[0]) and np.isinf(s1[b, 0]) and np.isinf(s2[b, 0])   # the sample item with e = +inf entered
        assert np.array_equal(cnt[b], cnt_ref)
        for got, ref in ((s1[b], s1_ref), (s2[b], s2_ref)):
            fin = np.isfinite(ref)
            assert np.array_equal(got[~fin], ref[~fin])
            assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-13 * np.abs(ref[fin]))
    for method in range(4):
        rec = device.read_select(device.select_best(cnt_t, s1_t, s2_t, flags_t, min_extra, method, sample_size=4))
        for b in range(2):
            best, err = ho.select(cnt[b], s1[b], s2[b], flags[b], min_extra, method)
            assert rec[b].best_h == best and best != 0
            if best >= 0:
                assert abs(rec[b].best_err - err) <= 1e-15 * err and rec[b].best_cnt == cnt[b, best]
    result = device.select_best(cnt_t, s1_t, s2_t, flags_t, min_extra, 3, sample_size=4)
    rec = device.read_select(result)
    mask = device.homography_inlier_mask(c, H_t, s, result, THR).cpu().numpy()
    for b in range(2):
        assert np.array_equal(mask[b], ho.mask(corr[b], H[b], S[b], rec[b].best_h, THR))
        assert (h == 1 and rec[b].best_h == -1) or np.count_nonzero(mask[b] == 2) == 4
    nothing = device.select_best(cnt_t, s1_t, s2_t, flags_t, n + 1, 3, sample_size=4)
    assert all(r.best_h == -1 for r in device.read_select(nothing))
    mask_t = torch.full((2, n), 7, dtype=torch.uint8, device=c.device)
    mask_t.copy_(device.homography_inlier_mask(c, H_t, s, nothing, THR))
    assert not mask_t.any()


def test_whole_pass_equals_the_separate_calls(dev):
    from structure_from_motion_amd import device

    n, h = TILE + 1, 257
    corr, S = _score_case(n, h, 9)
    c, s = _upload(corr, S)
    ws = device.HomographyWorkspace(2, n, h, dev)
    ws.S.copy_(s)
    ws.run(c, THR, 10, 3)
    H_t, flags_t = device.homography_fit(c, s)
    cnt_t, s1_t, s2_t = device.homography_score(c, H_t, s, THR)
    result = device.select_best(cnt_t, s1_t, s2_t, flags_t, 10, 3, sample_size=4)
    mask = device.homography_inlier_mask(c, H_t, s, result, THR)
    for got, ref in ((ws.H, H_t), (ws.flags, flags_t), (ws.cnt, cnt_t), (ws.s1, s1_t), (ws.s2, s2_t), (ws.result, result),
                     (ws.mask, mask)):
        assert torch.equal(got.view(torch.uint8) if got.dtype == torch.float64 else got,
                           ref.view(torch.uint8) if ref.dtype == torch.float64 else ref)
    out = ws.outcome(1)
    assert out.H.shape == (3, 3) and out.sample.shape == (4,) and out.extra_inliers == int(cnt_t[1, out.best_h])


@pytest.mark.parametrize("n", [4, 5])
def test_philox_route(dev, n):
    from structure_from_motion_amd import device

    corr = ho.motion_scene("plane_bench", n, 40 + n)["corr"]
    h = 70
    ws = device.HomographyWorkspace(1, n, h, dev)
    ws.S.fill_(-7)
    ws.run(device.to_device(corr[None]), THR, 0, 3, philox=(12345, 0, 1))
    S = ws.S.cpu().numpy()[0]
    assert np.all(S[:, n:] == -1) and np.all((S[:, :n] >= 0) & (S[:, :n] < n))
    assert all(len(set(row[:n])) == n for row in S)
    out = ws.outcome(0)
    assert out.best_h >= 0 and np.count_nonzero(out.mask == 2) == 4 and np.array_equal(np.sort(out.sample), np.sort(S[out.best_h, :4]))
    assert np.count_nonzero(out.mask == 1) == out.extra_inliers


def _matches(n):
    return [Match(a_index=i, b_index=i) for i in range(n)]


def test_public_route(dev):
    """estimate_homography_with_ransac against fit_with_ransac on the host with the oracle's callables: the same shuffles, so
    the same winner; H to 1e-9, identical inlier lists, and the same state of ``random`` afterwards."""
    from structure_from_motion_amd.epipolar import homography as hg

    sc = ho.motion_scene("plane_bench", 300, 7, 0.5, 0.3)
    H_ref, inliers_ref = ho.host_ransac(sc, THR, 20, 150, 17)
    state_ref = random.getstate()
    pairs = ho.feature_pairs(sc)
    random.seed(17)
    H, inliers = hg.estimate_homography_with_ransac(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(300), THR, 20,
                                                    max_iterations=150)
    assert random.getstate() == state_ref
    assert H.shape == (3, 3) and np.abs(H - H_ref).max() <= 1e-9
    assert [(a.x, a.y, b.x, b.y) for a, b in inliers] == [(a.x, a.y, b.x, b.y) for a, b in inliers_ref]
    assert len(inliers) >= 150 and inliers[0][0] is not pairs[0][0]
    with pytest.raises(ValueError, match="No model could be found with at least 303 inliers"):
        hg.estimate_homography_with_ransac(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(300), THR, 299, max_iterations=20)


@pytest.mark.parametrize("n, iterations, seed", [(12, 40, 3), (300, 3, 3)])
def test_degenerate_sample_raises_only_when_drawn(dev, monkeypatch, n, iterations, seed):
    """Items 0-3 repeat one pair: a sample holding two of them is flagged.  Whether one is drawn is read from the explicit
    table of the same shuffles; the call raises under SFM_DEGENERATE=raise exactly then, and never under skip."""
    from structure_from_motion_amd.epipolar import homography as hg

    sc = ho.motion_scene("plane_bench", n, 60, 0.5, 0.0)
    for key in ("pix_a", "pix_b", "corr"):
        sc[key][1:4] = sc[key][0]
    pairs = ho.feature_pairs(sc)
    flagged = ho.fit(sc["corr"], _tables(n, iterations, seed))[1].any()
    assert flagged == (n == 12)   # the two cases cover both outcomes
    args = (K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(n), THR)
    monkeypatch.setenv("SFM_DEGENERATE", "raise")
    random.seed(seed)
    if flagged:
        with pytest.raises(hg.HomographyCalculationError):
            hg.estimate_homography_with_ransac(*args, max_iterations=iterations)
    else:
        hg.estimate_homography_with_ransac(*args, max_iterations=iterations)
    monkeypatch.setenv("SFM_DEGENERATE", "skip")
    random.seed(seed)
    H, inliers = hg.estimate_homography_with_ransac(*args, max_iterations=iterations)
    assert np.isfinite(H).all() and len(inliers) >= 4


# scene seed 7 and shuffle seed 5: the NumPy loops of homography_oracle.host_model_choice give (homography count, essential
# count) = (205, 208) for pan10, (205, 206) for gen12, (205, 208) for plane_bench and (0, 205) for bench
@pytest.mark.parametrize("motion, kind", [("pan10", "homography"), ("gen12", "homography"), ("plane_bench", "homography"),
                                          ("bench", "essential")])
def test_model_choice(dev, monkeypatch, motion, kind):
    """Margins from the NumPy draft: ratio 0.97 to 0.99 for a rotation without translation and for a plane, 0.29 for the
    general scene.  On the pan, E alone has as many inliers as H: it cannot reject the pair."""
    from structure_from_motion_amd.epipolar import homography as hg

    monkeypatch.setenv("SFM_DEGENERATE", "raise")   # flagged hypotheses are ignored whatever the policy says
    sc = ho.motion_scene(motion, 300, 7, 0.5, 0.3)
    pairs = ho.feature_pairs(sc)
    random.seed(5)
    m = hg.select_two_view_model(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(300), THR, 20, 200)
    print(motion, m.kind, m.homography_count, m.essential_count, m.ratio)
    assert m.kind == kind
    assert m.essential_count == len(m.essential_inliers) and m.homography_count == len(m.homography_inliers)
    assert m.ratio == (m.homography_count / m.essential_count)
    if kind == "homography":
        assert m.ratio >= 0.9 and m.H.shape == (3, 3)
    else:
        assert m.ratio <= 0.5 and m.E.shape == (3, 3)
    if motion == "pan10":
        assert m.essential_count >= m.homography_count - 10


def test_model_choice_edges(dev):
    from structure_from_motion_amd.epipolar import homography as hg

    sc = ho.motion_scene("plane_bench", 5, 7)
    pairs = ho.feature_pairs(sc)
    random.seed(5)
    m = hg.select_two_view_model(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(5), THR, 0, 10)
    assert m.kind == "homography" and m.E is None and m.essential_count == 0 and m.ratio == float("inf") and m.homography_count == 5
    sc = ho.motion_scene("bench", 300, 7, 0.5, 0.3)
    pairs = ho.feature_pairs(sc)
    with pytest.raises(ValueError, match="Could not estimate"):
        hg.select_two_view_model(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(300), THR, 299, 20)
    random.seed(5)
    m8 = hg.select_two_view_model(K, [p[0] for p in pairs], [p[1] for p in pairs], _matches(300), THR, 20, 200,
                                  essential_solver="eight_point")
    assert m8.kind == "essential" and m8.ratio <= 0.5


def test_other_passes_are_untouched(dev):
    """One essential and one PnP pass before and after a homography pass on the same stream leave bit-equal records."""
    import pnp_oracle
    from structure_from_motion_amd import device

    n, h = 600, 256
    sc = ho.motion_scene("bench", n, 31, 0.5, 0.3)
    c = device.to_device(sc["corr"][None])
    table = _tables(n, h, 8)
    pts = device.to_device(pnp_oracle.scene(n, seed=21, K=K, outlier_fraction=0.3, noise_px=0.5)[0][None])

    def others():
        ews = device.RansacWorkspace(1, n, h, dev)
        ews.S.copy_(device.to_device(table[None], torch.int32))
        ews.run(c, 1.5e-6, 10, 3)
        pws = device.PnPWorkspace(1, n, h, dev)
        pws.S.copy_(device.to_device(table[None], torch.int32))
        pws.run(pts, K, 4.0, 10, 3)
        return [t.clone() for ws in (ews, pws) for t in (ws.result, ws.cnt, ws.s1.view(torch.int64), ws.s2.view(torch.int64),
                                                         ws.model.view(torch.int64), ws.flags, ws.mask)]

    before = others()
    hws = device.HomographyWorkspace(1, n, h, dev)
    hws.S.copy_(device.to_device(table[None], torch.int32))
    hws.run(c, THR, 10, 3)
    assert hws.outcome(0).best_h == -1 or hws.outcome(0).H.shape == (3, 3)
    after = others()
    assert before[0][0, 1] >= 0 and before[7][0, 1] >= 0   # both passes found a model
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_ops_pass_opcheck(dev):
    from structure_from_motion_amd import device, ops

    op = ops.load()
    n, h = 40, 9
    corr, S = _score_case(n, h, 2)
    c, s = _upload(corr, S)
    tests = ("test_schema", "test_faketensor")
    torch.library.opcheck(op.homography_fit.default, (c, s), test_utils=tests)
    H, flags = op.homography_fit(c, s)
    torch.library.opcheck(op.homography_score.default, (c, H, s, THR), test_utils=tests)
    cnt, s1, s2 = op.homography_score(c, H, s, THR)
    result = device.select_best(cnt, s1, s2, flags, 0, 3, sample_size=4)
    torch.library.opcheck(op.homography_inlier_mask.default, (c, H, s, result, THR), test_utils=tests)
    ws = device.HomographyWorkspace(2, n, h, dev)
    ws.S.copy_(s)
    args = (c, 5, 1, False, 0, THR, 0.0, 3, ws.S, ws.H, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask)
    torch.library.opcheck(op.homography_ransac_pass_.default, args, test_utils=tests)


def test_model_choice_app(dev):
    from apps import two_view_model_choice

    rows = {r["motion"]: r for r in two_view_model_choice.run(iterations=100)}
    assert set(rows) == set(two_view_model_choice.motion_cases.MOTIONS) | {"pan10", "gen12", "plane_bench"}
    assert all(rows[name]["kind"] == "homography" and rows[name]["ratio"] >= 0.9 for name in ("pan10", "gen12", "plane_bench"))
    assert rows["bench"]["kind"] == "essential" and rows["bench"]["ratio"] <= 0.5
