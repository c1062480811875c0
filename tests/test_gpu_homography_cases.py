"""The homography kernels on the MI355X (csrc/sfm_homography.h) on the special motions, planes and samples of
tests/homography_cases.py, against the NumPy definition (tests/homography_oracle.py, itself checked against a
multi-precision evaluation by tests/test_homography_cases_host.py) and, for the hand-made samples, against that
multi-precision evaluation directly.  Explicit sample tables and vectorised definitions only: no host RANSAC loop runs here."""
import math
import random

import numpy as np
import pytest
import torch

import homography_cases as hc
import homography_oracle as ho
import view_graph_oracle as vo
from oracle import sfm_oracle as orc
from structure_from_motion_amd.feature_matching.matching import Match

pytestmark = pytest.mark.gpu

K = hc.K
THR = hc.THR
N, H_COUNT = 300, 257   # four full 64-lane blocks of the fit launch and a partial one; one 256-lane scoring block and one lane
RMS = 3
MIN_EXTRA = 10


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _table(n, h, seed):
    from structure_from_motion_amd import device

    return device.PyShuffleTable(n, h, random.Random(seed), advance=False).S


@pytest.fixture(scope="module")
def sweep(dev):
    """Every (motion, shape) as one batch: corr (65, N, 4) with 30 % outliers and 0.5 px noise, a shuffle table per scene, and
    the NumPy fit of every sample (computed once, never written)."""
    from structure_from_motion_amd import device

    corr = np.stack([hc.scene(m, s, N, 21 + q, 0.5, 0.3)["corr"] for q, (m, s) in enumerate(hc.CASES)])
    S = np.stack([_table(N, H_COUNT, 5 + q) for q in range(len(hc.CASES))]).astype(np.int32)
    ref = [ho.fit(corr[q], S[q]) for q in range(len(hc.CASES))]
    return dict(corr=corr, S=S, ref=ref, corr_t=device.to_device(corr), S_t=device.to_device(S, torch.int32))


def test_fit_on_the_hand_made_samples(dev):
    """Every hand-made sample once in every lane position of the 64-lane fit block, and two rows with an index out of range,
    in one launch, against the NumPy definition and the multi-precision one: flags, the parity bound
    max(1e-9, 1e-13 / (sigma_8 / sigma_1)) (up to sign where |det H| <= 1e-9), det >= 0, unit norm."""
    from oracle.homography_mp import fit_homography_mp
    from structure_from_motion_amd import device

    names, corr, S0 = hc.sample_table()
    m, n = len(names), len(corr)
    assert math.gcd(m, 64) == 1   # row j holds sample j % m: over 64 repeats each sample meets each lane once
    S = np.tile(S0, (64, 1))
    outside = np.zeros((2, 8), dtype=np.int32)
    outside[0, :4], outside[1, :4] = (0, -1, 2, 3), (0, 1, 2, n)
    S = np.vstack([S, outside])
    assert len(S) % 64 != 0
    H_t, flags_t = device.homography_fit(device.to_device(corr[None]), device.to_device(S[None], torch.int32))
    H_all, flags_all = H_t.cpu().numpy()[0], flags_t.cpu().numpy()[0]
    assert flags_all[-2] == 1 and flags_all[-1] == 1
    H_rep, flags_rep = H_all[:-2].reshape(64, m, 9), flags_all[:-2].reshape(64, m)
    assert np.array_equal(flags_rep, np.tile(flags_rep[0], (64, 1)))
    assert np.array_equal(H_rep, np.tile(H_rep[:1], (64, 1, 1)), equal_nan=True)   # no result depends on the lane
    H_dev, flags_dev = H_rep[0], flags_rep[0]
    H_np, flags_np, ratio_np = ho.fit(corr, S0)
    worst = {}
    for k, name in enumerate(names):
        H_mp, ratio_mp = fit_homography_mp(corr[S0[k, :4]])
        ratio_mp = float(ratio_mp)
        assert not hc.in_dead_band(ratio_mp), name
        assert flags_dev[k] == flags_np[k] == int(not ratio_mp >= ho.DEGENERATE_FLOOR) == hc.EXPECTED_FLAG[name], name
        if flags_dev[k]:
            continue
        for ref, ratio, label in ((H_np[k], ratio_np[k], "numpy"), (H_mp, ratio_mp, "mp")):
            gap, bound = hc.parity_gap(H_dev[k], ref, ratio)
            key = (hc.FAMILY[name], label)
            worst[key] = max(worst.get(key, (0.0, "")), (float(gap / bound), name))
            assert gap <= bound, (name, label, gap, bound)
        assert ho.det(H_dev[k]) >= 0.0, name
        assert abs(np.sqrt(np.sum(H_dev[k] ** 2)) - 1.0) <= 1e-14, name
    for (family, label), (value, name) in sorted(worst.items()):
        print(f"{family} vs {label}: worst gap / bound {value:.3g} ({name})")
    assert {family for family, _ in worst} == {"exact", "aligned", "degenerate", "near_collinear"}


def test_fit_on_motions(dev, sweep):
    """257 shuffle samples of each of the 65 (motion, shape) scenes in one launch: the contract of test_fit_parity.  The flag
    of a sample whose ratio lies in the dead band around the floor is not asserted; at most 1 % may lie there."""
    from structure_from_motion_amd import device

    H_t, flags_t = device.homography_fit(sweep["corr_t"], sweep["S_t"])
    H_dev, flags_dev = H_t.cpu().numpy(), flags_t.cpu().numpy()
    worst, in_band, flagged = {}, 0, 0
    for q, (motion, shape) in enumerate(hc.CASES):
        H_ref, flags_ref, ratio = sweep["ref"][q]
        band = (ratio >= hc.DEAD_BAND[0]) & (ratio <= hc.DEAD_BAND[1])
        in_band += int(band.sum())
        flagged += int(flags_ref.sum())
        assert np.array_equal(flags_dev[q][~band], flags_ref[~band]), (motion, shape)
        ok = (flags_ref == 0) & (flags_dev[q] == 0)
        gap, bound = hc.parity_gap(H_dev[q][ok], H_ref[ok], ratio[ok])
        k = int(np.argmax(gap / bound))
        worst[shape] = max(worst.get(shape, (0.0, "", 0.0)), (float(gap[k] / bound[k]), motion, float(ratio[ok][k])))
        assert (gap <= bound).all(), (motion, shape, gap[k], bound[k], ratio[ok][k])
        assert np.all(ho.det(H_dev[q][ok]) >= 0.0), (motion, shape)
        assert np.abs(np.sqrt(np.sum(H_dev[q][ok] ** 2, axis=1)) - 1.0).max() <= 1e-14, (motion, shape)
    total = len(hc.CASES) * H_COUNT
    for shape, (value, motion, ratio) in worst.items():
        print(f"{shape}: worst gap / bound {value:.3g} ({motion}, ratio {ratio:.3g})")
    print(f"dead-band share {in_band / total:.5f} ({in_band} of {total}), flagged {flagged}")
    assert in_band <= total // 100


def _score_batch(n, cases, seed):
    """corr (3, n, 4), S (3, 257, 8) of three scenes; scene 1 holds an item with a NaN and one with an inf coordinate."""
    corr = np.stack([hc.scene(m, s, n, seed + q, 0.5, 0.3)["corr"] for q, (m, s) in enumerate(cases)])
    corr[1, 7, 1], corr[1, 9, 2] = np.nan, np.inf
    S = np.stack([_table(n, H_COUNT, seed + 10 + q) for q in range(len(cases))]).astype(np.int32)
    return corr, S


@pytest.mark.parametrize("n, cases", [(300, hc.SIX[0::2]), (513, hc.SIX[1::2])])
def test_score_selection_mask(dev, n, cases):
    """The device's own H on both sides, hypotheses 0-9 overwritten with the special models of homography_cases.SPECIAL:
    cnt exact, s1 and s2 within 1e-13 relative where finite and identical where not, the selection equal to the host rule for
    the four aggregation methods, the mask byte-equal, at the thresholds 0, 1e-12, 2e-5, 1e30, +inf and one equal to an
    item's error under hypothesis 1 (the identity); -1 and NaN leave no count and no winner.  An item with a NaN or an inf
    coordinate has a NaN or +inf error: it enters no count and no mask at a finite threshold unless it is in the sample."""
    from structure_from_motion_amd import device

    B, special = len(cases), len(hc.SPECIAL)
    index = {name: k for k, name in enumerate(hc.SPECIAL)}
    corr, S = _score_batch(n, cases, 3 + n % 7)
    c, s = device.to_device(corr), device.to_device(S, torch.int32)
    H_t, flags_t = device.homography_fit(c, s)
    H, flags = H_t.cpu().numpy(), flags_t.cpu().numpy()
    assert np.array_equal(flags, np.stack([ho.fit(corr[b], S[b])[1] for b in range(B)]))
    nonfinite_sampled = np.any((S[1, :, :4] == 7) | (S[1, :, :4] == 9), axis=1)
    assert nonfinite_sampled[special:].any() and np.all(flags[1][nonfinite_sampled] == 1)
    for b, (motion, shape) in enumerate(cases):
        models, _, _ = hc.special_models(corr[b], hc.true_homography(motion, shape), taken=(7, 9))
        H[b, :special] = np.stack([models[name] for name in hc.SPECIAL])
    flags[:, :special] = 0   # models from elsewhere: only their scores keep them from winning
    H_t, flags_t = device.to_device(H), device.to_device(flags, torch.int32)
    tie_item = next(i for i in range(n) if i not in S[0, index["identity"], :4])
    tie = float(ho.transfer_error(H[0, index["identity"]], corr[0])[tie_item])
    assert 0.0 < tie < np.inf
    for thr in hc.THRESHOLDS + (tie,) + hc.SENTINEL_THRESHOLDS:
        cnt_t, s1_t, s2_t = device.homography_score(c, H_t, s, thr)
        cnt, s1, s2 = cnt_t.cpu().numpy(), s1_t.cpu().numpy(), s2_t.cpu().numpy()
        for b in range(B):
            cnt_ref, s1_ref, s2_ref = ho.score_table(corr[b], H[b], S[b], thr)
            assert np.array_equal(cnt[b], cnt_ref), (thr, b, np.nonzero(cnt[b] != cnt_ref)[0][:5])
            for got, ref in ((s1[b], s1_ref), (s2[b], s2_ref)):
                fin = np.isfinite(ref)
                assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (thr, b)
                assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-13 * np.abs(ref[fin])), (thr, b)
            if thr == THR:   # the scaled copies of the true H count what the true H counts
                for name in ("scaled_up", "scaled_down"):
                    k = index[name]
                    H_true = hc.true_homography(*cases[b])
                    assert cnt[b, k] == ho.score_table(corr[b], H_true[None], S[b, k][None], thr)[0][0], (b, name)
            if thr in hc.SENTINEL_THRESHOLDS or np.isnan(thr):
                assert not cnt[b].any()
        if thr == tie:   # e <= thr holds with equality: the item is counted
            e = ho.transfer_error(H[0, index["identity"]], corr[0])
            assert cnt[0, index["identity"]] == np.count_nonzero(e <= tie) - np.count_nonzero(e[S[0, index["identity"], :4]] <= tie)
            assert e[tie_item] == tie
        for method in range(4):
            result = device.select_best(cnt_t, s1_t, s2_t, flags_t, MIN_EXTRA, method, sample_size=4)
            rec = device.read_select(result)
            for b in range(B):
                best, err = ho.select(cnt[b], s1[b], s2[b], flags[b], MIN_EXTRA, method)
                assert rec[b].best_h == best, (thr, method, b)
                assert best not in [index[name] for name in hc.NEVER_SELECTED]
                if best >= 0:
                    assert abs(rec[b].best_err - err) <= 1e-15 * err and rec[b].best_cnt == cnt[b, best]
                if not thr > 0.0:   # 0, -1 and NaN: no count reaches min_extra
                    assert best == -1
            if method == RMS:
                mask = device.homography_inlier_mask(c, H_t, s, result, thr).cpu().numpy()
                for b in range(B):
                    assert np.array_equal(mask[b], ho.mask(corr[b], H[b], S[b], rec[b].best_h, thr)), (thr, b)
                if np.isfinite(thr) and rec[1].best_h >= 0:
                    assert mask[1, 7] == 0 and mask[1, 9] == 0
        if np.isfinite(thr):   # the non-finite items pass no finite gate: dropping them changes no count outside the samples
            kept = np.setdiff1d(np.arange(n), [7, 9])
            renumber = np.cumsum(np.isin(np.arange(n), kept)) - 1
            rows = np.nonzero(~nonfinite_sampled)[0]
            cnt_without = ho.score_table(corr[1][kept], H[1][rows], renumber[S[1][rows, :4]], thr)[0]
            assert np.array_equal(cnt[1][rows], cnt_without)
    # the fixture is not vacuous at the ordinary threshold: every scene has a winner, and on the scenes one homography
    # explains the planted model has the inliers
    cnt_t, s1_t, s2_t = device.homography_score(c, H_t, s, THR)
    rec = device.read_select(device.select_best(cnt_t, s1_t, s2_t, flags_t, MIN_EXTRA, RMS, sample_size=4))
    for b, case in enumerate(cases):
        assert rec[b].best_h >= 0
        if case in hc.PLANTED:
            assert int(cnt_t[b, index["scaled_up"]]) >= 0.6 * n


def test_whole_pass(dev, sweep):
    """HomographyWorkspace.run on the explicit tables of all 65 scenes at once: record and mask equal the host rule on the
    workspace's own H, cnt, s1, s2 and flags; on every plane and every rotation (turn170 apart) a winner has most inliers."""
    from structure_from_motion_amd import device

    B = len(hc.CASES)
    ws = device.HomographyWorkspace(B, N, H_COUNT, dev)
    ws.S.copy_(sweep["S_t"])
    ws.run(sweep["corr_t"], THR, MIN_EXTRA, RMS)
    H, flags, cnt, s1, s2, mask = (t.cpu().numpy() for t in (ws.H, ws.flags, ws.cnt, ws.s1, ws.s2, ws.mask))
    rec = device.read_select(ws.result)
    counts = {}
    for q, case in enumerate(hc.CASES):
        best, err = ho.select(cnt[q], s1[q], s2[q], flags[q], MIN_EXTRA, RMS)
        assert rec[q].best_h == best, case
        if best >= 0:
            assert abs(rec[q].best_err - err) <= 1e-15 * err and rec[q].best_cnt == cnt[q, best], case
        assert np.array_equal(mask[q], ho.mask(sweep["corr"][q], H[q], sweep["S"][q], best, THR)), case
        counts[case] = 4 + int(rec[q].best_cnt) if best >= 0 else 0
        if case in hc.PLANTED:
            assert best >= 0 and counts[case] >= 190, (case, counts[case])
    planted = [counts[c] for c in hc.PLANTED]
    print(f"planted scenes: winner's count min {min(planted)}, max {max(planted)} of {N}")
    print("general scenes with a translation:", {c[0]: counts[c] for c in hc.CASES if c not in hc.PLANTED and c[1] == "general"})
    print("turn170:", {c[1]: counts[c] for c in hc.CASES if c[0] == "turn170"})


@pytest.mark.parametrize("motion, shape", hc.PUBLIC_ROUTE_CASES)
def test_public_route_counts(dev, monkeypatch, motion, shape):
    """select_two_view_model on the scene and shuffles of the host loops (test_homography_cases_host.py): its two counts are
    those the NumPy definitions give on the device's own tables of the same shuffles, and the kind follows from them.  No
    kind is assumed: forward motion over depth lands on either side of 0.8."""
    from structure_from_motion_amd import device
    from structure_from_motion_amd.epipolar import homography as hg

    monkeypatch.delenv("SFM_SAMPLER", raising=False)
    r = hc.ROUTE
    n, h, thr, min_extra = r["n"], r["iterations"], r["threshold"], r["min_extra"]
    sc = hc.scene(motion, shape, n, r["scene_seed"], r["noise_px"], r["outlier_fraction"])
    pairs = ho.feature_pairs(sc)
    random.seed(r["shuffle_seed"])
    m = hg.select_two_view_model(K, [p[0] for p in pairs], [p[1] for p in pairs], [Match(a_index=i, b_index=i) for i in range(n)],
                                 thr, min_extra, h)
    S = _table(n, h, r["shuffle_seed"]).astype(np.int32)
    c = device.normalize_correspondences(device.to_device(sc["pix_a"]), device.to_device(sc["pix_b"]), K).reshape(1, n, 4)
    corr = c.cpu().numpy()[0]
    s = device.to_device(S[None], torch.int32)
    H_t, flags_t = device.homography_fit(c, s)
    H = H_t.cpu().numpy()[0]
    cnt, s1, s2 = ho.score_table(corr, H, S, thr)
    best, _ = ho.select(cnt, s1, s2, flags_t.cpu().numpy()[0], min_extra, RMS)
    h_count = 4 + int(cnt[best]) if best >= 0 else 0
    ews = device.RansacWorkspace(1, n, h, dev)
    ews.S.copy_(s)
    ews.run(c, thr, min_extra, RMS, solver="five_point")
    E, e_flags = ews.E.cpu().numpy()[0], ews.flags.cpu().numpy()[0]
    e_cnt = np.zeros(h, dtype=np.int32)
    for k in range(h):
        passes = orc.sed_values(E[k].reshape(3, 3), corr) <= thr
        passes[S[k, :vo.E_SAMPLE]] = False
        e_cnt[k] = np.count_nonzero(passes)
    assert np.array_equal(e_cnt, ews.cnt.cpu().numpy()[0])
    e_best, _ = vo.select(e_cnt, ews.s1.cpu().numpy()[0], ews.s2.cpu().numpy()[0], e_flags, min_extra, vo.E_SAMPLE)
    e_count = vo.E_SAMPLE + int(e_cnt[e_best]) if e_best >= 0 else 0
    print(f"{motion}/{shape}: H {m.homography_count}, E {m.essential_count}, ratio {m.ratio:.3f}, kind {m.kind}")
    assert (m.homography_count, m.essential_count) == (h_count, e_count) and e_count > 0
    assert m.ratio == h_count / e_count
    assert (m.kind == "homography") == (h_count / e_count > hg.MAX_HOMOGRAPHY_RATIO)
    assert m.homography_count == len(m.homography_inliers) and m.essential_count == len(m.essential_inliers)
