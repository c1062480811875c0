"""The NumPy definition of the homography kernels (tests/homography_oracle.py) against a multi-precision evaluation
(oracle/homography_mp.py) on the special motions, planes and samples of tests/homography_cases.py: the fit, the flag around
its floor, the transfer error with its inf and NaN conventions, the score table, the selection and the mask on special
models and thresholds, and the host RANSAC loops of the model choice on six scenes.  Nothing here needs a GPU: it makes the
definition that tests/test_gpu_homography_cases.py compares the device with a checked one."""
import random

import mpmath as mp
import numpy as np
import pytest

import homography_cases as hc
import homography_oracle as ho
from oracle.homography_mp import fit_homography_mp, transfer_error_mp

SAMPLES_PER_SCENE = 200


def _compare_with_mp(corr, S, H, flags, ratio, label):
    """The assertions of the fit: per sample the flag outside the dead band, and for unflagged samples the parity bound.
    Returns (samples in the dead band, worst gap / bound)."""
    in_band, worst = 0, 0.0
    for k in range(S.shape[0]):
        H_mp, ratio_mp = fit_homography_mp(corr[S[k, :4]])
        ratio_mp = float(ratio_mp)
        if hc.in_dead_band(ratio_mp):
            in_band += 1
            continue
        assert flags[k] == int(not ratio_mp >= ho.DEGENERATE_FLOOR), (label, k, ratio[k], ratio_mp)
        if flags[k]:
            continue
        gap, bound = hc.parity_gap(H[k], H_mp, ratio_mp)
        assert gap <= bound, (label, k, gap, bound, ratio_mp)
        assert abs(ratio[k] - ratio_mp) <= 1e-12, (label, k)   # singular values are known to eps sigma_1
        worst = max(worst, float(gap / bound))
    return in_band, worst


def test_fit_on_the_hand_made_samples():
    names, corr, S = hc.sample_table()
    assert set(names) == set(hc.EXPECTED_FLAG) and len(names) == 23
    H, flags, ratio = ho.fit(corr, S)
    for k, name in enumerate(names):
        in_band, worst = _compare_with_mp(corr, S[k:k + 1], H[k:k + 1], flags[k:k + 1], ratio[k:k + 1], name)
        assert in_band == 0, name   # no hand-made sample sits in the dead band
        assert flags[k] == hc.EXPECTED_FLAG[name], name
        print(f"{name}: ratio {ratio[k]:.3g}, gap / bound {worst:.3g}")
    for name in hc.SINGULAR_H:
        assert abs(ho.det(H[names.index(name)])) <= 1e-12
    for name in ("coincident_four", "nan_coordinate", "inf_coordinate"):
        assert np.isnan(H[names.index(name)]).all()
    # exact structure gives exact models: the identity, the quarter and half turns, the zoom, the affine shift
    unit = lambda M: np.ravel(M) / np.linalg.norm(M)   # noqa: E731
    quarter, half = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.diag([-1.0, -1.0, 1.0])
    expected = {"identity_square": np.eye(3), "identity_general": np.eye(3), "roll90_square": quarter, "roll180_square": half,
                "zoom2_square": np.diag([2.0, 2.0, 1.0]),
                "shift_square": np.array([[1.0, 0.0, 0.05], [0.0, 1.0, -0.03], [0.0, 0.0, 1.0]])}
    for name, M in expected.items():
        assert np.abs(H[names.index(name)] - unit(M)).max() <= 1e-14, name
    # the near-collinear family brackets the floor from both sides, outside the dead band
    assert [hc.EXPECTED_FLAG[f"near_collinear_{r:g}"] for r in hc.NEAR_COLLINEAR_EPS] == [0, 0, 1, 1]


@pytest.mark.parametrize("motion, shape", hc.SIX)
def test_fit_on_shuffle_samples(motion, shape):
    """200 shuffle samples of a scene with 30 % outliers and 0.5 px noise."""
    from structure_from_motion_amd import device

    n = 300
    corr = hc.scene(motion, shape, n, 21, 0.5, 0.3)["corr"]
    S = device.PyShuffleTable(n, SAMPLES_PER_SCENE, random.Random(5), advance=False).S
    H, flags, ratio = ho.fit(corr, S)
    in_band, worst = _compare_with_mp(corr, S, H, flags, ratio, (motion, shape))
    print(f"{motion}/{shape}: dead-band share {in_band / SAMPLES_PER_SCENE:.3f}, flagged {int(flags.sum())}, "
          f"ratio min {np.nanmin(ratio):.3g}, worst gap / bound {worst:.3g}")
    assert in_band <= SAMPLES_PER_SCENE // 100


def test_out_of_range_and_repeated_indices():
    corr = hc.scene("bench", "plane", 10, 3)["corr"]
    S = np.array([[0, 1, 2, 3], [0, -1, 2, 3], [0, 1, 2, 10], [0, 1, 2, 0]])
    H, flags, _ = ho.fit(corr, S)
    assert flags.tolist() == [0, 1, 1, 1] and np.isnan(H[1]).all() and np.isnan(H[2]).all()


# ---- the scorer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def score_case():
    """One scene (tx over the steep plane, 30 % outliers, 0.5 px) with a NaN and an inf item, the special models first and
    then fitted hypotheses, and the multi-precision error of every (hypothesis, item)."""
    n, h = 60, 16
    motion, shape = "tx", "steep"
    corr = hc.scene(motion, shape, n, 11, 0.5, 0.3)["corr"].copy()
    corr[7, 1], corr[9, 2] = np.nan, np.inf
    rng = np.random.default_rng(4)
    S = np.array([rng.choice(n, 4, replace=False) for _ in range(h)])
    S[S == 7], S[S == 9] = 8, 10   # the non-finite items stay out of the samples here ...
    S[12, 0], S[13, 3] = 7, 9      # ... but for two hypotheses
    assert all(len(set(row)) == 4 for row in S)
    H, flags, _ = ho.fit(corr, S)
    assert flags[12] == 1 and flags[13] == 1 and flags[len(hc.SPECIAL):12].sum() == 0
    models, item_p, item_q = hc.special_models(corr, hc.true_homography(motion, shape), taken=(7, 9))
    for k, name in enumerate(hc.SPECIAL):
        H[k] = models[name]
        flags[k] = 0   # a model from elsewhere: only its score keeps it from winning
    e_mp = [[transfer_error_mp(H[k], corr[i]) for i in range(n)] for k in range(h)]
    return dict(corr=corr, S=S, H=H, flags=flags, e_mp=e_mp, item_p=item_p, item_q=item_q, n=n, h=h)


def test_transfer_error_conventions(score_case):
    corr, H, e_mp, n = score_case["corr"], score_case["H"], score_case["e_mp"], score_case["n"]
    index = {name: k for k, name in enumerate(hc.SPECIAL)}
    e = np.array([ho.transfer_error(H[k], corr) for k in range(score_case["h"])])
    finite_item = np.isfinite(corr).all(axis=1)
    # a NaN model: NaN, which passes no gate; a non-finite item or an inf model: NaN, or +inf where the other side's third
    # coordinate is <= 0 — never a finite value, so such an item passes no finite threshold
    assert np.isnan(e[index["nan"]]).all() and np.isnan(e[:, 7]).any() and np.isnan(e[:, 9]).any()
    assert not np.isfinite(e[:, 7]).any() and not np.isfinite(e[index["inf"]]).any() and not np.isfinite(e[:, 9]).any()
    # adj(H) = 0 for rank <= 1: q2 = 0, +inf on every finite item; rank 2 maps every x_b to one point with q2 of either sign
    for name in ("zero", "rank1"):
        assert np.all(e[index[name]][finite_item] == np.inf), name
    assert np.isinf(e[index["rank2"]][finite_item]).any()
    # the line at infinity, on each side alone
    for name, item in (("infinity_p2", score_case["item_p"]), ("infinity_q2", score_case["item_q"])):
        h = H[index[name]]
        xa, ya, xb, yb = corr[item]
        p2 = (h[6] * xa + h[7] * ya) + h[8]
        q2 = ((h[3] * h[7] - h[4] * h[6]) * xb + (h[1] * h[6] - h[0] * h[7]) * yb) + (h[0] * h[4] - h[1] * h[3])
        assert (p2 < 0.0 < q2) if name == "infinity_p2" else (q2 < 0.0 < p2), name
        assert e[index[name], item] == np.inf and np.isfinite(e[index[name]]).any()
    # against the multi-precision formula: +inf in the same places, and the values to rounding.  Each of du, dv, eu, ev
    # carries at most 16 roundings of magnitudes below 1 (coordinates below 0.6, unit-norm well-conditioned H): an absolute
    # error delta <= 16 eps each, so |e - e_mp| <= 2 * 4 * delta * sqrt(e) + 4 * delta^2
    delta = 16.0 * np.finfo(np.float64).eps
    for name in ("identity", "scaled_up", "scaled_down"):
        k = index[name]
        for i in np.nonzero(finite_item)[0]:
            ref = e_mp[k][i]
            assert (ref == mp.inf) == (e[k, i] == np.inf), (name, i)
            if ref != mp.inf:
                assert abs(mp.mpf(float(e[k, i])) - ref) <= 8.0 * delta * mp.sqrt(ref) + 4.0 * delta * delta, (name, i, e[k, i])
    # scaling H by 1e+-150 changes nothing but roundings in adj(H)
    assert np.allclose(e[index["scaled_up"]][finite_item], e[index["scaled_down"]][finite_item], rtol=1e-9, atol=0.0)
    for k in range(score_case["h"]):   # +inf exactly where the multi-precision sign says, unless p2 or q2 is at the rounding level
        for i in np.nonzero(finite_item)[0]:
            if np.isfinite(H[k]).all() and k not in (index["zero"], index["rank1"], index["rank2"]):
                assert (e_mp[k][i] == mp.inf) == (e[k, i] == np.inf), (k, i)


def _mp_decisions(e_mp_row, thr):
    """Per item: 1 / 0 whether the multi-precision error passes e <= thr, or -1 when it is within 1e-12 relative of thr or
    when the model or the item is not finite (IEEE rules decide those, not precision: test_transfer_error_conventions)."""
    out = []
    for ref in e_mp_row:
        if mp.isnan(ref):
            out.append(-1)
        elif np.isnan(thr):
            out.append(0)
        elif ref != mp.inf and np.isfinite(thr) and thr > 0.0 and abs(ref - mp.mpf(thr)) <= mp.mpf(1e-12) * mp.mpf(thr):
            out.append(-1)
        else:
            out.append(int(ref <= mp.mpf(thr)))
    return np.array(out)


def test_score_select_mask_on_special_models_and_thresholds(score_case):
    corr, S, H, flags, e_mp, n, h = (score_case[k] for k in ("corr", "S", "H", "flags", "e_mp", "n", "h"))
    index = {name: k for k, name in enumerate(hc.SPECIAL)}
    tie_item = next(i for i in range(n) if i not in S[index["identity"]] and np.isfinite(corr[i]).all())
    tie = float(ho.transfer_error(H[index["identity"]], corr)[tie_item])   # equal to one item's error bit for bit
    assert 0.0 < tie < np.inf
    for thr in hc.THRESHOLDS + (tie,) + hc.SENTINEL_THRESHOLDS:
        cnt, s1, s2 = ho.score_table(corr, H, S, thr)
        skipped = 0
        for k in range(h):
            sample = np.zeros(n, dtype=bool)
            sample[S[k]] = True
            decided = _mp_decisions(e_mp[k], thr)
            with np.errstate(invalid="ignore"):
                passes = ho.transfer_error(H[k], corr) <= thr
            if k == index["rank2"]:
                decided = np.where(np.isfinite(ho.transfer_error(H[k], corr)), decided, -1)   # q2 = 0 to rounding: sign arbitrary
            known = decided >= 0
            skipped += int((~known & np.isfinite(corr).all(axis=1)).sum()) if np.isfinite(H[k]).all() else 0
            assert np.array_equal(passes[known], decided[known] == 1), (thr, k)
            assert cnt[k] == np.count_nonzero(passes & ~sample), (thr, k)
            assert not (np.isfinite(thr) or np.isnan(thr)) or not (passes[7] or passes[9]), (thr, k)
            if known.all():
                assert cnt[k] == np.count_nonzero((decided == 1) & ~sample), (thr, k)
        if thr == tie:
            assert skipped >= 1 and cnt[index["identity"]] >= 1   # the item on the threshold is counted: e <= thr
            with np.errstate(invalid="ignore"):
                assert ho.transfer_error(H[index["identity"]], corr)[tie_item] <= thr
        if thr in (0.0, -1.0) or np.isnan(thr):
            assert not cnt.any()
        if thr == np.inf:   # everything finite passes, +inf passes too (inf <= inf), NaN does not
            e_true = ho.transfer_error(H[index["scaled_up"]], corr)
            assert cnt[index["scaled_up"]] == np.count_nonzero(~np.isnan(e_true)) - 4
        # the scaled copies of the true H count what the true H counts
        cnt_true = ho.score_table(corr, hc.true_homography("tx", "steep")[None], S[index["scaled_up"]][None], thr)[0][0]
        if thr != tie:
            assert cnt[index["scaled_up"]] == cnt_true and cnt[index["scaled_down"]] == ho.score_table(
                corr, hc.true_homography("tx", "steep")[None], S[index["scaled_down"]][None], thr)[0][0]
        # the non-finite items enter no count and no mask unless they are in the sample
        for method in range(4):
            best, err = ho.select(cnt, s1, s2, flags, 5, method)
            if thr in hc.SENTINEL_THRESHOLDS or thr == 0.0:
                assert best == -1 and err == np.inf
            assert best == -1 or best >= len(hc.SPECIAL) or hc.SPECIAL[best] not in hc.NEVER_SELECTED
            assert best not in (12, 13)   # flagged: a non-finite item in the sample
            mask = ho.mask(corr, H, S, best, thr)
            if best >= 0:
                assert np.isfinite(err) and mask[7] == 0 and mask[9] == 0 and np.count_nonzero(mask == 2) == 4
                assert np.count_nonzero(mask == 1) == cnt[best]
            else:
                assert not mask.any()
    # at the ordinary threshold the planted model wins over the fitted hypotheses of a 16-row table or ties with one of them
    cnt, s1, s2 = ho.score_table(corr, H, S, hc.THR)
    assert cnt[index["scaled_up"]] >= 30 and ho.select(cnt, s1, s2, flags, 5, 3)[0] >= 0
    # a sample that holds a non-finite item: NaN sums, never selected even without its flag
    assert np.isnan(s1[12]) and np.isnan(s1[13])
    assert ho.select(cnt[12:14], s1[12:14], s2[12:14], np.zeros(2, dtype=np.int32), 0, 3)[0] == -1


@pytest.mark.parametrize("motion, shape", hc.HOST_LOOP_CASES)
def test_host_loops_of_the_model_choice(motion, shape):
    """The two host RANSAC loops (four-point H, five-point E) on 300 matches, 30 % outliers, 0.5 px, threshold 2e-5, 200
    iterations, scene seed 7 and shuffle seed 5.  The counts are the project's own host definition of what
    select_two_view_model computes; the table records them.  Forward motion over a scene with depth (tz, roll15_tz) reaches
    the 0.8 of MAX_HOMOGRAPHY_RATIO by this definition itself: a property of the rule, not of a kernel."""
    expected = {("bench", "general"): (0, 205), ("tz", "general"): (159, 208), ("roll15_tz", "general"): (178, 206),
                ("tx", "fronto"): (205, 207), ("still", "general"): (205, 207), ("turn170", "plane"): (79, 123)}
    counts = hc.host_model_choice(motion, shape)
    print(f"{motion}/{shape}: H {counts[0]}, E {counts[1]}, ratio {counts[0] / counts[1]:.3f}")
    assert counts == expected[(motion, shape)]
