"""The directed track cases of tests/tracks_cases.py on the CPU: the NumPy oracle alone meets every precondition that
tests/test_gpu_tracks_cases.py relies on when it asks the device for the oracle's statuses exactly (no GPU)."""
import numpy as np
import pytest

import tracks_cases as tc
import tracks_oracle as to

STATUS_BAND = 1e-6   # tests/test_gpu_tracks.py: a point this close (relative) to a threshold may flip status
DEPTH_BAND = 1e-6    # the same for the cheirality test: |depth| relative to the point's distance from the camera


@pytest.fixture(scope="module")
def solved():
    """name -> (case, {refine: oracle result}), each computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            case = tc.CASES[name]()
            cache[name] = (case, {refine: tc.oracle(case, refine) for refine in tc.REFINES})
        return cache[name]

    return get


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_no_point_in_a_status_band_and_every_promise_kept(solved, name):
    """Every point but the co-centred pairs keeps more than STATUS_BAND from both thresholds and DEPTH_BAND from depth 0,
    the directed ones MARGIN, with and without refinement; the statuses a construction promises are the oracle's."""
    case, refs = solved(name)
    strict = np.ones(case["P"], dtype=bool)
    strict[case["loose"]] = False
    for refine, ref in refs.items():
        gap = tc.threshold_gap(case, ref)
        assert gap[strict].min() > STATUS_BAND, (refine, int(np.argmin(np.where(strict, gap, np.inf))), gap[strict].min())
        assert tc.depth_gap(case, ref)[strict].min() > DEPTH_BAND, refine
        if case["directed"]:
            assert gap[case["directed"]].min() >= tc.MARGIN, (refine, gap[case["directed"]])
        got = {p: int(ref["status"][p]) for p in case["expect"]}
        assert got == case["expect"], (refine, {p: (s, case["expect"][p]) for p, s in got.items() if s != case["expect"][p]})
        assert ref["info"]["status"] == 0
        assert ref["info"]["points_ok"] == np.count_nonzero(ref["status"] == to.OK)
        nan_point = np.isin(ref["status"], (to.FEW_VIEWS, to.DEGENERATE))
        assert np.array_equal(np.isnan(ref["points"]).all(axis=1), nan_point) and np.array_equal(np.isnan(ref["angle"]), nan_point)
        assert np.array_equal(np.isnan(ref["obs_error"]), nan_point[case["pt"]])


def test_every_status_and_the_precedence_of_the_rules(solved):
    case, refs = solved("every_status")
    for refine, ref in refs.items():
        assert set(ref["status"].tolist()) == {to.OK, to.FEW_VIEWS, to.DEGENERATE, to.BEHIND, to.SMALL_ANGLE, to.LARGE_ERROR}
        max_e = tc.largest_error(case, ref)
        narrow = ref["angle"] < case["min_angle"] * (1.0 - tc.MARGIN)
        off = max_e > case["max_error"] * (1.0 + tc.MARGIN)
        behind = _min_depth(case, ref) <= 0.0
        # 7 breaks all three rules and is BEHIND; 8 breaks two and is SMALL_ANGLE; 3, 4 and 5 break one each
        assert behind[7] and narrow[7] and off[7] and ref["status"][7] == to.BEHIND
        assert not behind[8] and narrow[8] and off[8] and ref["status"][8] == to.SMALL_ANGLE
        assert behind[3] and not narrow[3]
        assert not behind[4] and narrow[4] and not off[4]
        assert not behind[5] and not narrow[5] and off[5]
    tiled, trefs = solved("every_status_tiled")
    assert tiled["P"] == 190
    for ref in trefs.values():
        assert np.array_equal(ref["status"], np.tile(refs[0]["status"], 19))
        for wave in range(0, tiled["P"], 64):
            assert len(set(ref["status"][wave:wave + 64].tolist())) == 6


def _min_depth(case, out):
    pose = case["poses"][case["cam"]]
    c2 = np.einsum("mj,mj->m", pose[:, 6:9], out["points"][case["pt"]]) + pose[:, 11]
    depth = np.full(case["P"], np.inf)
    np.fmin.at(depth, case["pt"], np.where(np.isnan(c2), np.inf, c2))
    return depth


def test_neighbours_are_what_they_are_meant_to_be(solved):
    alone, arefs = solved("neighbours_alone")
    assert sorted(set(np.bincount(alone["pt"]).tolist())) == [2, 3, 4, 5, 6]
    for refine, ref in arefs.items():
        assert np.all(ref["status"] == to.OK) and ref["angle"].min() > 2.0 * tc.MIN_ANGLE
    for kind in tc.FILLERS:
        case, refs = solved(f"neighbours_{kind}")
        for refine, ref in refs.items():
            # the oracle works on each track alone: the 64 tracks come out as they do alone
            assert np.array_equal(ref["status"][0::2], arefs[refine]["status"])
            assert np.allclose(ref["points"][0::2], arefs[refine]["points"], rtol=1e-13, atol=0.0)
            filler = ref["status"][1::2]
            if kind == "few":
                assert np.all(filler == to.FEW_VIEWS)
            elif kind == "nan":
                assert np.all(filler == to.DEGENERATE)
            elif kind == "parallel":
                # 0.5 px of noise on a disparity of 0.26 px: the depth has either sign, and in front the angle stays small
                # (SMALL_ANGLE says so; the band test above keeps it away from 1 degree)
                assert np.all(np.isin(filler, (to.BEHIND, to.SMALL_ANGLE))) and len(set(filler.tolist())) == 2
            elif refine == 0:
                assert np.all(filler == to.LARGE_ERROR)
            else:
                assert np.all(filler != to.OK)


def test_min_views_marks_exactly_the_short_tracks(solved):
    counts = None
    for m in tc.MIN_VIEWS:
        case, refs = solved(f"min_views_{m}")
        counts = np.bincount(case["pt"], minlength=case["P"])
        assert np.array_equal(counts, case["lengths"]) and set(counts.tolist()) == set(range(9))
        assert np.count_nonzero(counts == 0) == 20
        for ref in refs.values():
            assert np.array_equal(ref["status"] == to.FEW_VIEWS, counts < m)
            assert np.all(ref["status"][counts >= m] == to.OK)


def test_long_tracks(solved):
    case, refs = solved("long_tracks")
    counts = np.bincount(case["pt"], minlength=case["P"])
    assert counts.tolist() == list(tc.LONG_LENGTHS)
    assert len(np.unique(case["cam"][case["pt"] == tc.LONG_CYCLE])) == 3
    assert all(len(np.unique(case["cam"][case["pt"] == p])) == counts[p] for p in range(case["P"]) if p != tc.LONG_CYCLE)
    expect = np.full(case["P"], to.OK)
    expect[tc.LONG_OUTLIER] = to.LARGE_ERROR
    assert np.array_equal(refs[0]["status"], expect)
    assert np.all(refs[10]["status"][expect == to.OK] == to.OK)
    # a ray-pair loop that stopped at 64 observations would see another angle on the tracks of 300 distinct cameras
    p = 4
    obs = np.nonzero(case["pt"] == p)[0][:64]
    short = tc.make(case["poses"], case["cam"][obs], np.zeros(64), case["uv"][obs], 1)
    short_angle = _angle_at(short, refs[0]["points"][p])
    assert refs[0]["angle"][p] - short_angle > 1e-3
    # the oracle's own sensitivity to the order of the rows
    back = tc.oracle(tc.reversed_rows(case), 0)
    moved = np.max(np.abs(back["points"] - refs[0]["points"]), axis=1) / np.linalg.norm(refs[0]["points"], axis=1)
    print(f"long tracks, oracle with the rows reversed: points move by {moved.max():.3g} relative")
    assert moved.max() <= 1e-9


def test_lm_step_count_is_decided_by_rounding(solved):
    """Why the device test cannot ask for the oracle's max_refine_steps_taken: once a point has converged, whether LM
    stops on this trial or a later one hangs on the last bits of F.  The oracle itself, given each track's rows in the
    opposite order, lands on the same points (well within REFINED_POINT_TOL = 1e-6) after a different number of steps."""
    case, refs = solved("min_views_3")
    back = tc.oracle(tc.reversed_rows(case), 10)
    ok = refs[10]["status"] == to.OK
    moved = np.max(np.abs(back["points"][ok] - refs[10]["points"][ok]), axis=1) / np.linalg.norm(refs[10]["points"][ok], axis=1)
    steps = (refs[10]["info"]["max_refine_steps_taken"], back["info"]["max_refine_steps_taken"])
    print(f"min_views_3, oracle with the rows reversed: points move by {moved.max():.3g}, most LM steps {steps[0]} -> {steps[1]}")
    assert np.array_equal(back["status"], refs[10]["status"]) and moved.max() <= 1e-8
    assert steps[0] != steps[1] and all(1 <= s <= 10 for s in steps)


def _angle_at(case, X):
    pose = case["poses"][case["cam"]]
    R = pose[:, :9].reshape(1, -1, 3, 3)
    d = to.rays(R, pose[None, :, 9:], X[None])[0]
    return float(np.arccos(np.clip((d @ d.T).min(), -1.0, 1.0)))


@pytest.mark.parametrize("thresholds", ["default", "app"])
def test_one_camera_tracks_are_degenerate_in_the_oracle(solved, thresholds):
    """Points 0 .. 35 name one camera each and are DEGENERATE with NaN outputs, whatever their pixels; the control with a
    second camera stays OK.  A co-centred pair is never OK under the app thresholds: any X in front of both cameras lies on
    one ray from the shared centre, so its two reprojection errors are at least (CO_CENTRED_SPLIT / 2)^2 = 400 px^2 in one
    of them, which the assertion below checks against 16 px^2 with the 1e-3 margin."""
    case, refs = solved(f"one_camera_{thresholds}")
    assert sorted(np.bincount(case["pt"][:-7]).tolist()) == sorted([2, 3, 4, 5] * 9)
    for ref in refs.values():
        one = np.arange(36)
        assert np.all(ref["status"][one] == to.DEGENERATE)
        assert np.all(np.isnan(ref["points"][one])) and np.all(np.isnan(ref["angle"][one]))
        assert np.all(np.isnan(ref["obs_error"][np.isin(case["pt"], one)]))
        assert ref["status"][case["control"]] == to.OK and np.all(np.isfinite(ref["points"][case["control"]]))
        if thresholds == "app":
            tc.check_co_centred(case, ref)


def test_non_finite_input_is_degenerate_and_nothing_else_is(solved):
    case, refs = solved("non_finite")
    assert len(case["touched"]) == 30
    for wave in range(0, case["P"], 64):
        inside = [p for p in case["touched"] if wave <= p < wave + 64]
        assert 0 < len(inside) < min(64, case["P"] - wave) // 2
    for ref in refs.values():
        assert np.array_equal(np.nonzero(ref["status"] == to.DEGENERATE)[0], case["touched"])
        assert np.all(ref["status"][np.setdiff1d(np.arange(case["P"]), case["touched"])] == to.OK)
        assert ref["info"]["status"] == 0
