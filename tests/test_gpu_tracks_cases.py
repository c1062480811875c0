"""Triangulation of multi-view tracks on the MI355X (csrc/sfm_tracks.hip) on the directed cases of tests/tracks_cases.py:
every status and the precedence of the rules, the same tracks among different wave mates, every ``min_views``, tracks of
up to 300 observations, tracks of one camera and non-finite input; against the NumPy oracle of tests/tracks_oracle.py.
tests/test_tracks_cases_host.py shows on the CPU that no point of these cases lies near a threshold, so the statuses,
the NaN and inf patterns, info.status and info.points_ok have to equal the oracle's exactly: there are no exclusions but
the two co-centred pairs of case 5, whose status rounding decides.  info.max_refine_steps_taken is held to its range
(see _check)."""
import numpy as np
import pytest
import torch

import tracks_cases as tc
import tracks_oracle as to
# the tolerances are those of test_gpu_tracks.py, reasoned there; none is set here
from test_gpu_tracks import COST_TOL, POINT_TOL, REFINED_ERROR_TOL, REFINED_POINT_TOL, VALUE_TOL

pytestmark = pytest.mark.gpu

WIDE = tc.MIN_ANGLE   # as in test_gpu_tracks.py, values are compared on tracks of at least 1 degree


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


@pytest.fixture(scope="module")
def solved():
    """(name, refine) -> (case, oracle result), each computed once and left unchanged."""
    cases, refs = {}, {}

    def get(name, refine):
        if name not in cases:
            cases[name] = tc.CASES[name]()
        if (name, refine) not in refs:
            refs[name, refine] = tc.oracle(cases[name], refine)
        return cases[name], refs[name, refine]

    return get


def _device_call(case, refine):
    from structure_from_motion_amd import device

    X, status, err, angle, info = device.triangulate_tracks(
        device.to_device(case["poses"]), device.to_device(case["cam"], dtype=torch.int32),
        device.to_device(case["pt"], dtype=torch.int32), device.to_device(case["uv"]), case["P"], tc.K, case["min_views"],
        case["min_angle"], case["max_error"], refine)
    return dict(points=X.cpu().numpy(), status=status.cpu().numpy(), obs_error=err.cpu().numpy(), angle=angle.cpu().numpy(),
                info=device.read_tracks_info(info))


def _gaps(case, a, b, points):
    """Worst gaps between two results on ``points`` (a mask): points relative to |X|, angle absolute, e and each
    point's cost relative above 1 px^2 (the measures of test_gpu_tracks.py::test_parity_with_oracle)."""
    if not points.any():
        return dict(points=0.0, angle=0.0, error=0.0, cost=0.0)
    dp = np.max(np.abs(a["points"][points] - b["points"][points]), axis=1) / np.linalg.norm(b["points"][points], axis=1)
    da = np.abs(a["angle"][points] - b["angle"][points])
    obs = points[case["pt"]] & np.isfinite(b["obs_error"])
    de = np.abs(a["obs_error"][obs] - b["obs_error"][obs]) / np.maximum(1.0, np.abs(b["obs_error"][obs]))
    cost_a = np.bincount(case["pt"][obs], weights=a["obs_error"][obs], minlength=case["P"])[points]
    cost_b = np.bincount(case["pt"][obs], weights=b["obs_error"][obs], minlength=case["P"])[points]
    dc = np.abs(cost_a - cost_b) / np.maximum(1.0, cost_b)
    return dict(points=float(dp.max()), angle=float(da.max()), error=float(de.max(initial=0.0)), cost=float(dc.max()))


def _assert_within(gaps, refine, what):
    print(f"{what} refine={refine}: " + ", ".join(f"{k} {v:.3g}" for k, v in gaps.items()))
    if refine == 0:
        assert gaps["points"] <= POINT_TOL and gaps["angle"] <= VALUE_TOL and gaps["error"] <= VALUE_TOL, (what, gaps)
    else:
        assert gaps["points"] <= REFINED_POINT_TOL and gaps["angle"] <= REFINED_POINT_TOL, (what, gaps)
        assert gaps["error"] <= REFINED_ERROR_TOL, (what, gaps)
    assert gaps["cost"] <= COST_TOL, (what, gaps)


def _check(name, case, got, ref, refine, narrow_too=False):
    """Statuses, NaN and inf patterns, info.status and info.points_ok equal the oracle's; the values of the points of at least 1
    degree (of every finite point with ``narrow_too``) are within the tolerances."""
    strict = np.ones(case["P"], dtype=bool)
    strict[case["loose"]] = False
    differ = np.nonzero((got["status"] != ref["status"]) & strict)[0]
    assert len(differ) == 0, (name, refine, [(int(p), int(got["status"][p]), int(ref["status"][p])) for p in differ[:10]])
    for p, status in case["expect"].items():
        assert got["status"][p] == status, (name, refine, p)
    assert np.array_equal(np.isnan(got["points"][strict]), np.isnan(ref["points"][strict]))
    assert np.array_equal(np.isnan(got["angle"][strict]), np.isnan(ref["angle"][strict]))
    obs = strict[case["pt"]]
    assert np.array_equal(np.isnan(got["obs_error"][obs]), np.isnan(ref["obs_error"][obs]))
    assert np.array_equal(np.isinf(got["obs_error"][obs]), np.isinf(ref["obs_error"][obs]))
    assert got["info"].status == ref["info"]["status"] == 0
    assert got["info"].points_ok == np.count_nonzero(got["status"] == to.OK)
    if not case["loose"]:
        assert got["info"].points_ok == ref["info"]["points_ok"]
    # The most LM steps of any point equal the oracle's only where no point refines at all.  Otherwise last bits decide
    # them: the oracle's own count moves by up to 7 per point, and its largest from 10 to 9 and from 6 to 8, when each
    # track's rows are merely reversed (test_tracks_cases_host.py::test_lm_step_count_is_decided_by_rounding, DESIGN.md
    # §6i), while each point's cost agrees to COST_TOL below.  So the count is held to its range.
    if ref["info"]["max_refine_steps_taken"] == 0:
        assert got["info"].max_refine_steps_taken == 0
    else:
        assert 1 <= got["info"].max_refine_steps_taken <= refine
    finite = strict & np.all(np.isfinite(ref["points"]), axis=1)
    with np.errstate(invalid="ignore"):
        compared = finite if narrow_too else finite & (ref["angle"] >= WIDE)
    _assert_within(_gaps(case, got, ref, compared), refine, f"tracks case {name} vs oracle")
    return compared


# Measured worst gaps to the oracle on one MI355X (points relative, angle, error, point cost), refine 0 / refine 10; the
# bounds are POINT_TOL = VALUE_TOL = 1e-9 / REFINED_POINT_TOL = 1e-6, REFINED_ERROR_TOL = 1e-5, and COST_TOL = 1e-9:
#   every_status (and tiled, the 0.07 degree tracks included)  2.3e-15 8.9e-14 9.1e-14 7.6e-15 / 1.3e-13 0 5.4e-26 1.5e-25
#   copies of a track vs its first copy                        0 (bit-identical here) in both
#   neighbours_alone                                           4.6e-14 8.7e-15 5.5e-12 3.3e-13 / 8.3e-11 1.3e-11 5.3e-9 8.8e-14
#   neighbours_few, _nan: the 64 tracks vs alone               0 (bit-identical) in both
#   neighbours_parallel, _outlier: the 64 tracks vs alone      2.2e-16 2.3e-15 1.6e-13 8.9e-14 / 2.2e-10 1.9e-11 2.5e-9 7.7e-14
#   neighbours_outlier, every point of at least 1 degree       5.1e-14 1.1e-14 6.6e-12 3.3e-13 / 1.7e-9 4.0e-10 7.3e-8 9.0e-14
#   min_views 2, 3, 4, 7 (worst)                               3.9e-14 8.8e-15 7.2e-12 2.1e-13 / 2.3e-10 2.1e-11 1.9e-8 2.2e-13
#   long_tracks (7 .. 300 observations)                        2.6e-15 1.6e-15 9.4e-13 1.2e-13 / 6.6e-12 2.2e-12 2.0e-9 6.4e-15
#   one_camera (the control)                                   1.1e-15 0 2.2e-13 2.7e-14 / 2.0e-12 1.6e-13 6.3e-11 3.6e-15
#   non_finite (the untouched wave mates)                      4.1e-14 9.8e-15 8.4e-12 5.0e-13 / 1.8e-9 1.5e-10 2.0e-8 1.4e-13
# The co-centred pairs came out BEHIND on the device and OK / OK (default thresholds) or SMALL_ANGLE / LARGE_ERROR (app
# thresholds) in the oracle.
@pytest.mark.parametrize("refine", tc.REFINES)
@pytest.mark.parametrize("name", ["every_status", "every_status_tiled"])
def test_every_status_through_the_kernel(dev, solved, name, refine):
    """One track per status and per combination of broken rules, alone in its wave and tiled so that each wave holds
    every kind.  The narrow tracks (0.07 degrees) are compared too; copies of a track agree within the tolerances, not bit
    for bit, since the wave decides how long null_vector4 iterates."""
    case, ref = solved(name, refine)
    got = _device_call(case, refine)
    _check(name, case, got, ref, refine, narrow_too=True)
    if "period" in case:
        first = np.arange(case["P"]) % case["period"]
        copy0 = dict(points=got["points"][first], angle=got["angle"][first],
                     obs_error=got["obs_error"][np.arange(len(case["pt"])) % (len(case["pt"]) // (case["P"] // case["period"]))])
        finite = np.all(np.isfinite(got["points"]), axis=1)
        _assert_within(_gaps(case, got, copy0, finite), refine, f"tracks case {name}, copies vs the first copy")


@pytest.mark.parametrize("refine", tc.REFINES)
def test_a_track_does_not_depend_on_its_wave_mates(dev, solved, refine):
    """The same 64 tracks alone and interleaved 1:1 with FEW_VIEWS tracks, NaN pixels, near-parallel pairs and gross
    outliers: a filler that does not converge sends the whole wave to null_vector4's Jacobi route, and the 64 tracks keep
    their status and stay within the tolerances of the oracle and of the call without fillers."""
    alone, ref_alone = solved("neighbours_alone", refine)
    got_alone = _device_call(alone, refine)
    _check("neighbours_alone", alone, got_alone, ref_alone, refine)
    m = len(alone["cam"])
    every = np.ones(64, dtype=bool)
    for kind in tc.FILLERS:
        case, ref = solved(f"neighbours_{kind}", refine)
        got = _device_call(case, refine)
        _check(f"neighbours_{kind}", case, got, ref, refine)
        mine = dict(points=got["points"][0::2], angle=got["angle"][0::2], status=got["status"][0::2], obs_error=got["obs_error"][:m])
        assert np.array_equal(mine["status"], got_alone["status"]) and np.all(mine["status"] == to.OK)
        _assert_within(_gaps(alone, mine, got_alone, every), refine, f"tracks case neighbours_{kind}, the 64 tracks vs alone")
        _assert_within(_gaps(alone, mine, ref_alone, every), refine, f"tracks case neighbours_{kind}, the 64 tracks vs oracle")


@pytest.mark.parametrize("refine", tc.REFINES)
@pytest.mark.parametrize("min_views", tc.MIN_VIEWS)
def test_min_views(dev, solved, min_views, refine):
    """FEW_VIEWS exactly where a point has fewer than min_views observations (0 .. 8 here), with NaN point, angle and
    errors; every other point matches the oracle."""
    name = f"min_views_{min_views}"
    case, ref = solved(name, refine)
    got = _device_call(case, refine)
    _check(name, case, got, ref, refine)
    few = case["lengths"] < min_views
    assert np.array_equal(got["status"] == to.FEW_VIEWS, few)
    assert np.all(np.isnan(got["points"][few])) and np.all(np.isnan(got["angle"][few]))
    assert np.array_equal(np.isnan(got["obs_error"]), few[case["pt"]])
    assert got["info"].points_ok == np.count_nonzero(~few)


def test_min_views_through_the_public_function(dev, solved):
    from lib.multiview.tracks import triangulate_tracks

    case, ref = solved("min_views_3", 10)
    r = triangulate_tracks(tc.K, case["poses"], case["cam"], case["pt"], case["uv"], num_points=case["P"], min_views=3,
                           min_angle_deg=1.0, max_reprojection_error=tc.MAX_ERROR, refine_steps=10)
    got = _device_call(case, 10)
    assert np.array_equal(r.status, got["status"]) and np.array_equal(r.status == to.FEW_VIEWS, case["lengths"] < 3)
    assert np.array_equal(r.points, got["points"], equal_nan=True)
    assert np.array_equal(r.observation_error, got["obs_error"], equal_nan=True)
    assert np.array_equal(r.angle_deg, np.degrees(got["angle"]), equal_nan=True) and r.info == got["info"]
    assert np.array_equal(r.status, ref["status"])


@pytest.mark.parametrize("refine", tc.REFINES)
def test_long_tracks(dev, solved, refine):
    """Tracks of 7, 63, 64, 65 and 300 observations, one that repeats 3 cameras 100 times and one with a 15 px outlier
    among 65: the Givens stream and the ray-pair loop beyond the 6 .. 8 observations of every other test.  On the CPU the
    oracle itself moves by 1.9e-15 when each track's rows are reversed (tests/test_tracks_cases_host.py)."""
    case, ref = solved("long_tracks", refine)
    got = _device_call(case, refine)
    compared = _check("long_tracks", case, got, ref, refine)
    assert compared.all()


@pytest.mark.parametrize("refine", tc.REFINES)
@pytest.mark.parametrize("thresholds", ["default", "app"])
def test_one_camera_tracks_are_degenerate(dev, solved, thresholds, refine):
    """Tracks whose observations all name one camera are DEGENERATE with NaN outputs, whatever their pixels and the
    thresholds; two observations of camera 0 and one of camera 1 stay OK.  A pair of distinct cameras with one centre and
    pixels 40 px apart is never OK under the app thresholds on either side (its status is left to rounding): any X in front
    of both lies on one ray from the shared centre, so one of its errors is at least (40 / 2)^2 = 400 px^2, which is
    asserted against 16 px^2 with the 1e-3 margin."""
    name = f"one_camera_{thresholds}"
    case, ref = solved(name, refine)
    got = _device_call(case, refine)
    _check(name, case, got, ref, refine)
    one = np.arange(36)
    assert np.all(got["status"][one] == to.DEGENERATE)
    assert np.all(np.isnan(got["points"][one])) and np.all(np.isnan(got["angle"][one]))
    assert np.all(np.isnan(got["obs_error"][np.isin(case["pt"], one)]))
    assert got["status"][case["control"]] == to.OK
    if thresholds == "app":
        tc.check_co_centred(case, ref)
        tc.check_co_centred(case, got)
    print(f"tracks case {name} refine={refine}: co-centred pairs device {got['status'][case['loose']]} "
          f"oracle {ref['status'][case['loose']]}")


@pytest.mark.parametrize("refine", tc.REFINES)
def test_non_finite_input(dev, solved, refine):
    """A NaN pixel, an infinite pixel and a NaN pose entry make exactly the tracks that touch them DEGENERATE with NaN
    outputs; their wave mates match the oracle, and info.status stays 0."""
    case, ref = solved("non_finite", refine)
    got = _device_call(case, refine)
    _check("non_finite", case, got, ref, refine)
    assert np.array_equal(np.nonzero(got["status"] == to.DEGENERATE)[0], case["touched"])
    assert np.all(np.isnan(got["points"][case["touched"]])) and np.all(np.isnan(got["angle"][case["touched"]]))
    assert np.all(np.isnan(got["obs_error"][np.isin(case["pt"], case["touched"])]))
    assert got["info"].status == 0
