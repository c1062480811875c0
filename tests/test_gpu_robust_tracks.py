"""Outlier-robust triangulation of multi-view tracks on the MI355X (csrc/sfm_tracks_robust.hip): parity with the NumPy
definition of tests/robust_tracks_oracle.py on the mixed-length scene of tests/robust_tracks_cases.py, byte-equality with
``triangulate_tracks`` on clean tracks, every status in one call, the bad-index record, empty inputs, run-to-run and
permutation determinism, the public function and the N-view app.  The stream case of the entry point
(tests/robust_tracks_cases.py) runs in test_gpu_streams.py.

Tolerances: ``rc.DEVICE_TOLERANCE``, ten times the spread between two runs of the definition that feed every track's rows
in run order and reversed (``rc.SPREAD``, measured on the CPU and re-measured by test_robust_tracks_host.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import robust_tracks_cases as rc
import robust_tracks_oracle as ro
from structure_from_motion_amd import synthetic

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _run(poses, cam, pt, uv, P, max_error=rc.MAX_ERROR, min_views=2, min_angle=0.0, refine_steps=0, max_hypotheses=64):
    from structure_from_motion_amd import device

    (X, status, err, inlier, angle, info), _ = device.triangulate_tracks_robust(
        device.to_device(np.asarray(poses)), device.to_device(np.asarray(cam), dtype=torch.int32),
        device.to_device(np.asarray(pt), dtype=torch.int32), device.to_device(np.asarray(uv).reshape(-1, 2)), P, K, max_error,
        min_views, min_angle, refine_steps, max_hypotheses)
    return dict(points=X.cpu().numpy(), status=status.cpu().numpy(), obs_error=err.cpu().numpy(), inlier=inlier.cpu().numpy(),
                angle=angle.cpu().numpy(), info=device.read_robust_tracks_info(info))


def _scene_run(sc, P, **options):
    return _run(sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], P, **options)


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("points", "status", "obs_error", "inlier", "angle")) and a["info"] == b["info"]


@pytest.mark.parametrize("options", rc.PARITY_OPTIONS, ids=lambda o: f"h{o[0]}-v{o[1]}-a{o[2]:.3f}-lm{o[3]}")
def test_parity_with_the_definition(dev, options):
    """On clear points the statuses and the inlier flags are the definition's; points, angles and errors agree within ten
    times the definition's own spread between row orders; the counters are equal where every point is clear."""
    max_hypotheses, min_views, min_angle, refine_steps = options
    sc = rc.parity_scene()
    ref = rc.oracle_run(options)
    got = _scene_run(sc, rc.POINTS, min_views=min_views, min_angle=min_angle, refine_steps=refine_steps,
                     max_hypotheses=max_hypotheses)
    clear = ref["clear"]
    clear_obs = clear[sc["point_indices"]]
    assert clear.mean() >= rc.MIN_CLEAR
    gap = rc.spread_between(dict(ref, clear=clear), got, rc.POINTS, sc["point_indices"])
    print(options, "device gaps:", gap, "allowed:", rc.DEVICE_TOLERANCE[refine_steps], "info:", got["info"])
    assert got["info"].status == 0
    assert np.array_equal(got["status"][clear], ref["status"][clear])
    assert np.array_equal(got["inlier"][clear_obs], ref["inlier"][clear_obs])
    assert np.array_equal(np.isnan(got["points"][clear]), np.isnan(ref["points"][clear]))
    assert np.array_equal(np.isnan(got["obs_error"][clear_obs]), np.isnan(ref["obs_error"][clear_obs]))
    assert np.array_equal(np.isnan(got["angle"][clear]), np.isnan(ref["angle"][clear]))
    for name, value in gap.items():
        assert value <= rc.DEVICE_TOLERANCE[refine_steps][name], (name, value)
    if clear.all():
        assert got["info"].hypotheses == ref["info"]["hypotheses"]
        assert got["info"].points_ok == ref["info"]["points_ok"]
        assert got["info"].inlier_observations == ref["info"]["inlier_observations"]
    assert got["info"].max_refine_steps_taken <= refine_steps
    assert (got["info"].max_refine_steps_taken > 0) == (refine_steps > 0)


@pytest.mark.parametrize("refine_steps", [0, 10])
@pytest.mark.parametrize("min_views,min_angle", [(2, 0.0), (3, rc.ONE_DEGREE)])
def test_clean_tracks_are_byte_equal_to_the_plain_triangulator(dev, min_views, min_angle, refine_steps):
    """No shifted pixel and a threshold no observation exceeds: every observation is an inlier of the winner, the refit runs
    over the whole track in run order, and points, angles and errors are the plain call's bytes (an infinite error limit
    there); the points below min_views are FEW_VIEWS in both.  Pins the shared refit code and its operation order."""
    from structure_from_motion_amd import device

    sc = rc.mixed_tracks(rc.CAMERAS, rc.POINTS, rc.LENGTHS, seed=5, shifted=0.0)
    got = _scene_run(sc, rc.POINTS, max_error=1e6, min_views=min_views, min_angle=min_angle, refine_steps=refine_steps)
    X, status, err, angle, info = device.triangulate_tracks(
        device.to_device(sc["poses"]), device.to_device(sc["camera_indices"], dtype=torch.int32),
        device.to_device(sc["point_indices"], dtype=torch.int32), device.to_device(sc["pixels"]), rc.POINTS, K, min_views,
        min_angle, float("inf"), refine_steps)
    plain = dict(points=X.cpu().numpy(), status=status.cpu().numpy(), obs_error=err.cpu().numpy(), angle=angle.cpu().numpy())
    assert set(plain["status"].tolist()) == ({ro.OK, ro.FEW_VIEWS} if min_views == 3 else {ro.OK})
    assert np.array_equal(got["status"], plain["status"]) and (got["status"] == ro.OK).sum() >= 100
    for name in ("points", "angle", "obs_error"):
        assert got[name].tobytes() == plain[name].tobytes(), name
    estimated = np.isin(got["status"], (ro.OK, ro.SMALL_ANGLE))[sc["point_indices"]]
    assert got["inlier"][estimated].all() and not got["inlier"][~estimated].any()
    assert got["info"].max_refine_steps_taken == device.read_tracks_info(info).max_refine_steps_taken
    assert got["info"].points_ok == device.read_tracks_info(info).points_ok


@pytest.mark.parametrize("refine_steps", [0, 10])
def test_every_status_in_one_call(dev, refine_steps):
    """tests/robust_tracks_cases.py::status_scene: each special track sits among OK tracks of its wave."""
    sc = rc.status_scene()
    ref = ro.triangulate(K, sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], sc["points"], rc.MAX_ERROR, 2,
                         sc["min_angle"], refine_steps)
    got = _scene_run(sc, sc["points"], min_angle=sc["min_angle"], refine_steps=refine_steps)
    assert ref["clear"].all()
    if refine_steps == 0:
        assert ref["status"].tolist() == sc["status"].tolist()
    assert got["status"].tolist() == ref["status"].tolist()
    assert np.array_equal(got["inlier"], ref["inlier"])
    assert {ro.OK, ro.FEW_VIEWS, ro.DEGENERATE, ro.SMALL_ANGLE, ro.NO_CONSENSUS} == set(got["status"].tolist())
    estimated = np.isin(ref["status"], (ro.OK, ro.SMALL_ANGLE))
    assert np.array_equal(np.isnan(got["points"]).all(axis=1), ~estimated) and np.array_equal(np.isnan(got["angle"]), ~estimated)
    assert np.array_equal(np.isnan(got["obs_error"]), ~estimated[sc["point_indices"]])
    assert np.allclose(got["points"][estimated], ref["points"][estimated], rtol=0, atol=1e-6)
    assert (got["info"].status, got["info"].points_ok, got["info"].inlier_observations, got["info"].hypotheses) == \
        (0, ref["info"]["points_ok"], ref["info"]["inlier_observations"], ref["info"]["hypotheses"])


def test_a_bad_index_turns_the_whole_call_nan(dev):
    sc = rc.status_scene()
    for cam, pt in ((len(rc.RIG_CENTRES), None), (-1, None), (None, sc["points"]), (None, -1)):
        cams, pts = sc["camera_indices"].copy(), sc["point_indices"].copy()
        if cam is not None:
            cams[17] = cam
        if pt is not None:
            pts[17] = pt
        got = _run(sc["poses"], cams, pts, sc["pixels"], sc["points"])
        assert (got["status"] == ro.BAD_INDEX).all() and np.isnan(got["points"]).all() and np.isnan(got["angle"]).all()
        assert np.isnan(got["obs_error"]).all() and not got["inlier"].any()
        assert got["info"] == type(got["info"])(1, 0, 0, 0, 0)


def test_empty_inputs_and_points_without_observations(dev):
    poses = rc.rig_poses()
    none = _run(poses, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0)
    assert none["points"].shape == (0, 3) and none["inlier"].shape == (0,) and none["info"] == type(none["info"])(0, 0, 0, 0, 0)
    no_obs = _run(poses, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 5)
    assert (no_obs["status"] == ro.FEW_VIEWS).all() and np.isnan(no_obs["points"]).all() and no_obs["info"].points_ok == 0
    cams, uv = rc.rig_track([0, 1, 2])
    some = _run(poses, cams, np.full(3, 3, np.int32), uv, 70)        # one track among 69 points without observations, two waves
    assert some["status"].tolist() == [ro.FEW_VIEWS] * 3 + [ro.OK] + [ro.FEW_VIEWS] * 66
    assert some["inlier"].tolist() == [1, 1, 1] and some["info"].hypotheses == 3 and some["info"].inlier_observations == 3
    no_points = _run(poses, cams, np.zeros(3, np.int32), uv, 0)      # observations of a point that does not exist
    assert no_points["info"].status == 1 and not no_points["inlier"].any() and np.isnan(no_points["obs_error"]).all()


def test_two_runs_and_a_track_preserving_permutation_are_byte_equal(dev):
    sc = rc.parity_scene()
    options = dict(min_views=2, min_angle=rc.ONE_DEGREE, refine_steps=10, max_hypotheses=16)
    first, second = _scene_run(sc, rc.POINTS, **options), _scene_run(sc, rc.POINTS, **options)
    assert _same_bytes(first, second)
    # observation m of the permuted call is the next unused observation of the track a random permutation puts at m
    rng = np.random.default_rng(8)
    pt = sc["point_indices"]
    nxt = {p: list(np.nonzero(pt == p)[0]) for p in range(rc.POINTS)}
    src = np.array([nxt[int(p)].pop(0) for p in pt[rng.permutation(len(pt))]], dtype=np.int64)
    assert not np.array_equal(src, np.arange(len(pt)))
    moved = _run(sc["poses"], sc["camera_indices"][src], pt[src], sc["pixels"][src], rc.POINTS, **options)
    for name in ("points", "status", "angle"):
        assert moved[name].tobytes() == first[name].tobytes(), name
    assert moved["obs_error"].tobytes() == first["obs_error"][src].tobytes()
    assert moved["inlier"].tobytes() == first["inlier"][src].tobytes() and moved["info"] == first["info"]
    assert first["info"].points_ok >= 100


def test_outputs_and_workspace_of_the_caller_are_used(dev):
    from structure_from_motion_amd import device

    sc = rc.parity_scene()
    M = len(sc["pixels"])
    args = (device.to_device(sc["poses"]), device.to_device(sc["camera_indices"], dtype=torch.int32),
            device.to_device(sc["point_indices"], dtype=torch.int32), device.to_device(sc["pixels"]), rc.POINTS, K, rc.MAX_ERROR)
    out, ws = device.triangulate_tracks_robust(*args)
    mine = tuple(torch.full_like(t, 7) for t in out)
    again, used = device.triangulate_tracks_robust(*args, out=mine, workspace=ws)
    assert used is ws and all(a is b for a, b in zip(again, mine))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, mine))
    small = torch.empty((16,), dtype=torch.uint8, device=dev)
    _, used = device.triangulate_tracks_robust(*args, workspace=small)
    assert used is not small and used.numel() >= device._native.load().sfm_tracks_robust_workspace_bytes(rc.POINTS, M)


def test_the_public_function_recovers_the_clean_observations(dev):
    """The value scene through ``triangulate_tracks_robust``: the definition's inlier sets on its clear points (measured on the
    CPU: 183 of the 184 tracks that hold a shifted observation come back with exactly the clean ones)."""
    from structure_from_motion_amd import device
    from structure_from_motion_amd.multiview.tracks import triangulate_tracks_robust

    sc = rc.value_scene()
    r = triangulate_tracks_robust(sc["K"], sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], 9.0)
    ref = ro.triangulate(sc["K"], sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], 300, 9.0)
    clear = ref["clear"][sc["point_indices"]]
    assert ref["clear"].mean() >= rc.MIN_CLEAR and r.inlier.dtype == np.bool_ and r.status.dtype == np.uint8
    assert np.array_equal(r.inlier[clear], ref["inlier"][clear].astype(bool))
    assert np.array_equal(r.status[ref["clear"]], ref["status"][ref["clear"]])
    dirty, robust = rc.recovered(r.inlier, sc, 300)
    print(f"tracks with a shifted observation {dirty}, the device recovers {robust}")
    assert robust >= 0.95 * dirty
    assert isinstance(r.info, device.RobustTracksInfo) and r.info.points_ok == int((r.status == ro.OK).sum())
    assert np.allclose(np.radians(r.angle_deg[r.status == ro.OK]), ref["angle"][r.status == ro.OK], rtol=0, atol=1e-9)


def test_app_registers_all_views_with_robust_triangulation(dev):
    """apps/sfm_multi_view.py --triangulation robust on its default scene: all 8 views, and its counts (printed; how many points
    end OK is recorded in profiles/robust_tracks/README.md, not a condition)."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "apps", "sfm_multi_view.py"), "--triangulation", "robust"],
                         capture_output=True, text=True, cwd=REPO, check=True).stdout
    result = json.loads(out.strip().splitlines()[-1])
    print({k: result[k] for k in ("views_registered", "points_ok", "rms_px", "ba_observations")})
    assert result["triangulation"] == "robust" and result["views_registered"] == 8
