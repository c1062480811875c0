"""Outlier-robust triangulation of tracks without a GPU: the NumPy definition (its hypothesis ranks, every status on a
constructed track, noise-free tracks), the feature's value as a condition, the share of clear points and the spread of the
parity inputs of tests/test_gpu_robust_tracks.py, the exports and bindings, the C ABI's refusals, the argument checks of the
public API, the lib re-export and the app's option."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import robust_tracks_cases as rc
import robust_tracks_oracle as ro
from structure_from_motion_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h
K = synthetic.BENCH_K


# ------------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------------
def test_ranks_are_distinct_increasing_and_below_the_pair_count():
    for k in range(2, 71):
        T = k * (k - 1) // 2
        for max_hypotheses in (1, 16, 64):
            ranks = ro.hypothesis_ranks(k, max_hypotheses)
            assert len(ranks) == min(T, max_hypotheses)
            assert all(a < b for a, b in zip(ranks, ranks[1:])) and ranks[0] == 0 and ranks[-1] < T
            if T <= max_hypotheses:
                assert ranks == list(range(T))
            else:   # evenly spaced: neighbouring gaps differ by at most one
                gaps = np.diff(ranks + [T])
                assert gaps.max() - gaps.min() <= 1
    # nothing overflows: the longest track the entry point admits
    k = 2**31 - 1
    ranks = ro.hypothesis_ranks(k, 1024)
    assert ranks[-1] < k * (k - 1) // 2 < 2**62 and ro.unrank_pair(ranks[-1], k)[1] < k


def test_unranking_is_a_bijection():
    for k in range(2, 71):
        pairs = [ro.unrank_pair(r, k) for r in range(k * (k - 1) // 2)]
        assert pairs == [(i, j) for i in range(k) for j in range(i + 1, k)]
    k = 2**31 - 1
    T = k * (k - 1) // 2
    assert ro.unrank_pair(0, k) == (0, 1) and ro.unrank_pair(T - 1, k) == (k - 2, k - 1) and ro.unrank_pair(k - 2, k) == (0, k - 1)
    assert ro.unrank_pair(k - 1, k) == (1, 2)


def _clean_scene(cameras=6, points=40, per_point=5, seed=2):
    pr = synthetic.bundle_problem(cameras, points, per_point=per_point, seed=seed, noise_px=0.0)
    return pr["poses_true"], pr["camera_indices"], pr["point_indices"], pr["pixels"], pr["points_true"]


def test_noise_free_tracks_come_back_with_every_flag_set():
    poses, cam, pt, uv, X = _clean_scene()
    for refine_steps in (0, 5):
        r = ro.triangulate(K, poses, cam, pt, uv, len(X), 1e-6, refine_steps=refine_steps)
        assert (r["status"] == ro.OK).all() and r["inlier"].all() and r["clear"].all()
        assert np.abs(r["points"] - X).max() < 1e-9 and r["obs_error"].max() < 1e-12
        assert r["info"] == dict(status=0, points_ok=len(X), max_refine_steps_taken=r["info"]["max_refine_steps_taken"],
                                 inlier_observations=len(cam), hypotheses=len(X) * 10, reserved=0)


def test_every_status_of_every_step_on_a_constructed_track():
    """tests/robust_tracks_cases.py::status_scene: every status of steps 0 to 5, each from every step that can set it.  The one
    exception is step 4's DEGENERATE: its refit runs over observations whose errors at a finite point are finite and within
    the threshold, from at least two cameras, so neither a non-finite row nor a null vector at infinity was constructed; the
    guard is checked on the null-vector function itself."""
    sc = rc.status_scene()
    args = (K, sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], sc["points"], rc.MAX_ERROR, 2, sc["min_angle"])
    r = ro.triangulate(*args)
    assert r["status"].tolist() == sc["status"].tolist() and r["clear"].all() and r["info"]["status"] == 0
    for p, name in enumerate(sc["names"]):
        if r["status"][p] not in (ro.FEW_VIEWS, ro.DEGENERATE):
            assert r["step"][p] == sc["step"][p], name
    seen = {(int(s), int(t)) for s, t in zip(r["status"], r["step"])}
    assert seen == {(ro.OK, 5), (ro.SMALL_ANGLE, 5), (ro.FEW_VIEWS, 0), (ro.DEGENERATE, 0), (ro.NO_CONSENSUS, 3),
                    (ro.NO_CONSENSUS, 4), (ro.NO_CONSENSUS, 5)}
    by_name = {name: p for p, name in enumerate(sc["names"])}
    flags = lambda name: r["inlier"][sc["point_indices"] == by_name[name]].tolist()   # noqa: E731
    assert flags("twice") == [1, 1, 1, 1] and flags("behind_mixed") == [0, 0, 1, 1, 1] and flags("narrow") == [1, 1, 1, 1]
    assert np.abs(r["points"][by_name["twice"]] - np.array(rc.RIG_POINT)).max() < 1e-9
    # OK and SMALL_ANGLE write the estimate, the angle, all errors and the flags; every other status NaN and no flags
    for p in range(sc["points"]):
        mine = sc["point_indices"] == p
        if r["status"][p] in (ro.OK, ro.SMALL_ANGLE):
            assert np.isfinite(r["points"][p]).all() and np.isfinite(r["angle"][p]) and np.isfinite(r["obs_error"][mine]).all()
            assert np.array_equal(r["inlier"][mine], r["obs_error"][mine] <= rc.MAX_ERROR)
        else:
            assert np.isnan(r["points"][p]).all() and np.isnan(r["angle"][p]) and np.isnan(r["obs_error"][mine]).all()
            assert not r["inlier"][mine].any()
    assert r["info"]["points_ok"] == int((r["status"] == ro.OK).sum())
    assert r["info"]["inlier_observations"] == int(r["inlier"][np.isin(sc["point_indices"], np.nonzero(r["status"] == ro.OK)[0])].sum())
    # the hypotheses of single tracks: the same-camera pair is skipped, the pair behind its cameras is not scored
    one = lambda cams, uv: rc._rig_run(cams, uv)["info"]["hypotheses"]   # noqa: E731
    assert one(*rc.rig_track([0, 2, 2, 1])) == 5 and one(*rc.rig_track([0, 1], rc.RIG_BEHIND)) == 0
    assert one(*rc.rig_track([0, 1], shifts={1: (0.0, 40.0)})) == 1
    # BAD_INDEX: the whole call, whichever index is out of range
    for cam, pt in ((6, 0), (-1, 0), (0, 70), (0, -1)):
        cams, pts = sc["camera_indices"].copy(), sc["point_indices"].copy()
        cams[17], pts[17] = (cam if cam else cams[17]), (pt if pt else pts[17])
        bad = ro.triangulate(K, sc["poses"], cams, pts, sc["pixels"], sc["points"], rc.MAX_ERROR)
        assert (bad["status"] == ro.BAD_INDEX).all() and bad["info"] == dict(status=1, points_ok=0, max_refine_steps_taken=0,
                                                                             inlier_observations=0, hypotheses=0, reserved=0)
        assert np.isnan(bad["points"]).all() and np.isnan(bad["obs_error"]).all() and np.isnan(bad["angle"]).all()
        assert not bad["inlier"].any()
    # FEW_VIEWS by min_views
    few = ro.triangulate(*args[:7], 4)
    lengths = np.bincount(sc["point_indices"], minlength=sc["points"])
    assert np.array_equal(few["status"] == ro.FEW_VIEWS, lengths < 4)
    # step 4's guard
    assert ro._null_vector(np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0], [0, 0, 0, 1.0]])) is None   # at infinity
    assert ro._null_vector(np.full((4, 4), np.nan)) is None and ro._null_vector(np.eye(4)[:3]) is not None
    # the arguments the definition refuses
    for bad in (dict(max_error=np.inf), dict(max_error=-1.0), dict(max_error=np.nan), dict(max_hypotheses=0),
                dict(max_hypotheses=1025), dict(min_views=1), dict(refine_steps=-1), dict(min_angle=-0.1)):
        with pytest.raises(ValueError):
            ro.triangulate(**{**dict(K=K, poses=sc["poses"], cam=[0, 1], pt=[0, 0], uv=np.zeros((2, 2)), num_points=1,
                                     max_error=9.0), **bad})


# ------------------------------------------------------------------------------------------------------
# the value, as a condition
# ------------------------------------------------------------------------------------------------------
def test_the_definition_recovers_the_clean_observations_and_thresholding_the_plain_fit_does_not():
    """8 cameras x 300 points x 6 per point at the true poses, 15 % of the pixels shifted by up to +-100 px, threshold 9 px^2.
    Measured: 184 tracks hold a shifted observation; the definition returns exactly the clean observations for 183 of them,
    thresholding the plain N-view DLT's errors for 0, with or without the second attempt."""
    sc = rc.value_scene()
    args = (sc["K"], sc["poses"], sc["camera_indices"], sc["point_indices"], sc["pixels"], 300, 9.0)
    r = ro.triangulate(*args)
    dirty, robust = rc.recovered(r["inlier"], sc, 300)
    print(f"tracks with a shifted observation {dirty}, the definition recovers {robust}")
    assert dirty > 150 and robust >= 0.95 * dirty
    for second_attempt in (False, True):
        _, plain = rc.recovered(ro.plain_threshold_inliers(*args, second_attempt=second_attempt), sc, 300)
        print(f"plain DLT threshold, second attempt {second_attempt}: {plain}")
        assert plain <= 0.05 * dirty


# ------------------------------------------------------------------------------------------------------
# what the GPU comparisons rest on
# ------------------------------------------------------------------------------------------------------
def test_parity_inputs_are_clear_and_the_spread_is_as_recorded():
    sc = rc.parity_scene()
    assert len(set(np.bincount(sc["point_indices"]).tolist())) == len(rc.LENGTHS) and rc.POINTS == 130
    assert {o[0] for o in rc.PARITY_OPTIONS} == {16, 64} and {o[1] for o in rc.PARITY_OPTIONS} == {2, 3}
    assert {o[2] for o in rc.PARITY_OPTIONS} == {0.0, rc.ONE_DEGREE} and {o[3] for o in rc.PARITY_OPTIONS} == {0, 10}
    worst = {steps: dict(points=0.0, angle=0.0, error=0.0) for steps in rc.SPREAD}
    for options in rc.PARITY_OPTIONS:
        a, b = rc.oracle_run(options), rc.oracle_run(options, reverse=True)
        clear = a["clear"]
        print(options, "clear", clear.mean(), "statuses", np.bincount(a["status"], minlength=8).tolist(), a["info"])
        assert clear.mean() >= rc.MIN_CLEAR
        assert np.array_equal(a["status"][clear], b["status"][clear])
        assert np.array_equal(a["inlier"][clear[sc["point_indices"]]], b["inlier"][clear[sc["point_indices"]]])
        assert (a["status"] == ro.OK).sum() >= 100 and (a["status"] == ro.NO_CONSENSUS).sum() >= 1
        s = rc.spread_between(a, b, rc.POINTS, sc["point_indices"])
        for k, v in s.items():
            worst[options[3]][k] = max(worst[options[3]][k], v)
    print("spread between row orders:", worst)
    for steps, spread in worst.items():
        for k, v in spread.items():
            assert v <= rc.SPREAD[steps][k], (steps, k, v)
            assert v >= 0.1 * rc.SPREAD[steps][k], (steps, k, v)   # the recorded figure is the measured one, not a generous one
    # the sampled ranks are in use: at 16 hypotheses a 12-long track scores at most 16, at 64 more
    assert rc.oracle_run(rc.PARITY_OPTIONS[0])["info"]["hypotheses"] < rc.oracle_run(rc.PARITY_OPTIONS[1])["info"]["hypotheses"]


# ------------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native, build, device
    from structure_from_motion_amd.multiview import tracks

    lib = _native.load()
    assert len(_native.SIGNATURES["sfm_triangulate_tracks_robust"]) == 22
    assert "sfm_tracks_robust_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(lib, "sfm_triangulate_tracks_robust") and hasattr(lib, "sfm_tracks_robust_workspace_bytes")
    assert "sfm_tracks_robust.hip" in build.SOURCES and "sfm_tracks_device.h" in build.HEADERS
    assert C.sizeof(_native.TracksRobustInfo) == 48
    assert [f[0] for f in _native.TracksRobustInfo._fields_] == ["status", "points_ok", "max_refine_steps_taken",
                                                                 "inlier_observations", "hypotheses", "reserved"]
    assert device.TRACKS_NO_CONSENSUS == ro.NO_CONSENSUS == 7 and callable(device.triangulate_tracks_robust)
    assert [f for f in device.RobustTracksInfo.__dataclass_fields__] == [f[0] for f in _native.TracksRobustInfo._fields_[:5]]
    assert callable(device.read_robust_tracks_info)
    assert lib.sfm_tracks_robust_workspace_bytes(130, 901) == lib.sfm_tracks_workspace_bytes(130, 901) > 0
    assert lib.sfm_tracks_robust_workspace_bytes(-1, 0) == -1 and lib.sfm_tracks_robust_workspace_bytes(0, 2**31) == -1
    assert lib.sfm_tracks_robust_workspace_bytes(2**31 - 1, 0) == -1
    parameters = inspect.signature(tracks.triangulate_tracks_robust).parameters
    assert list(parameters) == ["camera_matrix", "poses", "camera_indices", "point_indices", "pixels", "max_reprojection_error",
                                "num_points", "min_views", "min_angle_deg", "refine_steps", "max_hypotheses"]
    assert parameters["max_reprojection_error"].default is inspect.Parameter.empty
    assert {k: parameters[k].default for k in ("num_points", "min_views", "min_angle_deg", "refine_steps", "max_hypotheses")} == \
        dict(num_points=None, min_views=2, min_angle_deg=0.0, refine_steps=0, max_hypotheses=64)
    assert list(tracks.RobustTracksResult.__dataclass_fields__) == ["points", "status", "observation_error", "inlier", "angle_deg",
                                                                    "info"]
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header and lib.sfm_abi_version() == 15
    assert "#define SFM_TRACKS_NO_CONSENSUS 7" in header and "tests/robust_tracks_oracle.py" in header
    record = header[header.index("typedef struct sfm_tracks_robust_info {"):header.index("} sfm_tracks_robust_info;")]
    assert record.count("int64_t") == 6
    declaration = header[header.index("int sfm_triangulate_tracks_robust("):]
    declaration = " ".join(declaration[:declaration.index(";")].split())
    for text in ("double max_error, int refine_steps, int max_hypotheses", "uint8_t* inlier", "sfm_tracks_robust_info* info",
                 "int64_t workspace_bytes, void* stream)"):
        assert text in declaration
    # the entry point only enqueues: its comment must not claim otherwise
    comment = header[header.index("/* sfm_triangulate_tracks for tracks that hold wrong observations"):
                     header.index("int sfm_triangulate_tracks_robust(")]
    assert "synchronises" not in comment
    # the plain entry point is what it was
    assert len(_native.SIGNATURES["sfm_triangulate_tracks"]) == 20


def test_c_abi_refuses_bad_arguments_without_a_gpu(native_lib):
    from structure_from_motion_amd import _native

    lib = _native.load()
    buf = (C.c_int64 * 64)()   # host memory: a refused call never touches it
    base = C.addressof(buf)
    base += (-base) % 16
    dummy = C.c_void_p(base)
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    call = lib.sfm_triangulate_tracks_robust

    def refused(K=Kc, cameras=3, points=4, observations=8, poses=dummy, cam=dummy, pt=dummy, pixels=dummy, min_views=2,
                min_angle=0.0, max_error=9.0, refine_steps=0, max_hypotheses=64, points_out=dummy, status=dummy, obs_error=dummy,
                inlier=dummy, angle=dummy, info=dummy, workspace=dummy, workspace_bytes=1 << 20):
        return call(K, cameras, points, observations, poses, cam, pt, pixels, min_views, min_angle, max_error, refine_steps,
                    max_hypotheses, points_out, status, obs_error, inlier, angle, info, workspace, workspace_bytes, None) == EINVAL

    for name in ("cameras", "points", "observations"):
        assert refused(**{name: -1}), name
    assert refused(cameras=2**31) and refused(points=2**31 - 1) and refused(observations=2**31)
    assert refused(min_views=1) and refused(min_views=0) and b"min_views" in lib.sfm_last_error()
    for bad in (-1e-9, float("nan"), float("inf")):
        assert refused(min_angle=bad) and b"min_angle" in lib.sfm_last_error()
    for bad in (-1e-9, float("nan"), float("inf"), float("-inf")):
        assert refused(max_error=bad) and b"max_error" in lib.sfm_last_error()
    assert refused(refine_steps=-1) and b"refine_steps" in lib.sfm_last_error()
    for bad in (0, -1, 1025, 2**31 - 1):
        assert refused(max_hypotheses=bad) and b"max_hypotheses" in lib.sfm_last_error()
    bad_K = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    bad_K[8] = 2.0
    assert refused(K=bad_K) and refused(K=None)
    for name in ("poses", "cam", "pt", "pixels", "points_out", "status", "inlier", "info", "workspace"):
        assert refused(**{name: None}), name
        assert b"sfm_triangulate_tracks_robust: null pointer" in lib.sfm_last_error()
    need = lib.sfm_tracks_robust_workspace_bytes(4, 8)
    assert refused(workspace_bytes=need - 1) and b"workspace too small" in lib.sfm_last_error()
    assert refused(workspace=C.c_void_p(base + 8)) and b"16-byte" in lib.sfm_last_error()
    # the plain entry point keeps its own name in its messages
    assert lib.sfm_triangulate_tracks(Kc, 3, 4, 8, dummy, dummy, dummy, dummy, 1, 0.0, 9.0, 0, dummy, dummy, dummy, dummy, dummy,
                                      dummy, 1 << 20, None) == EINVAL
    assert lib.sfm_last_error() == b"sfm_triangulate_tracks: min_views must be at least 2"


def test_public_function_rejects_bad_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.multiview.tracks import triangulate_tracks_robust

    def no_device(*_a, **_k):
        raise AssertionError("device work before the checks")

    monkeypatch.setattr(device, "require_gpu", no_device)
    poses, cam, pt, uv, _ = _clean_scene(3, 4, 3)
    good = dict(camera_matrix=K, poses=poses, camera_indices=cam, point_indices=pt, pixels=uv, max_reprojection_error=9.0)
    changes = [
        dict(max_reprojection_error=-1.0), dict(max_reprojection_error=float("nan")), dict(max_reprojection_error=float("inf")),
        dict(max_reprojection_error="many"), dict(max_reprojection_error=None),
        dict(min_views=1), dict(min_views=2.0), dict(min_views=True), dict(min_angle_deg=-1.0), dict(min_angle_deg=float("inf")),
        dict(min_angle_deg=float("nan")), dict(refine_steps=-1), dict(refine_steps=1.5),
        dict(max_hypotheses=0), dict(max_hypotheses=1025), dict(max_hypotheses=64.0), dict(max_hypotheses=True),
        dict(num_points=-1), dict(num_points=2**31 - 1), dict(num_points=3.0),
        dict(camera_matrix=np.eye(4)), dict(camera_matrix=np.zeros((3, 3))),
        dict(poses=poses[:, :11]), dict(pixels=uv[:, :1]), dict(camera_indices=cam[:-1]), dict(point_indices=pt[:-1]),
    ]
    for change in changes:
        with pytest.raises(ValueError):
            triangulate_tracks_robust(**{**good, **change})
    with pytest.raises(TypeError):
        triangulate_tracks_robust(K, poses, cam, pt, uv)            # the error limit is required
    with pytest.raises(AssertionError, match="device work"):
        triangulate_tracks_robust(**good)                            # the checks pass: the next step is the device


def test_lib_reexport():
    from lib.multiview import tracks as lib_tracks
    from structure_from_motion_amd.multiview import tracks

    assert lib_tracks.triangulate_tracks_robust is tracks.triangulate_tracks_robust
    assert lib_tracks.RobustTracksResult is tracks.RobustTracksResult
    assert lib_tracks.triangulate_tracks is tracks.triangulate_tracks


def test_the_app_triangulates_plainly_unless_asked(monkeypatch, capsys):
    from apps import sfm_multi_view as app

    assert app.TRIANGULATIONS == ("plain", "robust")
    assert inspect.signature(app.run).parameters["triangulation"].default == "plain"
    assert inspect.signature(app.Reconstruction.__init__).parameters["triangulation"].default == "plain"
    with pytest.raises(ValueError, match="triangulation"):
        app.run(triangulation="ransac")
    seen = {}
    monkeypatch.setattr(app, "run", lambda *a, **k: seen.update(k) or {})
    monkeypatch.setattr("sys.argv", ["sfm_multi_view.py"])
    app.main()
    assert seen["triangulation"] == "plain"
    monkeypatch.setattr("sys.argv", ["sfm_multi_view.py", "--triangulation", "robust"])
    app.main()
    assert seen["triangulation"] == "robust"
    monkeypatch.setattr("sys.argv", ["sfm_multi_view.py", "--triangulation", "ransac"])
    with pytest.raises(SystemExit):
        app.main()
    capsys.readouterr()


def test_the_stream_case_is_registered():
    import stream_cases

    case = stream_cases.CASES["triangulate_tracks_robust"]
    assert case.entries == ("sfm_triangulate_tracks_robust",) and case.ops == () and not case.synchronising
