"""Triangulation of multi-view tracks, host side: the NumPy oracle of tests/tracks_oracle.py (noise-free recovery, the
two-view case against the reference's DLT, its LM gradient and every status), the C-ABI export and its refusals before
any launch, the op registration with its Meta kernels, the argument checks of the public API and the ``lib`` re-export
(no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_cases as gc
import tracks_cases as tc
import tracks_oracle as to
from oracle import sfm_oracle
from structure_from_motion_amd import synthetic

K = synthetic.BENCH_K


def _scene(views=6, points=200, seed=3, noise_px=0.0, outliers=0.0):
    return synthetic.multi_view_scene(views, points, seed, noise_px, outliers)


def _tri(sc, poses=None, **kw):
    return to.triangulate(sc["K"], sc["poses_true"] if poses is None else poses, sc["camera_indices"],
                          sc["point_indices"], sc["pixels"], len(sc["points_true"]), **kw)


def test_multi_view_scene_has_mixed_track_lengths():
    sc = synthetic.multi_view_scene()
    lengths = np.bincount(sc["point_indices"])
    assert len(lengths) == 2000 and lengths.min() >= 2 and lengths.max() == 8
    assert len(np.unique(lengths)) == 7
    assert 0.15 < np.mean(sc["is_outlier"]) < 0.25
    assert np.array_equal(sc["poses_true"][0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))


def test_oracle_recovers_noise_free_tracks():
    sc = _scene()
    out = _tri(sc)
    assert np.all(out["status"] == to.OK) and out["info"]["points_ok"] == len(sc["points_true"])
    assert np.max(np.abs(out["points"] - sc["points_true"])) <= 1e-9
    assert np.max(out["obs_error"]) <= 1e-12
    refined = _tri(sc, refine_steps=10)
    assert np.max(np.abs(refined["points"] - sc["points_true"])) <= 1e-9


def test_oracle_two_view_track_is_the_reference_dlt():
    """A two-observation track solves the reference's two-view DLT (oracle/sfm_oracle.py::triangulate_dlt), with any
    two poses, on noisy pixels."""
    sc = _scene(noise_px=0.7)
    keep = np.isin(sc["camera_indices"], (2, 4))
    cam, pt, uv = sc["camera_indices"][keep], sc["point_indices"][keep], sc["pixels"][keep]
    out = to.triangulate(K, sc["poses_true"], cam, pt, uv, len(sc["points_true"]))
    both = np.nonzero(np.bincount(pt, minlength=len(sc["points_true"])) == 2)[0]
    assert len(both) > 50
    a = np.array([uv[(pt == p) & (cam == 2)][0] for p in both])
    b = np.array([uv[(pt == p) & (cam == 4)][0] for p in both])
    P = [K @ np.hstack([sc["poses_true"][c, :9].reshape(3, 3), sc["poses_true"][c, 9:, None]]) for c in (2, 4)]
    ref = sfm_oracle.triangulate_dlt(np.hstack([a, b]), P[0], P[1])
    assert np.max(np.abs(out["points"][both] - ref) / np.linalg.norm(ref, axis=1, keepdims=True)) <= 1e-9


@pytest.mark.parametrize("world", ["id", "turned"])
@pytest.mark.parametrize("camera", ["bench", "skew", "affine"])
def test_oracle_gradient_matches_finite_differences(camera, world):
    """g = J^T r is half the gradient of F = sum e; H is J^T J; at cameras with K01 and K10 and in a turned world too
    (tests/geometry_cases.py)."""
    K = gc.CAMERAS[camera]
    sc = synthetic.multi_view_scene(6, 200, 3, 1.0, 0.0, K=K)
    sc = dict(sc, poses_true=gc.poses_to(world, sc["poses_true"]), points_true=gc.points_to(world, sc["points_true"]))
    out = _tri(sc)
    order = np.lexsort((np.arange(len(sc["point_indices"])), sc["point_indices"]))
    for p in (0, 7, 31):
        obs = order[sc["point_indices"][order] == p][None, :]
        c = sc["camera_indices"][obs]
        R, t, uv = sc["poses_true"][c, :9].reshape(1, -1, 3, 3), sc["poses_true"][c, 9:], sc["pixels"][obs]
        X = out["points"][p][None] + 0.01
        F, H, g = to.point_system(X, R, t, K, uv)
        h = 1e-6
        fd = np.zeros(3)
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            fd[k] = (to.point_system(X + d, R, t, K, uv)[0][0] - to.point_system(X - d, R, t, K, uv)[0][0]) / (4.0 * h)
        assert np.max(np.abs(fd - g[0])) <= 1e-5 * np.max(np.abs(g[0])), p
        assert np.all(np.linalg.eigvalsh(H[0]) > 0)


def test_oracle_refinement_lowers_the_cost():
    sc = _scene(noise_px=1.0)
    lin = _tri(sc)
    ref = _tri(sc, refine_steps=10)
    assert np.sum(ref["obs_error"]) < np.sum(lin["obs_error"])
    per_point_lin = np.bincount(sc["point_indices"], weights=lin["obs_error"])
    per_point_ref = np.bincount(sc["point_indices"], weights=ref["obs_error"])
    assert np.all(per_point_ref <= per_point_lin)
    assert 1 <= ref["info"]["max_refine_steps_taken"] <= 10


def test_oracle_produces_every_status():
    """One constructed track per status, in one call (tests/tracks_cases.py::every_status, its points 0 .. 6)."""
    case = tc.every_status()
    poses, cam, pt, uv = case["poses"], case["cam"].tolist(), case["pt"], case["uv"]
    out = to.triangulate(K, poses, np.array(cam), pt, uv, case["P"], min_angle=np.radians(1.0), max_error=4.0)
    assert out["status"][:7].tolist() == [to.OK, to.FEW_VIEWS, to.DEGENERATE, to.BEHIND, to.SMALL_ANGLE, to.LARGE_ERROR,
                                          to.FEW_VIEWS]
    assert np.all(np.isnan(out["points"][[1, 2, 6]])) and np.all(np.isnan(out["angle"][[1, 2, 6]]))
    assert np.all(np.isfinite(out["points"][[0, 3, 4, 5]]))
    assert np.isnan(out["obs_error"][3]) and np.all(np.isnan(out["obs_error"][4:6]))
    assert out["info"] == dict(status=0, points_ok=1, max_refine_steps_taken=0)
    bad = to.triangulate(K, poses, np.array(cam[:-1] + [4]), pt, uv, case["P"])
    assert np.all(bad["status"] == to.BAD_INDEX) and bad["info"]["status"] == 1
    assert np.all(np.isnan(bad["points"])) and np.all(np.isnan(bad["obs_error"])) and np.all(np.isnan(bad["angle"]))


def test_tracks_symbols_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    assert "sfm_triangulate_tracks" in _native.SIGNATURES and "sfm_tracks_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(native_lib, "sfm_triangulate_tracks")
    assert native_lib.sfm_tracks_workspace_bytes(100000, 400000) >= 4 * (100000 * 2 + 400000)
    assert native_lib.sfm_tracks_workspace_bytes(0, 0) > 0
    assert native_lib.sfm_tracks_workspace_bytes(-1, 10) == -1
    assert native_lib.sfm_tracks_workspace_bytes(10, -1) == -1
    assert native_lib.sfm_tracks_workspace_bytes((1 << 31) - 1, 10) == -1
    assert native_lib.sfm_tracks_workspace_bytes(10, 1 << 31) == -1


def test_tracks_rejects_bad_arguments_before_launch(native_lib):
    """Every refusal happens on the host before the launch (no GPU needed): device pointers are never dereferenced."""
    lib = native_lib
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    Kbad = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    Kbad[6] = 0.1
    p = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before the launch

    def call(cams=4, pts=100, obs=400, K_=Kc, poses=p, cam=p, pt=p, pix=p, min_views=2, min_angle=0.0, max_error=float("inf"),
             refine=0, X=p, status=p, info=p, ws=p, ws_bytes=1 << 40):
        return lib.sfm_triangulate_tracks(C.cast(K_, C.c_void_p) if K_ is not None else None, cams, pts, obs, poses, cam, pt,
                                          pix, min_views, min_angle, max_error, refine, X, status, None, None, info, ws,
                                          ws_bytes, None)

    assert call(cams=-1) == -1 and b"negative" in lib.sfm_last_error()
    assert call(pts=-1) == -1
    assert call(obs=-1) == -1
    assert call(pts=(1 << 31) - 1) == -1 and b"2^31" in lib.sfm_last_error()
    assert call(obs=1 << 31) == -1
    assert call(min_views=1) == -1 and b"min_views" in lib.sfm_last_error()
    assert call(min_angle=-0.1) == -1 and b"min_angle" in lib.sfm_last_error()
    assert call(min_angle=float("nan")) == -1
    assert call(min_angle=float("inf")) == -1
    assert call(max_error=-1.0) == -1 and b"max_error" in lib.sfm_last_error()
    assert call(max_error=float("nan")) == -1
    assert call(refine=-1) == -1 and b"refine_steps" in lib.sfm_last_error()
    assert call(K_=Kbad) == -1 and b"row 2" in lib.sfm_last_error()
    assert call(K_=None) == -1
    for name in ("poses", "cam", "pt", "pix", "X", "status", "info", "ws"):
        assert call(**{name: None}) == -1 and b"null" in lib.sfm_last_error(), name
    assert call(ws_bytes=1000) == -1 and b"workspace" in lib.sfm_last_error()
    assert call(ws=C.c_void_p(0x1008)) == -1 and b"aligned" in lib.sfm_last_error()


def test_tracks_ops_registered_with_meta_kernels(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "triangulate_tracks" in ops.FUNCTIONAL_OPS and "triangulate_tracks_" in ops.INPLACE_OPS
    schema = str(op.triangulate_tracks_.default._schema)
    assert "Tensor(a!) points_out" in schema and "Tensor(e!) info" in schema
    meta = dict(device="meta")
    Cn, P, M = 7, 300, 1200
    args = (torch.empty((Cn, 12), dtype=torch.float64, **meta), torch.empty((M,), dtype=torch.int32, **meta),
            torch.empty((M,), dtype=torch.int32, **meta), torch.empty((M, 2), dtype=torch.float64, **meta))
    X, status, err, angle, info = op.triangulate_tracks(*args, P, [float(v) for v in K.reshape(9)], 2, 0.0, float("inf"), 10)
    assert X.shape == (P, 3) and X.dtype == torch.float64 and X.device.type == "meta"
    assert status.shape == (P,) and status.dtype == torch.uint8
    assert err.shape == (M,) and err.dtype == torch.float64
    assert angle.shape == (P,) and angle.dtype == torch.float64
    assert info.shape == (4,) and info.dtype == torch.int64
    with pytest.raises(RuntimeError, match="pixels"):
        op.triangulate_tracks(*args[:3], torch.empty((M, 3), dtype=torch.float64, **meta), P,
                              [float(v) for v in K.reshape(9)], 2, 0.0, float("inf"), 0)
    with pytest.raises(RuntimeError, match="min_views"):
        op.triangulate_tracks(*args, P, [float(v) for v in K.reshape(9)], 1, 0.0, float("inf"), 0)


def test_triangulate_tracks_validates_before_device_work(monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.multiview import tracks

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)
    sc = _scene(views=3, points=20)
    args = [K, sc["poses_true"], sc["camera_indices"], sc["point_indices"], sc["pixels"]]

    def call(i=None, value=None, **kw):
        a = list(args)
        if i is not None:
            a[i] = value
        return tracks.triangulate_tracks(*a, **kw)

    K_bad = K.copy()
    K_bad[2, 1] = 1.0
    with pytest.raises(ValueError, match="row 2"):
        call(0, K_bad)
    with pytest.raises(ValueError, match="poses"):
        call(1, sc["poses_true"][:, :9])
    with pytest.raises(ValueError, match="camera_indices"):
        call(2, sc["camera_indices"][:-1])
    with pytest.raises(ValueError, match="integers"):
        call(3, sc["point_indices"].astype(np.float64))
    with pytest.raises(ValueError, match="32 bits"):
        call(3, sc["point_indices"].astype(np.int64) + (1 << 40))
    with pytest.raises(ValueError, match="pixels"):
        call(4, sc["pixels"][:, :1])
    with pytest.raises(ValueError, match="num_points"):
        call(num_points=-1)
    with pytest.raises(ValueError, match="num_points"):
        call(num_points=2.5)
    with pytest.raises(ValueError, match="min_views"):
        call(min_views=1)
    with pytest.raises(ValueError, match="min_angle_deg"):
        call(min_angle_deg=-1.0)
    with pytest.raises(ValueError, match="min_angle_deg"):
        call(min_angle_deg=float("nan"))
    with pytest.raises(ValueError, match="max_reprojection_error"):
        call(max_reprojection_error=-1.0)
    with pytest.raises(ValueError, match="refine_steps"):
        call(refine_steps=-1)
    with pytest.raises(ValueError, match="refine_steps"):
        call(refine_steps=True)


def test_lib_reexports_triangulate_tracks():
    from lib.multiview import tracks as lib_tracks
    from structure_from_motion_amd.multiview import tracks

    assert lib_tracks.triangulate_tracks is tracks.triangulate_tracks


def test_multi_view_app_refuses_more_than_64_views():
    from apps import sfm_multi_view

    with pytest.raises(ValueError, match="64"):
        sfm_multi_view.run(views=65)
