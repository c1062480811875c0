"""Bundle adjustment with the iterative Schur solver, host side: the NumPy oracle of tests/bundle_pcg_oracle.py against
the Schur solver of tests/bundle_oracle.py, the C-ABI export and its refusals before any launch, the op registration with
its Meta kernels, the argument checks of the public API and the sequence problem generator (no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bundle_oracle as bo
import bundle_pcg_oracle as pco
from structure_from_motion_amd import synthetic

K = synthetic.BENCH_K


@pytest.mark.parametrize("C,P,seed", [(3, 200, 1), (8, 2000, 2), (16, 2000, 3), (64, 2000, 4)])
def test_tight_pcg_step_equals_schur_step(C, P, seed):
    """With cg_tolerance = 1e-10 and 6F iterations, one PCG step is the Schur solver's step.  Measured gaps over these
    sizes: 2.5e-11 in dc and 1.0e-10 in dX, for steps of 2e-2 .. 3e-2; 1e-8 leaves two orders of margin."""
    pr = synthetic.bundle_problem(C, P, seed=seed)
    prob = pco.Problem(K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], (0,))
    s = prob.system(pr["poses"], pr["points"])
    dc, dX = prob.solve_schur(s, 1e-3)
    (pdc, pdX), k = prob.solve_pcg(s, 1e-3, 1e-10, 6 * (C - 1))
    assert 1 <= k <= 6 * (C - 1)
    assert np.max(np.abs(pdc - dc)) <= 1e-8, np.max(np.abs(pdc - dc))
    assert np.max(np.abs(pdX - dX)) <= 1e-8, np.max(np.abs(pdX - dX))


def test_default_pcg_reaches_dense_minimum_beyond_64_cameras():
    """100 cameras (more than the dense device path takes; the NumPy oracle has no limit).  Measured: both end at
    6171.035455791 (relative gap 7e-16) after 7 and 8 accepted steps."""
    pr = synthetic.bundle_problem(100, 5000, seed=5)
    args = (K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])
    ref = bo.adjust(*args)
    got = pco.adjust_pcg(*args)
    assert got["status"] == bo.OK and got["accepted"] >= 3
    assert abs(got["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"], (got["final_cost"], ref["final_cost"])
    assert got["cg_max"] <= pco.MAX_CG_ITERATIONS and got["cg_iterations"] == sum(got["cg"])
    assert len(got["cg"]) == got["steps"]


def test_oracle_pcg_gauge_and_edge_rules():
    pr = synthetic.bundle_problem(5, 200, per_point=3, seed=8)
    args = (K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])
    out = pco.adjust_pcg(*args, fixed=(3,))
    assert out["accepted"] >= 2 and np.array_equal(out["poses"][3], pr["poses"][3])
    c0 = bo.centre(pr["poses"][3])
    before = np.linalg.norm(bo.centre(pr["poses"][0]) - c0)
    assert abs(np.linalg.norm(bo.centre(out["poses"][0]) - c0) - before) <= 1e-12 * before
    none = pco.adjust_pcg(*args, max_steps=0)
    assert none["steps"] == 0 and none["cg"] == [] and np.array_equal(none["poses"], pr["poses"])
    behind = pr["points"].copy()
    behind[3, 2] = -2.0
    bad = pco.adjust_pcg(K, pr["poses"], behind, pr["camera_indices"], pr["point_indices"], pr["pixels"])
    assert bad["status"] == bo.BAD_START and np.array_equal(bad["points"], behind)
    cam = pr["camera_indices"].copy()
    cam[0] = 5
    bad = pco.adjust_pcg(K, pr["poses"], pr["points"], cam, pr["point_indices"], pr["pixels"])
    assert bad["status"] == bo.BAD_INDEX


def test_sequence_problem_shapes_and_banded_visibility():
    pr = synthetic.sequence_bundle_problem(50, 3000, track_length=4, seed=3)
    assert pr["poses"].shape == (50, 12) and pr["points"].shape == (3000, 3)
    M = 3000 * 4
    assert pr["camera_indices"].shape == (M,) and pr["point_indices"].shape == (M,) and pr["pixels"].shape == (M, 2)
    assert pr["camera_indices"].dtype == np.int32 and pr["point_indices"].dtype == np.int32
    assert np.array_equal(pr["poses"][0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    order = np.lexsort((pr["camera_indices"], pr["point_indices"]))
    cams = pr["camera_indices"][order].reshape(3000, 4)
    assert np.all(np.diff(cams, axis=1) == 1)   # a contiguous window of 4 neighbouring cameras per point
    assert np.bincount(pr["camera_indices"], minlength=50).min() > 0
    # every observation projects in front of its camera and inside the image, near the pixel
    R = pr["poses_true"][pr["camera_indices"], :9].reshape(-1, 3, 3)
    xc = np.einsum("mij,mj->mi", R, pr["points_true"][pr["point_indices"]]) + pr["poses_true"][pr["camera_indices"], 9:]
    assert np.all(xc[:, 2] > 3.0)
    uv = (xc @ K.T)[:, :2] / xc[:, 2:3]
    assert np.all(uv >= 0.0) and np.all(uv[:, 0] < 2 * K[0, 2]) and np.all(uv[:, 1] < 2 * K[1, 2])
    assert np.max(np.abs(uv - pr["pixels"])) < 5.0
    short = synthetic.sequence_bundle_problem(3, 100, track_length=4, seed=1)
    assert short["camera_indices"].shape == (300,)


def test_bundle_pcg_symbols_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    assert "sfm_bundle_adjust_pcg" in _native.SIGNATURES and "sfm_bundle_pcg_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(native_lib, "sfm_bundle_adjust_pcg")
    ws = native_lib.sfm_bundle_pcg_workspace_bytes
    assert ws(65, 3000, 12000) > 0
    assert ws(4096, 2000000, 8000000) > 8000000 * 4 * 6
    assert ws(1, 0, 0) > 0
    assert ws(0, 10, 10) == -1
    assert ws(4, -1, 10) == -1
    assert ws(4, 10, -1) == -1
    assert ws(4, 1 << 31, 10) == -1
    assert ws(4, 10, 1 << 31) == -1


def test_bundle_pcg_rejects_bad_arguments_before_launch(native_lib):
    """Every refusal happens on the host before the launch (no GPU needed): device pointers are never dereferenced."""
    lib = native_lib
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    Kbad = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    Kbad[7] = 0.5
    p = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before the launch

    def call(cams=4, pts=100, obs=400, K_=Kc, fixed=(1, 0, 0, 0), steps=10, cg_it=100, cg_tol=0.1, poses=p, points=p,
             cam=p, pt=p, pix=p, info=p, ws=p, ws_bytes=1 << 40):
        fx = (C.c_uint8 * max(1, len(fixed)))(*fixed) if fixed is not None else None
        return lib.sfm_bundle_adjust_pcg(C.cast(K_, C.c_void_p) if K_ is not None else None, cams, pts, obs,
                                         C.cast(fx, C.c_void_p) if fx is not None else None, poses, points, cam, pt, pix,
                                         steps, cg_it, cg_tol, poses, points, info, ws, ws_bytes, None)

    assert call(cams=0) == -1
    assert call(pts=-1) == -1
    assert call(obs=-1) == -1
    assert call(steps=-1) == -1
    assert call(pts=1 << 31) == -1
    assert call(obs=1 << 31) == -1
    assert call(cg_it=0) == -1 and b"max_cg_iterations" in lib.sfm_last_error()
    assert call(cg_it=-5) == -1
    for tol in (0.0, -0.1, 1.0, 2.0, float("nan"), float("inf")):
        assert call(cg_tol=tol) == -1 and b"cg_tolerance" in lib.sfm_last_error(), tol
    assert call(K_=Kbad) == -1 and b"row 2" in lib.sfm_last_error()
    assert call(K_=None) == -1
    assert call(fixed=None) == -1
    assert call(fixed=(0, 0, 0, 0)) == -1 and b"fixed" in lib.sfm_last_error()
    assert call(cams=100, fixed=(0,) * 100) == -1 and b"fixed" in lib.sfm_last_error()
    assert call(poses=None) == -1 and b"null" in lib.sfm_last_error()
    assert call(points=None) == -1
    assert call(cam=None) == -1
    assert call(pt=None) == -1
    assert call(pix=None) == -1
    assert call(info=None) == -1
    assert call(ws=None) == -1
    assert call(ws_bytes=1000) == -1 and b"workspace" in lib.sfm_last_error()
    assert call(cams=4096, fixed=(1,) + (0,) * 4095, ws_bytes=1000) == -1 and b"workspace" in lib.sfm_last_error()
    assert call(ws=C.c_void_p(0x1008)) == -1 and b"aligned" in lib.sfm_last_error()


def test_bundle_pcg_ops_registered_with_meta_kernels(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "bundle_adjust_pcg" in ops.FUNCTIONAL_OPS and "bundle_adjust_pcg_" in ops.INPLACE_OPS
    assert "Tensor(a!) poses" in str(op.bundle_adjust_pcg_.default._schema)
    meta = dict(device="meta")
    Cn, P, M = 130, 300, 1200

    def args(pixels_cols=2, cg_it=100, cg_tol=0.1):
        return (torch.empty((Cn, 12), dtype=torch.float64, **meta), torch.empty((P, 3), dtype=torch.float64, **meta),
                torch.empty((M,), dtype=torch.int32, **meta), torch.empty((M,), dtype=torch.int32, **meta),
                torch.empty((M, pixels_cols), dtype=torch.float64, **meta), [float(v) for v in K.reshape(9)], [0], 50,
                cg_it, cg_tol)

    poses, points, info = op.bundle_adjust_pcg(*args())
    assert poses.shape == (Cn, 12) and poses.dtype == torch.float64 and poses.device.type == "meta"
    assert points.shape == (P, 3) and points.dtype == torch.float64
    assert info.shape == (5,) and info.dtype == torch.int64
    with pytest.raises(RuntimeError, match="pixels"):
        op.bundle_adjust_pcg(*args(pixels_cols=3))
    with pytest.raises(RuntimeError, match="max_cg_iterations"):
        op.bundle_adjust_pcg(*args(cg_it=0))
    with pytest.raises(RuntimeError, match="cg_tolerance"):
        op.bundle_adjust_pcg(*args(cg_tol=1.0))


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def test_bundle_adjust_validates_solver_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd.bundle import bundle

    _no_device(monkeypatch)
    pr = synthetic.bundle_problem(3, 20, per_point=3, seed=1)
    args = [K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"]]
    with pytest.raises(ValueError, match="linear_solver"):
        bundle.bundle_adjust(*args, linear_solver="cholesky")
    with pytest.raises(ValueError, match="linear_solver"):
        bundle.bundle_adjust(*args, linear_solver=None)
    for bad in (0, -1, 2.5, True, "10"):
        with pytest.raises(ValueError, match="max_cg_iterations"):
            bundle.bundle_adjust(*args, linear_solver="iterative", max_cg_iterations=bad)
    for bad in (0.0, -0.5, 1.0, 3.0, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="cg_tolerance"):
            bundle.bundle_adjust(*args, linear_solver="iterative", cg_tolerance=bad)
    with pytest.raises(ValueError, match="cameras"):
        bundle.bundle_adjust(K, np.zeros((0, 12)), *args[2:], linear_solver="iterative")
    with pytest.raises(ValueError, match="64 cameras"):
        bundle.bundle_adjust(K, np.zeros((65, 12)), *args[2:], linear_solver="dense")
    with pytest.raises(ValueError, match="fixed_cameras"):
        bundle.bundle_adjust(*args, linear_solver="iterative", fixed_cameras=(3,))
    with pytest.raises(ValueError, match="max_steps"):
        bundle.bundle_adjust(*args, linear_solver="iterative", max_steps=-1)


def test_iterative_solver_beyond_64_cameras_reaches_the_device_call(monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.bundle import bundle

    pr = synthetic.sequence_bundle_problem(70, 500, seed=2)
    calls = []

    def fake(poses, points, cam, pt, pixels, K_, fixed, max_steps, max_cg_iterations, cg_tolerance):
        calls.append((poses.shape, points.shape, cam.dtype, list(fixed), max_steps, max_cg_iterations, cg_tolerance))
        return poses, points, torch.zeros(5, dtype=torch.int64)

    monkeypatch.setattr(device, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(device, "to_device", lambda a, dtype=torch.float64: torch.as_tensor(np.asarray(a), dtype=dtype))
    monkeypatch.setattr(device, "bundle_adjust_pcg", fake)
    monkeypatch.setattr(device, "bundle_adjust", lambda *a, **k: (_ for _ in ()).throw(AssertionError("dense path")))
    poses, points, info = bundle.bundle_adjust(K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"],
                                               pr["pixels"], linear_solver="iterative", max_cg_iterations=7,
                                               cg_tolerance=0.25, max_steps=3)
    assert calls == [((70, 12), (500, 3), torch.int32, [0], 3, 7, 0.25)]
    assert isinstance(info, device.BundlePcgInfo) and info.cg_iterations == 0
    assert np.array_equal(poses, pr["poses"])


def test_multi_view_app_view_limits_by_solver():
    """The dense default keeps the 64-view limit; bundle_solver="auto" takes up to 1 024 views.  Refused before any work."""
    from apps import sfm_multi_view

    with pytest.raises(ValueError, match="64"):
        sfm_multi_view.run(views=65, bundle_solver="dense")
    with pytest.raises(ValueError, match="1024"):
        sfm_multi_view.run(views=1025, bundle_solver="auto")
    with pytest.raises(ValueError, match="1024"):
        sfm_multi_view.run(views=1, bundle_solver="auto")
    with pytest.raises(ValueError, match="bundle_solver"):
        sfm_multi_view.run(views=8, bundle_solver="iterative")
