"""Robust losses of both bundle adjusters, host side: the NumPy oracle of tests/bundle_robust_oracle.py
against the squared oracles, the loss functions themselves, what the losses buy against the truth, the C-ABI export and
its refusals before any launch, the op registration with Meta kernels and the argument checks of the public API and the
multi-view app (no GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bundle_oracle as bo
import bundle_pcg_oracle as pco
import bundle_robust_oracle as bro
from structure_from_motion_amd import synthetic

K = synthetic.BENCH_K
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(pr):
    return (pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])


# ---------------------------------------------------------------------------------------------------------------------
# squared through the robust oracle is the squared oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,P,seed", [(6, 300, 5), (8, 600, 12), (16, 2000, 13)])
def test_squared_robust_oracle_equals_the_dense_oracle(C_, P, seed):
    pr = synthetic.bundle_problem(C_, P, seed=seed)
    ref = bo.adjust(*_args(pr))
    got = bro.adjust(*_args(pr), loss="squared", loss_scale=3.0)
    assert np.array_equal(got["poses"], ref["poses"]) and np.array_equal(got["points"], ref["points"])
    for key in ("initial_cost", "final_cost", "steps", "accepted", "status"):
        assert got[key] == ref[key], key


@pytest.mark.parametrize("kind,C_,P,seed,steps", [("random", 16, 2000, 13, 50), ("random", 100, 3000, 14, 6),
                                                  ("sequence", 80, 3000, 15, 6)])
def test_squared_robust_oracle_equals_the_pcg_oracle(kind, C_, P, seed, steps):
    make = synthetic.bundle_problem if kind == "random" else synthetic.sequence_bundle_problem
    pr = make(C_, P, seed=seed)
    ref = pco.adjust_pcg(*_args(pr), max_steps=steps)
    got = bro.adjust_pcg(*_args(pr), max_steps=steps, loss="squared", loss_scale=0.5)
    assert np.array_equal(got["poses"], ref["poses"]) and np.array_equal(got["points"], ref["points"])
    assert got["cg"] == ref["cg"] and got["cg_iterations"] == ref["cg_iterations"] and got["cg_max"] == ref["cg_max"]
    for key in ("initial_cost", "final_cost", "steps", "accepted", "status"):
        assert got[key] == ref[key], key


# ---------------------------------------------------------------------------------------------------------------------
# rho and w
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
@pytest.mark.parametrize("a", [0.5, 2.0, 7.0])
def test_weight_is_the_derivative_of_rho(loss, a):
    """Central difference with h = 1e-6 e: its truncation error is h^2 rho''' / 6, far below the 1e-7 relative bound, and
    its rounding error about eps rho / (h w) <= 1e-9.  Points within h of the Huber kink are left out."""
    e = np.concatenate([np.geomspace(1e-3, 1e6, 400), a * a * np.array([0.25, 0.9, 1.1, 4.0])])
    e = e[np.abs(e - a * a) > 1e-5 * a * a]
    h = 1e-6 * e
    up, _ = bro.rho_and_weight(e + h, loss, a)
    down, _ = bro.rho_and_weight(e - h, loss, a)
    _, w = bro.rho_and_weight(e, loss, a)
    assert np.max(np.abs((up - down) / (2.0 * h) - w) / w) <= 1e-7


@pytest.mark.parametrize("a", [0.5, 2.0, 7.0])
def test_rho_and_weight_at_zero_at_the_huber_kink_and_at_infinity(a):
    a2 = a * a
    for loss in bro.LOSSES:
        f, w = bro.rho_and_weight(np.array([0.0, np.inf]), loss, a)
        assert f[0] == 0.0 and w[0] == 1.0 and f[1] == np.inf
        if loss != "squared":
            assert w[1] == 0.0
    # Huber: rho and w are continuous at e = a2 (one ulp of e moves them by a few ulps)
    e = np.array([a2, np.nextafter(a2, np.inf)])
    f, w = bro.rho_and_weight(e, "huber", a)
    assert f[0] == a2 and w[0] == 1.0
    assert abs(f[1] - f[0]) <= 8 * np.spacing(a2) and abs(w[1] - 1.0) <= 8 * np.spacing(1.0)
    # squared ignores the scale
    e = np.geomspace(1e-3, 1e6, 50)
    f, w = bro.rho_and_weight(e, "squared", a)
    assert np.array_equal(f, e) and np.all(w == 1.0)


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_weighted_squared_cost_majorises_rho(loss):
    """rho is concave in e: rho(e) <= rho(e0) + w(e0) (e - e0) for every pair, up to rounding of the right-hand side."""
    a = 2.0
    grid = np.concatenate([[0.0], np.geomspace(1e-4, 1e7, 300)])
    e0, e = np.meshgrid(grid, grid, indexing="ij")
    f0, w0 = bro.rho_and_weight(e0, loss, a)
    f, _ = bro.rho_and_weight(e, loss, a)
    bound = f0 + w0 * (e - e0)
    assert np.all(f <= bound + 1e-12 * (np.abs(f0) + np.abs(w0 * e) + np.abs(w0 * e0) + 1.0))
    assert np.array_equal(np.diag(f), np.diag(bound))   # touches at e = e0


# ---------------------------------------------------------------------------------------------------------------------
# what the losses buy: rotation error against the truth
# ---------------------------------------------------------------------------------------------------------------------
def test_cauchy_recovers_the_clean_result_from_gross_outliers():
    """16 x 2 000, 5 % of the pixels shifted by up to +-200 px, 50 steps.  Measured: squared on the clean data 4.8e-4 rad,
    squared on the corrupted data 9.2e-2 rad, Cauchy (scale 2) on the corrupted data 5.2e-4 rad (1.08 x and 0.006 x)."""
    pr = synthetic.bundle_problem(16, 2000, seed=13)
    bad, mask = synthetic.corrupt_observations(pr, 0.05, 200.0, seed=113)
    assert 0.03 * len(mask) < mask.sum() < 0.07 * len(mask)
    clean = bro.rotation_error(bo.adjust(*_args(pr))["poses"], pr["poses_true"])
    squared = bro.rotation_error(bo.adjust(*_args(bad))["poses"], pr["poses_true"])
    out = bro.adjust(*_args(bad), loss="cauchy", loss_scale=2.0)
    cauchy = bro.rotation_error(out["poses"], pr["poses_true"])
    print(f"clean squared {clean:.3e}  corrupted squared {squared:.3e}  corrupted cauchy {cauchy:.3e}")
    assert out["status"] == bo.OK
    assert cauchy <= 2.0 * clean, (cauchy, clean)
    assert cauchy <= 0.1 * squared, (cauchy, squared)
    assert np.median(out["weights"][mask]) < 0.01 < 0.5 < np.median(out["weights"][~mask])
    assert np.max(np.abs(out["points"])) < 10.0   # Cauchy re-descends: no point escapes


@pytest.mark.parametrize("C_,P,seed", [(16, 2000, 13), (8, 2000, 12), (3, 200, 11)])
def test_huber_halves_the_error_from_moderate_outliers(C_, P, seed):
    """5 % of the pixels shifted by up to +-40 px, 10 steps on both sides.  Measured ratios to the squared run: 0.19,
    0.07, 0.22.  Huber's tail keeps a pull of 2 a per pixel, so it is tested on moderate outliers."""
    pr = synthetic.bundle_problem(C_, P, seed=seed)
    bad, _ = synthetic.corrupt_observations(pr, 0.05, 40.0, seed=seed + 100)
    squared = bro.rotation_error(bo.adjust(*_args(bad), max_steps=10)["poses"], pr["poses_true"])
    out = bro.adjust(*_args(bad), max_steps=10, loss="huber", loss_scale=2.0)
    huber = bro.rotation_error(out["poses"], pr["poses_true"])
    print(f"{C_} x {P}: squared {squared:.3e}  huber {huber:.3e}  ratio {huber / squared:.3f}")
    assert huber <= 0.5 * squared, (huber, squared)
    assert np.max(np.abs(out["points"])) < 10.0


def test_corrupt_observations_recipe():
    pr = synthetic.bundle_problem(4, 500, seed=3)
    bad, mask = synthetic.corrupt_observations(pr, 0.1, 50.0, seed=9)
    again, mask2 = synthetic.corrupt_observations(pr, 0.1, 50.0, seed=9)
    assert np.array_equal(bad["pixels"], again["pixels"]) and np.array_equal(mask, mask2)
    assert mask.dtype == bool and mask.shape == (len(pr["pixels"]),)
    assert bad["pixels"] is not pr["pixels"] and np.array_equal(bad["pixels"][~mask], pr["pixels"][~mask])
    shift = bad["pixels"][mask] - pr["pixels"][mask]
    assert np.all(np.abs(shift) <= 50.0) and np.max(np.abs(shift)) > 40.0
    rng = np.random.default_rng(9)
    want = rng.random(len(mask)) < 0.1
    assert np.array_equal(mask, want)
    assert np.array_equal(shift, (pr["pixels"][mask] + rng.uniform(-50.0, 50.0, (int(want.sum()), 2))) - pr["pixels"][mask])
    for key in ("poses", "points", "camera_indices", "point_indices", "poses_true"):
        assert bad[key] is pr[key]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI, the ops, the public API and the app
# ---------------------------------------------------------------------------------------------------------------------
def test_robust_symbols_in_the_header_and_bound(native_lib):
    from structure_from_motion_amd import _native

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header
    for name in ("SFM_BUNDLE_LOSS_SQUARED 0", "SFM_BUNDLE_LOSS_HUBER 1", "SFM_BUNDLE_LOSS_CAUCHY 2",
                 "typedef struct sfm_bundle_options", "int sfm_bundle_adjust_ex(", "int sfm_bundle_adjust_pcg_ex(",
                 "int64_t sfm_bundle_pcg_workspace_bytes_ex("):
        assert name in header, name
    assert "sfm_bundle_adjust_ex" in _native.SIGNATURES and "sfm_bundle_adjust_pcg_ex" in _native.SIGNATURES
    assert "sfm_bundle_pcg_workspace_bytes_ex" in _native.OTHER_SYMBOLS
    assert hasattr(native_lib, "sfm_bundle_adjust_ex") and hasattr(native_lib, "sfm_bundle_adjust_pcg_ex")
    assert C.sizeof(_native.BundleOptions) == 16
    assert _native.BUNDLE_LOSSES == ("squared", "huber", "cauchy")
    # the plain sizes keep their values; only a non-squared iterative call needs more: sqrt(w), 8 B per observation
    ws, ws_ex = native_lib.sfm_bundle_pcg_workspace_bytes, native_lib.sfm_bundle_pcg_workspace_bytes_ex
    Cn, P, M = 100, 3000, 15000
    plain = ws(Cn, P, M)
    assert ws_ex(Cn, P, M, None) == plain
    assert ws_ex(Cn, P, M, C.byref(_native.BundleOptions(0, 0, 5.0))) == plain
    for loss in (1, 2):
        grown = ws_ex(Cn, P, M, C.byref(_native.BundleOptions(loss, 0, 2.0)))
        assert 8 * M <= grown - plain < 8 * M + 256
    for bad in (_native.BundleOptions(3, 0, 2.0), _native.BundleOptions(-1, 0, 2.0), _native.BundleOptions(1, 1, 2.0),
                _native.BundleOptions(1, 0, 0.0), _native.BundleOptions(2, 0, float("nan"))):
        assert ws_ex(Cn, P, M, C.byref(bad)) == -1
    assert ws_ex(0, P, M, None) == -1


@pytest.mark.parametrize("solver", ["dense", "pcg"])
def test_robust_entry_points_reject_bad_options_before_launch(native_lib, solver):
    """Every refusal happens on the host before the launch (no GPU needed): device pointers are never dereferenced."""
    from structure_from_motion_amd import _native

    lib = native_lib
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    p = C.c_void_p(0x1000)
    fx = (C.c_uint8 * 4)(1, 0, 0, 0)

    def call(options, ws_bytes=1000):
        opt = C.byref(options) if options is not None else None
        head = (C.cast(Kc, C.c_void_p), 4, 100, 400, C.cast(fx, C.c_void_p), p, p, p, p, p, 10)
        if solver == "dense":
            return lib.sfm_bundle_adjust_ex(*head, p, p, p, p, ws_bytes, None, opt)
        return lib.sfm_bundle_adjust_pcg_ex(*head, 100, 0.1, p, p, p, p, ws_bytes, None, opt)

    # good options get as far as the workspace check (still before any launch)
    for good in (None, _native.BundleOptions(0, 0, 1.0), _native.BundleOptions(1, 0, 2.0), _native.BundleOptions(2, 0, 1e6)):
        assert call(good) == -1 and b"workspace" in lib.sfm_last_error()
    for loss in (-1, 3, 100):
        assert call(_native.BundleOptions(loss, 0, 2.0), ws_bytes=1 << 40) == -1 and b"options" in lib.sfm_last_error()
    assert call(_native.BundleOptions(2, 7, 2.0), ws_bytes=1 << 40) == -1 and b"options" in lib.sfm_last_error()
    for scale in (0.0, -2.0, float("nan"), float("inf"), float("-inf")):
        for loss in (0, 1, 2):
            assert call(_native.BundleOptions(loss, 0, scale), ws_bytes=1 << 40) == -1
            assert b"options" in lib.sfm_last_error(), (loss, scale)


def test_robust_ops_registered_with_meta_kernels(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    for name in ("bundle_adjust_robust", "bundle_adjust_pcg_robust"):
        assert name in ops.FUNCTIONAL_OPS and name + "_" in ops.INPLACE_OPS
        assert "int loss, float loss_scale" in str(getattr(op, name).default._schema)
        assert "Tensor(a!) poses" in str(getattr(op, name + "_").default._schema)
    # no existing schema changed
    assert "loss" not in str(op.bundle_adjust.default._schema) and "loss" not in str(op.bundle_adjust_pcg.default._schema)
    meta = dict(device="meta")
    Cn, P, M = 20, 300, 1200

    def args(*tail):
        return (torch.empty((Cn, 12), dtype=torch.float64, **meta), torch.empty((P, 3), dtype=torch.float64, **meta),
                torch.empty((M,), dtype=torch.int32, **meta), torch.empty((M,), dtype=torch.int32, **meta),
                torch.empty((M, 2), dtype=torch.float64, **meta), [float(v) for v in K.reshape(9)], [0], 50) + tail

    poses, points, info = op.bundle_adjust_robust(*args(2, 2.0))
    assert poses.shape == (Cn, 12) and points.shape == (P, 3) and poses.device.type == "meta"
    assert info.shape == (4,) and info.dtype == torch.int64
    poses, points, info = op.bundle_adjust_pcg_robust(*args(100, 0.1, 1, 2.0))
    assert poses.shape == (Cn, 12) and points.shape == (P, 3) and info.shape == (5,) and info.dtype == torch.int64
    rec = torch.empty(4, dtype=torch.int64, **meta)
    a = args()
    assert op.bundle_adjust_robust_(a[0], a[1], *a[2:], 1, 2.0, rec) is None
    rec = torch.empty(5, dtype=torch.int64, **meta)
    assert op.bundle_adjust_pcg_robust_(a[0], a[1], *a[2:], 100, 0.1, 2, 2.0, rec) is None
    with pytest.raises(RuntimeError, match="loss"):
        op.bundle_adjust_robust(*args(3, 2.0))
    with pytest.raises(RuntimeError, match="loss_scale"):
        op.bundle_adjust_robust(*args(1, 0.0))
    with pytest.raises(RuntimeError, match="loss_scale"):
        op.bundle_adjust_pcg_robust(*args(100, 0.1, 2, float("nan")))
    with pytest.raises(RuntimeError, match="cg_tolerance"):
        op.bundle_adjust_pcg_robust(*args(100, 1.0, 2, 2.0))


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def test_bundle_adjust_validates_the_loss_before_device_work(monkeypatch):
    from lib.bundle.bundle import bundle_adjust
    from structure_from_motion_amd import device
    from structure_from_motion_amd.bundle import bundle

    assert bundle.LOSSES == device.BUNDLE_LOSSES == ("squared", "huber", "cauchy")
    _no_device(monkeypatch)
    pr = synthetic.bundle_problem(3, 20, per_point=3, seed=1)
    for solver in ("dense", "iterative"):
        for bad in ("tukey", "Huber", "", None, 1, b"cauchy"):
            with pytest.raises(ValueError, match="loss"):
                bundle_adjust(*_args(pr), linear_solver=solver, loss=bad)
        for bad in (0.0, -2.0, float("nan"), float("inf"), "2.0", None, True, [2.0]):
            for loss in ("squared", "huber", "cauchy"):
                with pytest.raises(ValueError, match="loss_scale"):
                    bundle_adjust(*_args(pr), linear_solver=solver, loss=loss, loss_scale=bad)
    # good arguments reach the device
    for loss in ("squared", "huber", "cauchy"):
        with pytest.raises(AssertionError, match="device touched"):
            bundle_adjust(*_args(pr), loss=loss, loss_scale=np.float64(2.0))
    with pytest.raises(AssertionError, match="device touched"):
        bundle_adjust(*_args(pr), loss="cauchy", loss_scale=3)


def test_public_api_passes_the_loss_to_the_device_call_only_when_robust(monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.bundle import bundle

    pr = synthetic.bundle_problem(3, 20, per_point=3, seed=1)
    calls = []

    def fake(n):
        def f(poses, points, *rest, **kw):
            calls.append(kw)
            return poses, points, torch.zeros(n, dtype=torch.int64)
        return f

    monkeypatch.setattr(device, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(device, "to_device", lambda a, dtype=torch.float64: torch.as_tensor(np.asarray(a), dtype=dtype))
    monkeypatch.setattr(device, "bundle_adjust", fake(4))
    monkeypatch.setattr(device, "bundle_adjust_pcg", fake(5))
    bundle.bundle_adjust(*_args(pr))
    bundle.bundle_adjust(*_args(pr), loss="squared", loss_scale=7.0)
    bundle.bundle_adjust(*_args(pr), loss="huber", loss_scale=3)
    bundle.bundle_adjust(*_args(pr), linear_solver="iterative", loss="cauchy")
    assert calls == [{}, {}, dict(loss="huber", loss_scale=3.0), dict(loss="cauchy", loss_scale=1.0)]


def test_device_layer_refuses_an_unknown_loss_before_the_op(native_lib):
    from structure_from_motion_amd import device

    for fn in (device.bundle_adjust, device.bundle_adjust_pcg):
        with pytest.raises(ValueError, match="loss"):
            fn(None, None, None, None, None, K, loss="tukey")
        with pytest.raises(ValueError, match="loss_scale"):
            fn(None, None, None, None, None, K, loss="huber", loss_scale=0.0)


def test_multi_view_app_refuses_an_unknown_loss_before_any_work():
    from apps import sfm_multi_view

    assert sfm_multi_view.BUNDLE_LOSSES == ("squared", "huber", "cauchy")
    with pytest.raises(ValueError, match="bundle_loss"):
        sfm_multi_view.run(bundle_loss="tukey")
    with pytest.raises(ValueError, match="bundle_loss_scale"):
        sfm_multi_view.run(bundle_loss="cauchy", bundle_loss_scale=0.0)
    with pytest.raises(ValueError, match="bundle_loss_scale"):
        sfm_multi_view.run(bundle_loss="cauchy", bundle_loss_scale=float("nan"))
