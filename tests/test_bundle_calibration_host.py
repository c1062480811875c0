"""The calibrating bundle adjuster without a GPU (sfm_bundle_adjust_calibrated): the NumPy oracle against
finite differences, against itself (dense and Schur solver) and against ``bundle_oracle`` with nothing to refine; the
refusals of the C entry point; the ops and their Meta kernels; the argument checks of ``bundle_adjust`` and of the app."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import bundle_calibration_cases as cases   # registers the stream case of the new entry point (see that module)
import bundle_calibration_oracle as bco
import bundle_oracle as bo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "op_schemas_before_calibration.json")


def _args(pr, K=None):
    return (pr["K"] if K is None else K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_intrinsic_rows_match_central_differences_of_the_projection():
    pr = cases.ring_problem(4, 30, seed=3)
    K = np.array([[830.0, 2.0, 325.0], [1.5, 845.0, 236.0], [0.0, 0.0, 1.0]])   # skew and K10: the whole block scales with f
    cam, pt, uv = pr["camera_indices"], pr["point_indices"], pr["pixels"]
    e, r, _, _ = bo.residuals(pr["poses"], pr["points"], cam, pt, uv, K)
    Jq = bco.intrinsic_rows(r, uv, K, np.isfinite(e))
    idx = np.arange(3)
    for k, h in enumerate((1e-3, 1e-3, 1e-3)):
        d = np.zeros(3)
        d[k] = h
        plus = bco.project(pr["poses"], pr["points"], cam, pt, bco.stepped(K, idx, d))
        minus = bco.project(pr["poses"], pr["points"], cam, pt, bco.stepped(K, idx, -d))
        numeric = (plus - minus) / (2.0 * h)
        # the projection is affine in cx and cy and, with the block scaled as a whole, in f: only rounding is left,
        # about eps * 1000 px / h = 2e-10
        assert np.max(np.abs(numeric - Jq[:, :, k])) < 1e-8, k
    # a zero entry of the block stays exactly zero, and the other entries keep their proportions
    Kz = bco.stepped(cases.RING_K, idx, np.array([17.0, 0.0, 0.0]))
    assert Kz[0, 1] == 0.0 and Kz[1, 0] == 0.0 and Kz[0, 0] == 817.0
    assert abs(Kz[1, 1] / Kz[0, 0] - 810.0 / 800.0) < 1e-15
    for bad in (-800.0, -900.0, np.nan, np.inf):
        assert bco.stepped(cases.RING_K, idx, np.array([bad, 0.0, 0.0])) is None
    assert bco.stepped(cases.RING_K, np.array([1, 2]), np.array([3.0, 4.0]))[0, 2] == 323.0


@pytest.mark.parametrize("name", list(cases.parity_cases()))
def test_dense_and_schur_oracle_steps_agree(name):
    """One damped step of both solvers at the start, at three dampings: the same system solved in two orders."""
    c = cases.parity_cases()[name]
    pr = c["pr"]
    prob = bco.Problem(c["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"],
                       c["fixed"], c["refine"], **c["loss"])
    s = prob.system(pr["poses"], pr["points"])
    for lam in (1e-3, 1e-1, 1e-6):
        a, b = prob.solve_schur(s, lam), prob.solve_dense(s, lam)
        for x, y in zip(a, b):
            assert x.shape == y.shape
            assert np.max(np.abs(x - y), initial=0.0) <= 1e-9 * max(1.0, np.max(np.abs(y), initial=0.0)), (name, lam)
        assert len(a[2]) == len(prob.idx) and np.all(a[0][prob.fixed] == 0.0) and np.all(a[1][~prob.moving] == 0.0)


@pytest.mark.parametrize("name", list(cases.parity_cases()))
def test_the_recorded_oracle_spread_holds(name):
    """The device's tolerances are ten times the spread between the oracle's two solvers over the parity cases
    (cases.SPREAD, profiles/bundle_calibration/README.md): every case stays inside the recorded spread."""
    c = cases.parity_cases()[name]
    a = bco.adjust(*_args(c["pr"], c["K"]), c["fixed"], cases.PARITY_STEPS, c["refine"], solver="schur", **c["loss"])
    b = bco.adjust(*_args(c["pr"], c["K"]), c["fixed"], cases.PARITY_STEPS, c["refine"], solver="dense", **c["loss"])
    gaps = {k: float(np.max(np.abs(a[k] - b[k]))) for k in ("poses", "points", "K")}
    gaps["cost"] = abs(a["final_cost"] - b["final_cost"]) / b["final_cost"]
    print(name, a["steps"], a["accepted"], gaps)
    assert (a["steps"], a["accepted"], a["status"]) == (b["steps"], b["accepted"], b["status"])
    assert a["accepted"] >= 3
    for out in (a, b):   # every accept test is decided well above rounding
        assert min(abs(new - cur) / cur for cur, new in out["trace"]) >= cases.MIN_MARGIN, out["trace"]
    for k, gap in gaps.items():
        assert gap <= cases.SPREAD[k], (name, k, gap)


@pytest.mark.parametrize("seed,fixed", [(0, (0,)), (1, (0, 2))])
def test_oracle_without_a_free_intrinsic_is_bundle_oracle_bit_for_bit(seed, fixed):
    from structure_from_motion_amd import synthetic

    pr = synthetic.bundle_problem(5, 60, seed=seed)
    ref = bo.adjust(*_args(pr), fixed, 12)
    for solver in ("schur", "dense"):
        want = ref if solver == "schur" else bo.adjust(*_args(pr), fixed, 12, solver="dense")
        got = bco.adjust(*_args(pr), fixed, 12, (), solver=solver)
        assert got["poses"].tobytes() == want["poses"].tobytes() and got["points"].tobytes() == want["points"].tobytes()
        assert (got["initial_cost"], got["final_cost"], got["steps"], got["accepted"], got["status"]) == \
            (want["initial_cost"], want["final_cost"], want["steps"], want["accepted"], want["status"])
        assert got["K"].tobytes() == np.asarray(pr["K"], dtype=np.float64).tobytes()
    assert ref["accepted"] >= 3


def test_oracle_recovers_the_focal_length_on_the_ring():
    """The numbers of the feature's recovery test, on the oracle: 5 % off comes back within 0.7 % at 0.5 px noise, and to
    cases.EXACT_FOCAL without noise."""
    for seed in range(3):
        pr = cases.ring_problem(6, 96, seed=seed)
        K = cases.wrong_camera(pr["K"], 0.05)
        held = bco.adjust(*_args(pr, K))
        for refine in (("focal",), ("focal", "principal_point")):
            out = bco.adjust(*_args(pr, K), refine=refine)
            assert abs(out["K"][0, 0] / 800.0 - 1.0) < 0.007 and out["final_cost"] < held["final_cost"], (seed, refine)
            assert out["K"][0, 1] == 0.0 and out["K"][1, 0] == 0.0
            assert abs(out["K"][1, 1] / out["K"][0, 0] - 810.0 / 800.0) < 1e-14
    for seed in range(3):
        pr = cases.ring_problem(6, 96, seed=seed, noise_px=0.0)
        out = bco.adjust(*_args(pr, cases.wrong_camera(pr["K"], 0.05)), refine=("focal",))
        assert abs(out["K"][0, 0] / 800.0 - 1.0) <= cases.EXACT_FOCAL, (seed, out["K"][0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_in_the_header_and_bound(native_lib):
    from structure_from_motion_amd import _native

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    for text in ("#define SFM_BUNDLE_REFINE_FOCAL 1", "#define SFM_BUNDLE_REFINE_PRINCIPAL_POINT 2",
                 "typedef struct sfm_bundle_calibration_options", "int sfm_bundle_adjust_calibrated(",
                 "int64_t sfm_bundle_calibrated_workspace_bytes("):
        assert text in header, text
    assert len(_native.SIGNATURES["sfm_bundle_adjust_calibrated"]) == len(_native.SIGNATURES["sfm_bundle_adjust_ex"]) + 1
    assert "sfm_bundle_calibrated_workspace_bytes" in _native.OTHER_SYMBOLS
    assert C.sizeof(_native.BundleCalibrationOptions) == 24 and _native.BUNDLE_REFINE == {"focal": 1, "principal_point": 2}


def test_workspace_size(native_lib):
    plain, cal = native_lib.sfm_bundle_workspace_bytes, native_lib.sfm_bundle_calibrated_workspace_bytes
    for sizes in ((1, 0, 0), (3, 24, 72), (31, 200, 800), (32, 200, 800), (64, 5000, 20000), (64, 500000, 2000000)):
        assert cal(*sizes) >= plain(*sizes) > 0, sizes
        # W_qp per point (72 B) is the only part that grows with the problem beyond the cameras
        assert cal(*sizes) - plain(*sizes) >= 72 * sizes[1]
    for sizes in ((0, 5, 5), (65, 5, 5), (3, -1, 5), (3, 5, -1), (3, 2**31, 5), (3, 5, 2**31)):
        assert plain(*sizes) == -1 and cal(*sizes) == -1, sizes


def test_entry_point_refuses_before_the_first_launch(native_lib):
    """Every refusal happens on the host with device pointers that are never dereferenced (null, or 0x1000 where a null
    pointer is itself the refusal under test)."""
    from structure_from_motion_amd import _native

    lib = native_lib
    p = C.c_void_p(0x1000)

    def call(refine=3, reserved=0, loss=(0, 0, 1.0), K=cases.RING_K, cameras=4, points=100, fixed=(1, 0, 0, 0), steps=10,
             ws_bytes=1 << 40, options=True, K_out=p, ws=p, dev=p):
        Kc = (C.c_double * 9)(*[float(v) for v in np.asarray(K).reshape(9)]) if K is not None else None
        fx = (C.c_uint8 * len(fixed))(*fixed) if fixed is not None else None
        opt = _native.BundleCalibrationOptions(_native.BundleOptions(*loss), refine, reserved)
        rc = lib.sfm_bundle_adjust_calibrated(C.cast(Kc, C.c_void_p), cameras, points, 400, C.cast(fx, C.c_void_p), dev, dev, dev,
                                              dev, dev, steps, dev, dev, dev, K_out, ws, ws_bytes, None,
                                              C.byref(opt) if options else None)
        return rc, lib.sfm_last_error()

    def refused(word, **kw):
        rc, message = call(**kw)
        assert rc == -1 and word in message, (kw, rc, message)

    for refine in (1, 2, 3):   # good options get as far as the workspace check (still before any launch)
        refused(b"workspace", refine=refine, ws_bytes=1000)
    for refine in (0, 4, -1, 7):
        refused(b"refine", refine=refine)
    refused(b"reserved", reserved=1)
    refused(b"options", options=False)
    for loss in ((3, 0, 1.0), (-1, 0, 1.0), (1, 1, 2.0), (1, 0, 0.0), (2, 0, float("nan")), (0, 0, float("inf"))):
        refused(b"loss", loss=loss)
    zero_focal = np.array([[0.0, 3.0, 320.0], [2.0, 810.0, 240.0], [0.0, 0.0, 1.0]])   # invertible block, K00 = 0
    refused(b"K[0,0]", K=zero_focal, refine=1)
    refused(b"K[0,0]", K=zero_focal, refine=3)
    refused(b"workspace", K=zero_focal, refine=2, ws_bytes=1000)
    # everything sfm_bundle_adjust_ex refuses
    refused(b"singular", K=np.array([[0.0, 0.0, 320.0], [0.0, 810.0, 240.0], [0.0, 0.0, 1.0]]))
    refused(b"row 2", K=np.array([[800.0, 0.0, 320.0], [0.0, 810.0, 240.0], [0.0, 0.0, 2.0]]))
    refused(b"null camera matrix", K=None)
    refused(b"bad size", cameras=0)
    refused(b"bad size", points=-1)
    refused(b"bad size", steps=-1)
    refused(b"64 cameras", cameras=65, fixed=(1,) + (0,) * 64)
    refused(b"2^31", points=2**31)
    refused(b"fixed", fixed=None)
    refused(b"at least one camera", fixed=(0, 0, 0, 0))
    refused(b"null pointer", dev=None)
    refused(b"null pointer", K_out=None)
    refused(b"null pointer", ws=None)
    refused(b"16-byte aligned", ws=C.c_void_p(0x1008))


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_registered_with_meta_kernels(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "bundle_adjust_calibrated" in ops.FUNCTIONAL_OPS and "bundle_adjust_calibrated_" in ops.INPLACE_OPS
    tail = "float[] K, int[] fixed, int max_steps, int loss, float loss_scale, int refine"
    schema = str(op.bundle_adjust_calibrated.default._schema)
    assert tail + ") -> (Tensor, Tensor, Tensor, Tensor)" in schema and "!" not in schema
    schema = str(op.bundle_adjust_calibrated_.default._schema)
    assert "Tensor(a!) poses, Tensor(b!) points" in schema and tail + ", Tensor(c!) info, Tensor(d!) K_out) -> ()" in schema
    meta = dict(device="meta")
    Cn, P, M = 20, 300, 1200

    def args(*tail):
        return (torch.empty((Cn, 12), dtype=torch.float64, **meta), torch.empty((P, 3), dtype=torch.float64, **meta),
                torch.empty((M,), dtype=torch.int32, **meta), torch.empty((M,), dtype=torch.int32, **meta),
                torch.empty((M, 2), dtype=torch.float64, **meta), [float(v) for v in cases.RING_K.reshape(9)], [0], 50) + tail

    poses, points, info, K_out = op.bundle_adjust_calibrated(*args(2, 2.0, 3))
    assert poses.shape == (Cn, 12) and points.shape == (P, 3) and poses.device.type == "meta"
    assert info.shape == (4,) and info.dtype == torch.int64 and K_out.shape == (3, 3) and K_out.dtype == torch.float64
    a = args()
    rec, Kt = torch.empty(4, dtype=torch.int64, **meta), torch.empty((3, 3), dtype=torch.float64, **meta)
    assert op.bundle_adjust_calibrated_(a[0], a[1], *a[2:], 0, 1.0, 1, rec, Kt) is None
    for refine in (0, 4, -1):
        with pytest.raises(RuntimeError, match="refine"):
            op.bundle_adjust_calibrated(*args(0, 1.0, refine))
    with pytest.raises(RuntimeError, match="loss"):
        op.bundle_adjust_calibrated(*args(3, 2.0, 1))
    with pytest.raises(RuntimeError, match="loss_scale"):
        op.bundle_adjust_calibrated(*args(1, 0.0, 1))


def test_no_existing_schema_changed(native_lib):
    """tests/golden/op_schemas_before_calibration.json: every op's schema as registered before this feature."""
    from structure_from_motion_amd import ops

    op = ops.load()
    with open(GOLDEN) as f:
        before = json.load(f)
    new = {"bundle_adjust_calibrated", "bundle_adjust_calibrated_"}
    assert set(before) == set(ops.FUNCTIONAL_OPS + ops.INPLACE_OPS) - new and len(before) >= 48
    for name, schema in before.items():
        assert str(getattr(op, name).default._schema) == schema, name


# ---------------------------------------------------------------------------------------------------------------------
# the public API and the app
# ---------------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def test_bundle_adjust_validates_refine_intrinsics_before_device_work(monkeypatch):
    from lib.bundle.bundle import bundle_adjust

    _no_device(monkeypatch)
    pr = cases.ring_problem(3, 20, per_point=3, seed=1)
    for bad in ("focal", b"focal", ("focus",), ("focal", "focal"), ("principal_point", "cx"), (1,), (None,), 3, None,
                ("focal", "principal_point", "skew")):
        with pytest.raises(ValueError, match="refine_intrinsics"):
            bundle_adjust(*_args(pr), refine_intrinsics=bad)
    for good in (("focal",), ["principal_point"], ("principal_point", "focal"), {"focal"}):
        with pytest.raises(ValueError, match="refine_intrinsics needs linear_solver"):
            bundle_adjust(*_args(pr), refine_intrinsics=good, linear_solver="iterative")
        with pytest.raises(AssertionError, match="device touched"):
            bundle_adjust(*_args(pr), refine_intrinsics=good)
    zero_focal = np.array([[0.0, 3.0, 320.0], [2.0, 810.0, 240.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="focal length"):
        bundle_adjust(zero_focal, *_args(pr)[1:], refine_intrinsics=("focal",))
    with pytest.raises(AssertionError, match="device touched"):
        bundle_adjust(zero_focal, *_args(pr)[1:], refine_intrinsics=("principal_point",))
    # the empty default is the call of before, for both solvers
    for solver in ("dense", "iterative"):
        with pytest.raises(AssertionError, match="device touched"):
            bundle_adjust(*_args(pr), linear_solver=solver, refine_intrinsics=())


def test_public_api_routes_a_calibrating_call(monkeypatch):
    """An empty ``refine_intrinsics`` is the device call of before and a ``BundleInfo``; a non-empty one goes to
    ``device.bundle_adjust_calibrated`` and comes back as a ``BundleCalibrationInfo``."""
    from structure_from_motion_amd import device
    from structure_from_motion_amd.bundle import bundle

    pr = cases.ring_problem(3, 20, per_point=3, seed=1)
    calls = []

    def plain(poses, points, *rest, **kw):
        calls.append(("plain", kw))
        return poses, points, torch.zeros(4, dtype=torch.int64)

    def calibrated(poses, points, *rest, **kw):
        calls.append(("calibrated", kw))
        return poses, points, torch.zeros(4, dtype=torch.int64), torch.arange(9, dtype=torch.float64).reshape(3, 3)

    monkeypatch.setattr(device, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(device, "to_device", lambda a, dtype=torch.float64: torch.as_tensor(np.asarray(a), dtype=dtype))
    monkeypatch.setattr(device, "bundle_adjust", plain)
    monkeypatch.setattr(device, "bundle_adjust_calibrated", calibrated)
    info = bundle.bundle_adjust(*_args(pr))[2]
    assert type(info) is device.BundleInfo
    info = bundle.bundle_adjust(*_args(pr), refine_intrinsics=[])[2]
    assert type(info) is device.BundleInfo
    out = bundle.bundle_adjust(*_args(pr), refine_intrinsics=("principal_point", "focal"), loss="huber", loss_scale=3)
    assert len(out) == 3 and type(out[2]) is device.BundleCalibrationInfo
    assert np.array_equal(out[2].camera_matrix, np.arange(9.0).reshape(3, 3)) and out[2].status == 0
    assert calls == [("plain", {}), ("plain", {}),
                     ("calibrated", dict(refine=["principal_point", "focal"], loss="huber", loss_scale=3.0))]
    assert [f for f in device.BundleCalibrationInfo.__dataclass_fields__][:5] == list(device.BundleInfo.__dataclass_fields__)


def test_device_layer_refuses_bad_refine_names_before_the_op(native_lib):
    from structure_from_motion_amd import device

    for bad in ("focal", ("focus",), ("focal", "focal"), ()):
        with pytest.raises(ValueError, match="refine|intrinsic"):
            device.bundle_adjust_calibrated(None, None, None, None, None, cases.RING_K, refine=bad)
    with pytest.raises(ValueError, match="loss"):
        device.bundle_adjust_calibrated(None, None, None, None, None, cases.RING_K, loss="tukey")


def test_multi_view_app_refuses_a_bad_bundle_refine_before_any_work(monkeypatch, capsys):
    from apps import sfm_multi_view
    from structure_from_motion_amd import synthetic

    def no_work(*args, **kwargs):
        raise AssertionError("work started")

    monkeypatch.setattr(synthetic, "multi_view_scene", no_work)
    for bad in (("focus",), "focal", ("focal", "focal")):
        with pytest.raises(ValueError, match="refine_intrinsics"):
            sfm_multi_view.run(bundle_refine=bad)
    with pytest.raises(ValueError, match="bundle_refine needs the dense solver"):
        sfm_multi_view.run(views=65, bundle_solver="auto", bundle_refine=("focal",))
    with pytest.raises(ValueError, match="focal_error"):
        sfm_multi_view.run(focal_error=-1.0)
    for argv in (["--bundle-refine", "focus"], ["--bundle-refine", "focal,focal"], ["--bundle-refine", "focal,skew"],
                 ["--bundle-refine", "focal", "--views", "65"], ["--focal-error", "nan"]):
        monkeypatch.setattr(sys, "argv", ["sfm_multi_view.py"] + argv)
        with pytest.raises(SystemExit) as stop:
            sfm_multi_view.main()
        assert stop.value.code == 2
        assert "--bundle-refine" in capsys.readouterr().err or argv[0] == "--focal-error"
    monkeypatch.setattr(sys, "argv", ["sfm_multi_view.py", "--bundle-refine", "focal,principal_point", "--focal-error", "0.05"])
    with pytest.raises(AssertionError, match="work started"):   # good flags reach the pipeline
        sfm_multi_view.main()
