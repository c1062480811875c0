"""Rotation averaging without a GPU: what is exported and bound, every refusal before the first launch, the Meta
kernel, the argument checks of the public functions, the edges a ``ViewGraph`` contributes, and the properties of the NumPy
definition (tests/rotation_averaging_oracle.py) that tests/test_gpu_rotation_averaging.py rests on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rotation_averaging_oracle as ro

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_DEG = np.radians(1.0)
ORACLE_SPREAD = 3.55e-16   # the figure tests/test_gpu_rotation_averaging.py takes its tolerance from


# ---- exports -------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_structs(native_lib):
    from structure_from_motion_amd import _native, build, device

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    assert "sfm_rotation_averaging.hip" in build.SOURCES
    assert "sfm_average_rotations" in _native.SIGNATURES and "sfm_average_rotations_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(native_lib, "sfm_average_rotations") and hasattr(native_lib, "sfm_average_rotations_workspace_bytes")
    assert C.sizeof(_native.RotavgOptions) == 40 and C.sizeof(_native.RotavgInfo) == 40
    header = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    assert "#define SFM_ABI_VERSION 15" in header
    for code, name in enumerate(("CONVERGED", "MAX_STEPS", "CG_FAILED", "BAD_INDEX")):
        assert f"#define SFM_ROTAVG_{name} {code}" in header
        assert getattr(device, f"ROTAVG_{name}") == code and device.ROTAVG_STATUS[code] == name.lower() == ro.STATUS[code]
    assert "#define SFM_ROTAVG_INIT_TREE 0" in header and "#define SFM_ROTAVG_INIT_GIVEN 1" in header
    assert (_native.ROTAVG_INIT_TREE, _native.ROTAVG_INIT_GIVEN) == (0, 1)
    for text in ("typedef struct sfm_rotavg_options", "typedef struct sfm_rotavg_info", "int sfm_average_rotations(",
                 "int64_t sfm_average_rotations_workspace_bytes(int64_t cameras, int64_t edges);",
                 "added under ABI 15 without a version change"):
        assert text in header, text
    assert tuple(_native.BUNDLE_LOSSES) == ro.LOSSES


def test_workspace_bytes_monotone_and_refused(native_lib):
    ws = native_lib.sfm_average_rotations_workspace_bytes
    sizes = [(1, 0), (2, 1), (300, 299), (1000, 20000), (100000, 2000000), ((1 << 31) - 1, (1 << 30) - 1)]
    values = [ws(c, q) for c, q in sizes]
    assert all(v > 0 for v in values) and values == sorted(values)
    for c in (1, 7, 1000):
        for q in (0, 5, 4000):
            assert ws(c + 1, q) >= ws(c, q) and ws(c, q + 1) >= ws(c, q)
    assert ws(100000, 2000000) >= 2000000 * (8 + 4 * 8) + 100000 * 22 * 8   # ord, omega, r; the CG vectors
    for c, q in ((0, 0), (-1, 5), (1 << 31, 5), (5, -1), (5, 1 << 30)):
        assert ws(c, q) == -1, (c, q)


def test_every_refusal_before_the_first_launch(native_lib):
    """No GPU needed: device pointers are never dereferenced."""
    from structure_from_motion_amd import _native

    lib = native_lib
    p = C.c_void_p(0x1000)
    defaults = dict(loss=0, init=0, max_steps=10, max_cg_iterations=50, loss_scale=0.01, cg_tolerance=1e-6, step_tolerance=1e-8)

    def call(cams=6, edges=9, pairs=p, rel=p, w=p, root=0, initial=None, opts=True, R=p, reg=p, level=p, res=p, info=p, ws=p,
             ws_bytes=1 << 40, **o):
        options = _native.RotavgOptions(**{**defaults, **o})
        return lib.sfm_average_rotations(cams, edges, pairs, rel, w, root, initial, C.byref(options) if opts else None, R, reg,
                                         level, res, info, ws, ws_bytes, None)

    err = lib.sfm_last_error
    for kw in (dict(cams=0), dict(cams=1 << 31), dict(edges=-1), dict(edges=1 << 30)):
        assert call(**kw) == -1 and b"cameras" in err(), kw
    for root in (-1, 6, 1 << 40):
        assert call(root=root) == -1 and b"root" in err()
    assert call(opts=False) == -1 and b"options" in err()
    for loss in (-1, 3):
        assert call(loss=loss) == -1 and b"loss" in err()
    for init in (-1, 2):
        assert call(init=init) == -1 and b"init" in err()
    assert call(max_steps=-1) == -1 and b"max_steps" in err()
    assert call(max_cg_iterations=0) == -1 and b"max_cg_iterations" in err()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert call(loss_scale=v) == -1 and b"loss_scale" in err(), v
        assert call(step_tolerance=v) == -1 and b"step_tolerance" in err(), v
    for v in (0.0, -0.1, 1.0, float("nan"), float("inf")):
        assert call(cg_tolerance=v) == -1 and b"cg_tolerance" in err(), v
    for name in ("pairs", "rel", "w", "R", "reg", "res", "info", "ws"):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    assert call(init=1, initial=None) == -1 and b"null" in err()
    assert call(ws_bytes=1000) == -1 and b"workspace too small" in err()
    assert call(ws=C.c_void_p(0x1008)) == -1 and b"aligned" in err()
    need = lib.sfm_average_rotations_workspace_bytes(6, 9)
    assert call(ws_bytes=need - 1) == -1 and b"workspace too small" in err()


def test_op_schema_and_meta_kernel(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "average_rotations" in ops.FUNCTIONAL_OPS
    schema = str(op.average_rotations.default._schema)
    assert schema.startswith("sfm_hip::average_rotations(Tensor pairs, Tensor relative, Tensor weights, int cameras, int root, "
                             "Tensor? initial, int loss, float loss_scale, int max_steps, int max_cg_iterations, "
                             "float cg_tolerance, float step_tolerance)")
    Cn, Q = 40, 130

    def args(pair_cols=2, rel_shape=(Q, 3, 3), cameras=Cn, root=0, initial=None, loss=1, scale=0.02, steps=50, cg_it=500,
             cg_tol=1e-6, step_tol=1e-8):
        meta = dict(device="meta")
        return (torch.empty((Q, pair_cols), dtype=torch.int32, **meta), torch.empty(rel_shape, dtype=torch.float64, **meta),
                torch.empty((Q,), dtype=torch.float64, **meta), cameras, root, initial, loss, scale, steps, cg_it, cg_tol, step_tol)

    R, reg, level, res, info = op.average_rotations(*args())
    assert R.shape == (Cn, 3, 3) and R.dtype == torch.float64 and R.device.type == "meta"
    assert reg.shape == (Cn,) and reg.dtype == torch.uint8 and level.shape == (Cn,) and level.dtype == torch.int32
    assert res.shape == (Q,) and res.dtype == torch.float64 and info.shape == (5,) and info.dtype == torch.int64
    assert op.average_rotations(*args(rel_shape=(Q, 9), initial=torch.empty((Cn, 9), dtype=torch.float64, device="meta")))[0].shape == (Cn, 3, 3)
    for kw, match in ((dict(pair_cols=3), "pairs"), (dict(rel_shape=(Q, 3, 4)), "relative"), (dict(cameras=0), "cameras"),
                      (dict(root=Cn), "root"), (dict(loss=3), "loss"), (dict(scale=0.0), "loss_scale"), (dict(steps=-1), "max_steps"),
                      (dict(cg_it=0), "max_cg_iterations"), (dict(cg_tol=1.0), "cg_tolerance"), (dict(step_tol=0.0), "step_tolerance"),
                      (dict(initial=torch.empty((Cn + 1, 3, 3), dtype=torch.float64, device="meta")), "initial")):
        with pytest.raises(RuntimeError, match=match):
            op.average_rotations(*args(**kw))


def test_lib_reexport():
    import lib.multiview.rotation_averaging as shim
    from structure_from_motion_amd.multiview import rotation_averaging as ra

    for name in ("GlobalRotations", "average_rotations", "average_graph_rotations", "inconsistent_pairs"):
        assert getattr(shim, name) is getattr(ra, name)
    fields = [f for f in ra.GlobalRotations.__dataclass_fields__]
    for name in ("R", "registered", "residual_deg", "steps", "cg_iterations", "initial_cost", "final_cost", "status"):
        assert name in fields
    assert "Cauchy" in ra.__doc__ or "cauchy" in ra.average_rotations.__doc__


# ---- the argument checks of the public functions ------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)
    monkeypatch.setattr(device, "average_rotations", no_device)


def test_every_value_error_before_any_device_work(monkeypatch):
    from lib.multiview.rotation_averaging import average_rotations

    _no_device(monkeypatch)
    rng = np.random.default_rng(1)
    pairs = np.array([[0, 1], [1, 2], [2, 0]])
    rel = np.array([ro.random_rotation(rng) for _ in range(3)])

    def bad(match, num=3, pairs=pairs, rel=rel, **kw):
        with pytest.raises(ValueError, match=match):
            average_rotations(num, pairs, rel, **kw)

    for num in (0, -1, 2.5, True, 2**31):
        bad("num_cameras", num=num)
    bad("pairs", pairs=np.array([[0, 1, 2]]))
    bad("pairs", pairs=np.array([[0.0, 1.0], [1.0, 2.0], [2.0, 0.0]]))
    bad("pairs", pairs=np.array([0, 1, 2]))
    bad(r"camera indices in \[0, 3\)", pairs=np.array([[0, 1], [1, 3], [2, 0]]))
    bad("camera indices", pairs=np.array([[0, 1], [-1, 2], [2, 0]]))
    bad("itself", pairs=np.array([[0, 1], [1, 1], [2, 0]]))
    bad("relative_rotations", rel=rel[:2])
    bad("relative_rotations", rel=rel.reshape(3, 9))
    bad("relative_rotations", rel="abc")
    bad("weights", weights=np.ones(2))
    bad("weights", weights=np.ones((3, 1)))
    for root in (-1, 3, 1.0):
        bad("root", root=root)
    bad("loss", loss="tukey")
    for v in (0.0, -1.0, np.nan, np.inf, "x"):
        bad("loss_scale_deg", loss_scale_deg=v)
        bad("step_tolerance", step_tolerance=v)
    for v in (0.0, 1.0, -0.5, np.nan):
        bad("cg_tolerance", cg_tolerance=v)
    bad("initial_rotations", initial_rotations=np.zeros((2, 3, 3)))
    bad("max_steps", max_steps=-1)
    bad("max_steps", max_steps=1.5)
    bad("max_cg_iterations", max_cg_iterations=0)
    # an active edge's matrix must be a rotation; an inactive edge's is not looked at
    scaled, mirrored = rel.copy(), rel.copy()
    scaled[1] *= 1.0 + 1e-5
    mirrored[2] = mirrored[2] @ np.diag([1.0, 1.0, -1.0])
    bad(r"relative_rotations\[1\] is not a rotation", rel=scaled)
    bad(r"relative_rotations\[2\] is not a rotation", rel=mirrored)
    with pytest.raises(AssertionError, match="device touched"):   # past every check
        average_rotations(3, pairs, scaled, weights=np.array([1.0, 0.0, 1.0]))
    with pytest.raises(AssertionError, match="device touched"):
        average_rotations(3, pairs, rel * (1.0 + 1e-8))


def test_no_edges_needs_no_gpu(monkeypatch):
    from lib.multiview.rotation_averaging import average_rotations, inconsistent_pairs

    _no_device(monkeypatch)
    r = average_rotations(4, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3, 3)), root=2)
    assert r.status == "converged" and r.steps == 0 and r.registered.tolist() == [False, False, True, False]
    assert np.array_equal(r.R[2], np.eye(3)) and np.isnan(r.R[[0, 1, 3]]).all() and r.level.tolist() == [-1, -1, 0, -1]
    assert r.residual_deg.shape == (0,) and inconsistent_pairs(r, 5.0).tolist() == []
    r = average_rotations(1, [], [])
    assert r.registered.tolist() == [True] and r.initial_cost == r.final_cost == 0.0
    want = ro.average_rotations(4, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3, 3)), root=2)
    assert want["status"] == ro.CONVERGED and want["steps"] == 0 and np.array_equal(want["registered"], [False, False, True, False])


def test_inconsistent_pairs():
    from lib.multiview.rotation_averaging import GlobalRotations, inconsistent_pairs

    r = GlobalRotations(np.zeros((2, 3, 3)), np.ones(2, bool), np.zeros(2), np.array([0.1, 7.0, np.nan, 5.0, 5.1]), 1, 1, 0.0, 0.0,
                        "converged")
    assert inconsistent_pairs(r, 5.0).tolist() == [1, 4] and inconsistent_pairs(r, 0.05).tolist() == [0, 1, 3, 4]
    for v in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="max_residual_deg"):
            inconsistent_pairs(r, v)


def test_graph_edges_and_weights(monkeypatch):
    """``average_graph_rotations`` on a hand-made ViewGraph: the pairs, rotations, weights and root it hands on."""
    from lib.epipolar.view_graph import PairPoses, ViewGraph
    from structure_from_motion_amd.multiview import rotation_averaging as ra

    rng = np.random.default_rng(2)
    Q = 6
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 2], [1, 3]])
    R = np.array([ro.random_rotation(rng) for _ in range(Q)])
    R[2] = np.nan
    kind = ["essential", "homography", "essential", "essential", "essential", "none"]
    status = ["ok", "ok", "no_vote", "ok", "ok", "no_model"]
    in_front = np.array([40, 90, 0, 75, 75, 0])
    pose = PairPoses(R, np.zeros((Q, 3)), np.zeros((Q, 4), np.int64), in_front, np.zeros(Q), status)
    none = np.full((Q, 3, 3), np.nan)
    graph = ViewGraph(pairs, kind, none, none, np.zeros(Q, np.int64), np.zeros(Q, np.int64), np.zeros(Q), [], [], [], pose)
    idx, p, r, w = ra.graph_edges(graph)
    assert idx.tolist() == [0, 3, 4] and p.tolist() == [[0, 1], [3, 0], [4, 2]] and w.tolist() == [40.0, 75.0, 75.0]
    assert np.array_equal(r, R[[0, 3, 4]])
    assert ra.graph_edges(graph, kinds=("essential", "homography"))[0].tolist() == [0, 1, 3, 4]
    seen = {}

    def fake(num_cameras, pairs, relative_rotations, weights=None, root=0, **options):
        seen.update(num=num_cameras, pairs=pairs, rel=relative_rotations, w=weights, root=root, options=options)
        return ra.GlobalRotations(np.zeros((num_cameras, 3, 3)), np.ones(num_cameras, bool), np.zeros(num_cameras),
                                  np.array([1.0, 2.0, 3.0]), 1, 1, 0.0, 0.0, "converged")

    monkeypatch.setattr(ra, "average_rotations", fake)
    out = ra.average_graph_rotations(graph, 5, loss="huber", max_steps=7)
    assert seen["num"] == 5 and seen["pairs"].tolist() == [[0, 1], [3, 0], [4, 2]]
    assert seen["w"].tolist() == [40.0, 75.0, 75.0] and seen["options"] == dict(loss="huber", max_steps=7)
    assert seen["root"] == 0   # the lower image of the heaviest used pair, the first of equals: (3, 0)
    assert np.array_equal(out.residual_deg, [1.0, np.nan, np.nan, 2.0, 3.0, np.nan], equal_nan=True)
    ra.average_graph_rotations(graph, 5, root=4)
    assert seen["root"] == 4
    with pytest.raises(ValueError, match="graph.pose"):
        ra.average_graph_rotations(graph._replace(pose=None), 5)
    assert "lower image of the heaviest used pair" in ra.average_graph_rotations.__doc__


# ---- the properties of the definition that the GPU tests rest on ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def losses():
    case = ro.case_losses()
    kw = dict(num_cameras=24, pairs=case["pairs"], relative_rotations=case["relative"], loss_scale=ONE_DEG)
    squared = ro.average_rotations(**kw)
    huber = ro.average_rotations(**kw, loss="huber", max_steps=100, step_tolerance=1e-10)
    cauchy = ro.average_rotations(**kw, loss="cauchy", initial_rotations=huber["R"], max_steps=100, step_tolerance=1e-10)
    clean = ~case["outlier"]
    alone = ro.average_rotations(24, case["pairs"][clean], case["relative"][clean])
    return case, kw, squared, huber, cauchy, alone


def test_oracle_losses_on_the_outlier_graph(losses):
    case, kw, squared, huber, cauchy, alone = losses
    assert case["outlier"].sum() == 21 and len(case["pairs"]) == 104   # 20 %
    err = {name: ro.max_error_deg(r["R"], case["R_true"]) for name, r in
           (("squared", squared), ("huber", huber), ("cauchy", cauchy), ("alone", alone))}
    print(err, "huber steps", huber["steps"], "cauchy steps", cauchy["steps"])
    assert err["squared"] > 20.0                                    # measured 45.4
    assert err["huber"] < 3.0 and huber["steps"] <= 100             # measured 0.88 after 28 steps
    assert err["cauchy"] <= 2.0 * err["alone"]                      # measured 0.61 against 0.69
    assert set(np.nonzero(np.degrees(cauchy["residual"]) > 5.0)[0]) == set(np.nonzero(case["outlier"])[0])
    # with margin: the smallest planted residual is 50.9 degrees, the largest other 1.65
    assert np.degrees(cauchy["residual"][case["outlier"]].min()) > 10.0 and np.degrees(cauchy["residual"][~case["outlier"]].max()) < 2.5
    # cauchy from the tree stays far from the answer: why initial_rotations is part of the interface
    tree = ro.average_rotations(**kw, loss="cauchy", max_steps=100)
    print("cauchy from the tree", ro.max_error_deg(tree["R"], case["R_true"]))
    assert ro.max_error_deg(tree["R"], case["R_true"]) > 10.0 * err["cauchy"]


def test_oracle_dense_and_pcg_agree(losses):
    """The spread the GPU tests' tolerance is 1 000 times of: dense against PCG with reversed adjacency order."""
    case, kw, squared, huber, cauchy, alone = losses
    tight = dict(step_tolerance=1e-12)
    dense = ro.average_rotations(**kw, solver="dense", **tight)
    pcg = ro.average_rotations(**kw, solver="pcg", reverse_adjacency=True, **tight)
    spread = ro.max_rotation_difference(dense["R"], pcg["R"])
    print("squared", spread, dense["steps"], pcg["steps"])
    assert dense["status"] == pcg["status"] == ro.CONVERGED and dense["steps"] == pcg["steps"]
    # measured 3.55e-16 (three ulps of a rotation entry); ten times that leaves room for another LAPACK behind the dense solve
    # and is still a hundredth of the GPU tests' tolerance
    assert spread <= 10 * ORACLE_SPREAD and np.allclose(dense["residual"], pcg["residual"], rtol=0, atol=1e-14)
    fixed = dict(loss="huber", max_steps=60, step_tolerance=1e-300, cg_tolerance=1e-10)
    dense = ro.average_rotations(**kw, solver="dense", **fixed)
    pcg = ro.average_rotations(**kw, solver="pcg", reverse_adjacency=True, **fixed)
    spread = ro.max_rotation_difference(dense["R"], pcg["R"])
    print("huber", spread)
    assert dense["status"] == pcg["status"] == ro.MAX_STEPS and spread <= 10 * ORACLE_SPREAD   # measured 7.98e-17


def test_oracle_small_properties():
    rng = np.random.default_rng(3)
    # the logarithm inverts the exponential, also next to 0 and next to pi; the half turn about x exactly
    for angle in (0.0, 1e-12, 1e-7, 0.3, 3.0, np.pi - 1e-12, np.pi):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        back = ro.log_map(ro.exp_map(axis * angle))
        assert abs(np.linalg.norm(back) - angle) <= 1e-9 and np.linalg.norm(np.cross(back, axis)) <= 1e-6 * max(angle, 1e-12), angle
    assert np.allclose(ro.log_map(np.diag([1.0, -1.0, -1.0])), [np.pi, 0.0, 0.0], rtol=0, atol=0)
    assert np.allclose(np.abs(ro.log_map(np.diag([-1.0, -1.0, 1.0]))), [0.0, 0.0, np.pi], rtol=0, atol=0)
    # bad indices and a self-pair
    R = np.array([np.eye(3)] * 2)
    for pairs in ([[0, 2], [0, 1]], [[-1, 0], [0, 1]], [[1, 1], [0, 1]]):
        r = ro.average_rotations(2, np.array(pairs), R)
        assert r["status"] == ro.BAD_INDEX and np.isnan(r["R"]).all() and np.isnan(r["residual"]).all() and not r["registered"].any()
    # one edge either way round: the other camera's rotation is the edge's (or its transpose), bit for bit
    Rq = ro.random_rotation(rng)
    assert np.array_equal(ro.average_rotations(2, np.array([[0, 1]]), Rq[None])["R"][1], Rq)
    assert np.array_equal(ro.average_rotations(2, np.array([[1, 0]]), Rq[None])["R"][1], Rq.T)
    # the robust weights and losses are those of csrc/sfm_loss.h
    a = 0.02
    for e in (0.0, a * a, 4 * a * a, 1.0):
        assert ro.weight("squared", a, e) == 1.0 and ro.rho("squared", a, e) == e
        assert ro.weight("huber", a, e) == (1.0 if e <= a * a else a / np.sqrt(e))
        assert ro.weight("cauchy", a, e) == 1.0 / (1.0 + e / (a * a))
    assert ro.rho("huber", a, 4 * a * a) == pytest.approx(3 * a * a) and ro.rho("cauchy", a, a * a) == pytest.approx(a * a * np.log(2))
