"""Translation averaging without a GPU: what is exported and bound, every refusal before the first launch, the
Meta kernel, the argument checks of the public functions, the edges a ``ViewGraph`` contributes, ``global_poses``, and the
properties of the NumPy definition (tests/translation_averaging_oracle.py) that tests/test_gpu_translation_averaging.py rests
on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import translation_averaging_oracle as to

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SPREAD = 1.52e-12   # the figure tests/test_gpu_translation_averaging.py takes its tolerance from


# ---- exports -------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_structs(native_lib):
    from structure_from_motion_amd import _native, build, device

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    assert "sfm_translation_averaging.hip" in build.SOURCES and "sfm_graph_cg.h" in build.HEADERS
    assert "sfm_average_translations" in _native.SIGNATURES
    assert "sfm_average_translations_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(native_lib, "sfm_average_translations") and hasattr(native_lib, "sfm_average_translations_workspace_bytes")
    assert len(_native.SIGNATURES["sfm_average_translations"]) == 18
    assert C.sizeof(_native.TransavgOptions) == 48 and C.sizeof(_native.TransavgInfo) == 40
    header = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    assert "#define SFM_ABI_VERSION 15" in header
    for code, name in enumerate(("CONVERGED", "MAX_STEPS", "CG_FAILED", "BAD_INDEX")):
        assert f"#define SFM_TRANSAVG_{name} {code}" in header
        assert getattr(device, f"TRANSAVG_{name}") == code and device.TRANSAVG_STATUS[code] == name.lower() == to.STATUS[code]
    assert "#define SFM_TRANSAVG_INIT_TREE 0" in header and "#define SFM_TRANSAVG_INIT_GIVEN 1" in header
    assert (_native.TRANSAVG_INIT_TREE, _native.TRANSAVG_INIT_GIVEN) == (0, 1)
    for text in ("typedef struct sfm_transavg_options", "typedef struct sfm_transavg_info", "int sfm_average_translations(",
                 "int64_t sfm_average_translations_workspace_bytes(int64_t cameras, int64_t edges);", "int32_t warmup_steps;"):
        assert text in header, text
    assert header.count("added under ABI 15 without a version change") >= 2
    # the shared kernels are defined once: the rotation file no longer carries its own
    rot = open(os.path.join(REPO, "structure_from_motion_amd", "csrc", "sfm_rotation_averaging.hip")).read()
    tra = open(os.path.join(REPO, "structure_from_motion_amd", "csrc", "sfm_translation_averaging.hip")).read()
    for source in (rot, tra):
        assert '#include "sfm_graph_cg.h"' in source and "graphcg::run<" in source
        assert "void cg_apply_kernel" not in source and "void rotavg_cg_apply_kernel" not in source


def test_workspace_bytes_monotone_and_refused(native_lib):
    ws, rot = native_lib.sfm_average_translations_workspace_bytes, native_lib.sfm_average_rotations_workspace_bytes
    sizes = [(1, 0), (2, 1), (300, 299), (1000, 20000), (100000, 2000000), ((1 << 31) - 1, (1 << 30) - 1)]
    values = [ws(c, q) for c, q in sizes]
    assert all(v > 0 for v in values) and values == sorted(values)
    for c in (1, 7, 1000):
        for q in (0, 5, 4000):
            assert ws(c + 1, q) >= ws(c, q) and ws(c, q + 1) >= ws(c, q)
            assert ws(c, q) >= rot(c, q) + 3 * 8 * q   # the shared workspace and the world directions
    for c, q in ((0, 0), (-1, 5), (1 << 31, 5), (5, -1), (5, 1 << 30)):
        assert ws(c, q) == -1, (c, q)


def test_every_refusal_before_the_first_launch(native_lib):
    """No GPU needed: device pointers are never dereferenced."""
    from structure_from_motion_amd import _native

    lib = native_lib
    p = C.c_void_p(0x1000)
    defaults = dict(loss=0, init=0, max_steps=10, max_cg_iterations=50, warmup_steps=3, reserved=0, loss_scale=0.03,
                    cg_tolerance=1e-6, step_tolerance=1e-8)

    def call(cams=6, edges=9, pairs=p, dirs=p, rot=None, w=p, root=0, initial=None, opts=True, pos=p, reg=p, level=p, res=p,
             scale=p, info=p, ws=p, ws_bytes=1 << 40, **o):
        options = _native.TransavgOptions(**{**defaults, **o})
        return lib.sfm_average_translations(cams, edges, pairs, dirs, rot, w, root, initial, C.byref(options) if opts else None,
                                            pos, reg, level, res, scale, info, ws, ws_bytes, None)

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
    assert call(warmup_steps=-1) == -1 and b"warmup_steps" in err()
    assert call(reserved=1) == -1 and b"reserved" in err()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert call(loss_scale=v) == -1 and b"loss_scale" in err(), v
        assert call(step_tolerance=v) == -1 and b"step_tolerance" in err(), v
    for v in (0.0, -0.1, 1.0, float("nan"), float("inf")):
        assert call(cg_tolerance=v) == -1 and b"cg_tolerance" in err(), v
    for name in ("pairs", "dirs", "w", "pos", "reg", "res", "scale", "info", "ws"):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    assert call(init=1, initial=None) == -1 and b"null" in err()
    assert call(ws_bytes=1000) == -1 and b"workspace too small" in err()
    assert call(ws=C.c_void_p(0x1008)) == -1 and b"aligned" in err()
    need = lib.sfm_average_translations_workspace_bytes(6, 9)
    assert call(ws_bytes=need - 1) == -1 and b"workspace too small" in err()


def test_op_schema_and_meta_kernel(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "average_translations" in ops.FUNCTIONAL_OPS
    schema = str(op.average_translations.default._schema)
    assert schema.startswith("sfm_hip::average_translations(Tensor pairs, Tensor directions, Tensor? rotations, Tensor weights, "
                             "int cameras, int root, Tensor? initial, int loss, float loss_scale, int warmup_steps, "
                             "int max_steps, int max_cg_iterations, float cg_tolerance, float step_tolerance)")
    Cn, Q = 40, 130
    meta = dict(device="meta")

    def args(pair_cols=2, dir_shape=(Q, 3), rotations=None, cameras=Cn, root=0, initial=None, loss=1, scale=0.03, warm=10,
             steps=50, cg_it=500, cg_tol=1e-6, step_tol=1e-8):
        return (torch.empty((Q, pair_cols), dtype=torch.int32, **meta), torch.empty(dir_shape, dtype=torch.float64, **meta),
                rotations, torch.empty((Q,), dtype=torch.float64, **meta), cameras, root, initial, loss, scale, warm, steps, cg_it,
                cg_tol, step_tol)

    c, reg, level, res, scale, info = op.average_translations(*args())
    assert c.shape == (Cn, 3) and c.dtype == torch.float64 and c.device.type == "meta"
    assert reg.shape == (Cn,) and reg.dtype == torch.uint8 and level.shape == (Cn,) and level.dtype == torch.int32
    assert res.shape == (Q,) and res.dtype == torch.float64 and scale.shape == (Q,) and scale.dtype == torch.float64
    assert info.shape == (5,) and info.dtype == torch.int64
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, **meta)   # noqa: E731
    assert op.average_translations(*args(rotations=f64(Cn, 9), initial=f64(Cn, 3)))[0].shape == (Cn, 3)
    assert op.average_translations(*args(rotations=f64(Cn, 3, 3)))[0].shape == (Cn, 3)
    for kw, match in ((dict(pair_cols=3), "pairs"), (dict(dir_shape=(Q, 4)), "directions"), (dict(cameras=0), "cameras"),
                      (dict(root=Cn), "root"), (dict(loss=3), "loss"), (dict(scale=0.0), "loss_scale"), (dict(steps=-1), "max_steps"),
                      (dict(warm=-1), "warmup_steps"), (dict(cg_it=0), "max_cg_iterations"), (dict(cg_tol=1.0), "cg_tolerance"),
                      (dict(step_tol=0.0), "step_tolerance"), (dict(initial=f64(Cn + 1, 3)), "initial"),
                      (dict(rotations=f64(Cn, 3, 4)), "rotations")):
        with pytest.raises(RuntimeError, match=match):
            op.average_translations(*args(**kw))


def test_lib_reexport():
    import lib.multiview.translation_averaging as shim
    from structure_from_motion_amd.multiview import rotation_averaging as ra
    from structure_from_motion_amd.multiview import translation_averaging as ta

    for name in ("GlobalPositions", "average_translations", "average_graph_translations", "global_poses", "inconsistent_pairs"):
        assert getattr(shim, name) is getattr(ta, name)
    assert ta.inconsistent_pairs is ra.inconsistent_pairs   # reused, not copied
    fields = [f for f in ta.GlobalPositions.__dataclass_fields__]
    assert fields == ["c", "registered", "level", "residual_deg", "scale", "steps", "cg_iterations", "initial_cost", "final_cost",
                      "status"]
    assert "initial_positions" in ta.average_translations.__doc__ and "Huber first" in ta.__doc__


# ---- the argument checks of the public functions ------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)
    monkeypatch.setattr(device, "average_translations", no_device)


def test_every_value_error_before_any_device_work(monkeypatch):
    from lib.multiview.translation_averaging import average_translations

    _no_device(monkeypatch)
    pairs = np.array([[0, 1], [1, 2], [2, 0]])
    v = to.unit(np.random.default_rng(1).normal(size=(3, 3)))

    def bad(match, num=3, pairs=pairs, v=v, **kw):
        with pytest.raises(ValueError, match=match):
            average_translations(num, pairs, v, **kw)

    for num in (0, -1, 2.5, True, 2**31):
        bad("num_cameras", num=num)
    bad("pairs", pairs=np.array([[0, 1, 2]]))
    bad("pairs", pairs=np.array([[0.0, 1.0], [1.0, 2.0], [2.0, 0.0]]))
    bad("pairs", pairs=np.array([0, 1, 2]))
    bad(r"camera indices in \[0, 3\)", pairs=np.array([[0, 1], [1, 3], [2, 0]]))
    bad("camera indices", pairs=np.array([[0, 1], [-1, 2], [2, 0]]))
    bad("itself", pairs=np.array([[0, 1], [1, 1], [2, 0]]))
    bad("directions", v=v[:2])
    bad("directions", v=v.reshape(9))
    bad("directions", v="abc")
    bad("weights", weights=np.ones(2))
    bad("weights", weights=np.ones((3, 1)))
    for root in (-1, 3, 1.0):
        bad("root", root=root)
    bad("loss", loss="tukey")
    for x in (0.0, -1.0, np.nan, np.inf, "x", 90.0):
        bad("loss_scale_deg", loss_scale_deg=x)
    for x in (0.0, -1.0, np.nan, np.inf, "x"):
        bad("step_tolerance", step_tolerance=x)
    for x in (0.0, 1.0, -0.5, np.nan):
        bad("cg_tolerance", cg_tolerance=x)
    bad("initial_positions", initial_positions=np.zeros((2, 3)))
    bad("initial_positions must be finite", initial_positions=np.full((3, 3), np.nan))
    bad("max_steps", max_steps=-1)
    bad("max_steps", max_steps=1.5)
    bad("warmup_steps", warmup_steps=-1)
    bad("max_cg_iterations", max_cg_iterations=0)
    # an active edge's direction must be unit to 1e-6; an inactive edge's is not looked at
    scaled = v.copy()
    scaled[1] *= 1.0 + 1e-5
    bad(r"directions\[1\] is not a unit vector", v=scaled)
    with pytest.raises(AssertionError, match="device touched"):   # past every check
        average_translations(3, pairs, scaled, weights=np.array([1.0, 0.0, 1.0]))
    with pytest.raises(AssertionError, match="device touched"):
        average_translations(3, pairs, v * (1.0 + 1e-8))


def test_no_edges_needs_no_gpu(monkeypatch):
    from lib.multiview.translation_averaging import average_translations, inconsistent_pairs

    _no_device(monkeypatch)
    r = average_translations(4, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3)), root=2)
    assert r.status == "converged" and r.steps == 0 and r.registered.tolist() == [False, False, True, False]
    assert np.array_equal(r.c[2], np.zeros(3)) and np.isnan(r.c[[0, 1, 3]]).all() and r.level.tolist() == [-1, -1, 0, -1]
    assert r.residual_deg.shape == (0,) and r.scale.shape == (0,) and inconsistent_pairs(r, 5.0).tolist() == []
    r = average_translations(1, [], [], initial_positions=np.array([[1.0, 2.0, 3.0]]))
    assert r.registered.tolist() == [True] and r.initial_cost == r.final_cost == 0.0 and r.c.tolist() == [[1.0, 2.0, 3.0]]
    want = to.average_translations(4, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 3)), root=2)
    assert want["status"] == to.CONVERGED and want["steps"] == 0 and np.array_equal(want["registered"], [False, False, True, False])
    assert np.array_equal(want["c"][2], np.zeros(3))


def _hand_made_graph():
    from lib.epipolar.view_graph import PairPoses, ViewGraph

    rng = np.random.default_rng(2)
    Q = 6
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 2], [1, 3]])
    t = to.unit(rng.normal(size=(Q, 3)))
    kind = ["essential", "homography", "essential", "essential", "essential", "none"]
    status = ["ok", "ok", "no_vote", "ok", "ok", "no_model"]
    in_front = np.array([40, 90, 0, 75, 75, 0])
    pose = PairPoses(np.full((Q, 3, 3), np.nan), t, np.zeros((Q, 4), np.int64), in_front, np.zeros(Q), status)
    none = np.full((Q, 3, 3), np.nan)
    return ViewGraph(pairs, kind, none, none, np.zeros(Q, np.int64), np.zeros(Q, np.int64), np.zeros(Q), [], [], [], pose), t


def test_graph_edges_weights_and_root(monkeypatch):
    """``average_graph_translations`` on a hand-made ViewGraph: the pairs, t, rotations, weights and root it hands on."""
    from rotation_averaging_oracle import random_rotation
    from structure_from_motion_amd.multiview import rotation_averaging as ra
    from structure_from_motion_amd.multiview import translation_averaging as ta

    graph, t = _hand_made_graph()
    rng = np.random.default_rng(3)
    R = np.array([random_rotation(rng) for _ in range(5)])
    R[4] = np.nan
    rot = ra.GlobalRotations(R, np.array([True, True, True, True, False]), np.array([1, 2, 3, 0, -1]), np.zeros(6), 1, 1, 0.0, 0.0,
                             "converged")
    seen = {}

    def fake(C, pair_arr, v, w, root, loss, scale, init, options, rotations=None):
        seen.update(C=C, pairs=pair_arr, v=v, w=w, root=root, loss=loss, scale=scale, init=init, options=options, R=rotations)
        return ta.GlobalPositions(np.zeros((C, 3)), np.ones(C, bool), np.zeros(C), np.array([1.0, 2.0]), np.array([0.5, 0.25]), 1,
                                  1, 0.0, 0.0, "converged")

    monkeypatch.setattr(ta, "_run", fake)
    out = ta.average_graph_translations(graph, rot, 5, loss="huber", max_steps=7)
    # (4, 2) is a pair rotation averaging would use, but image 4 is not registered in the rotations
    assert seen["C"] == 5 and seen["pairs"].tolist() == [[0, 1], [3, 0]] and seen["w"].tolist() == [40.0, 75.0]
    assert np.array_equal(seen["v"], t[[0, 3]]) and seen["root"] == 3 and seen["loss"] == "huber"
    assert seen["scale"] == pytest.approx(np.sin(np.radians(2.0))) and seen["options"]["max_steps"] == 7
    assert seen["options"]["warmup_steps"] == 10 and np.array_equal(seen["R"][:4], R[:4]) and np.isnan(seen["R"][4]).all()
    assert np.array_equal(out.residual_deg, [1.0, np.nan, np.nan, 2.0, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(out.scale, [0.5, np.nan, np.nan, 0.25, np.nan, np.nan], equal_nan=True)
    ta.average_graph_translations(graph, rot, 5, root=1)
    assert seen["root"] == 1
    with pytest.raises(ValueError, match="graph.pose"):
        ta.average_graph_translations(graph._replace(pose=None), rot, 5)
    with pytest.raises(ValueError, match="unknown options"):
        ta.average_graph_translations(graph, rot, 5, steps=3)
    with pytest.raises(ValueError, match="max_steps"):
        ta.average_graph_translations(graph, rot, 5, max_steps=-1)
    with pytest.raises(ValueError, match="rotations.R"):
        ta.average_graph_translations(graph, rot, 6)


def test_global_poses():
    from rotation_averaging_oracle import random_rotation
    from structure_from_motion_amd.multiview import rotation_averaging as ra
    from structure_from_motion_amd.multiview import translation_averaging as ta

    rng = np.random.default_rng(4)
    R = np.array([random_rotation(rng) for _ in range(4)])
    c = rng.normal(size=(4, 3))
    rot = ra.GlobalRotations(R, np.array([True, True, False, True]), np.zeros(4), np.zeros(0), 1, 1, 0.0, 0.0, "converged")
    pos = ta.GlobalPositions(c, np.array([True, True, True, False]), np.zeros(4), np.zeros(0), np.zeros(0), 1, 1, 0.0, 0.0, "converged")
    P = ta.global_poses(rot, pos)
    assert P.shape == (4, 3, 4) and np.isnan(P[2:]).all() and np.array_equal(P[:2, :, :3], R[:2])
    for k in range(2):   # the centre projects to the origin of its camera
        assert np.allclose(P[k] @ np.append(c[k], 1.0), 0.0, atol=1e-15)
    with pytest.raises(ValueError, match="positions.c"):
        ta.global_poses(rot, ta.GlobalPositions(c[:3], np.ones(3, bool), np.zeros(3), np.zeros(0), np.zeros(0), 1, 1, 0.0, 0.0, "x"))


# ---- the properties of the definition that the GPU tests rest on ----------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["dense", "pcg"])
def test_oracle_recovers_exact_positions_up_to_scale(solver):
    g = to.make_graph(12, 30, seed=9, noise_deg=0.0)
    for loss in to.LOSSES:
        r = to.average_translations(12, g["pairs"], g["directions"], loss=loss, solver=solver, step_tolerance=1e-10,
                                    max_steps=1000)
        err = to.max_position_error(r["c"], g["centres"])
        print(solver, loss, "steps", r["steps"], "largest error after alignment", err, "largest residual", r["residual"].max())
        assert r["status"] == to.CONVERGED and r["registered"].all()
        # the alternation converges linearly: a last step of 1e-10 at a rate up to 0.9999 leaves at most 1e-6 (scene radius
        # about 5).  Measured 1.4e-8 to 1.7e-8 after 433 to 544 steps, residuals below 8e-10 rad.
        assert err <= 1e-6 and r["residual"].max() <= 1e-7
    chain = to.case_chain(40)
    r = to.run_case(chain, solver=solver)
    assert r["status"] == to.CONVERGED and to.max_position_error(r["c"], chain["centres"]) <= 1e-12   # unit baselines: the tree is exact


def test_oracle_dense_and_pcg_agree():
    """The spread the GPU tests' tolerance is 1 000 times of: dense against PCG with reversed adjacency order, at the fixed
    step counts of the GPU tests' comparisons."""
    worst = 0.0
    for name, case, options in to.comparison_cases():
        dense = to.run_case(case, solver="dense", **to.FIXED, **options)
        pcg = to.run_case(case, solver="pcg", reverse_adjacency=True, **to.FIXED, **options)
        s = to.spread(dense, pcg)
        worst = max(worst, s)
        print(f"{name}: spread {s:.3g} after {dense['steps']} steps, cg {pcg['cg_iterations']} (most {pcg['cg_max']})")
        assert dense["status"] == pcg["status"] == to.MAX_STEPS and dense["steps"] == pcg["steps"] == options["max_steps"]
    # measured: hub 1.52e-12, ring 6.54e-13 (what CG to 1e-12 leaves of a step), losses squared 1.78e-15, huber 3.11e-15,
    # reversed edge 8.88e-16, reversed camera 8.88e-16, registration 2.78e-17.  Three times the largest leaves room for
    # another LAPACK behind the dense solve; 1 000 times it stays below the cap of 1e-8 tree baselines.
    assert worst <= 3 * ORACLE_SPREAD and 1000 * ORACLE_SPREAD < 1e-8


@pytest.fixture(scope="module")
def losses():
    case = to.case_losses()
    kw = dict(solver="dense", max_steps=300)
    squared = to.run_case(case, **kw)
    huber = to.run_case(case, loss="huber", loss_scale=to.HUBER_SCALE, **kw)
    cauchy = to.run_case(case, loss="cauchy", loss_scale=to.HUBER_SCALE, warmup_steps=0, initial_positions=huber["c"], **kw)
    tree = to.run_case(case, loss="cauchy", loss_scale=to.HUBER_SCALE, warmup_steps=0, **kw)
    return case, squared, huber, cauchy, tree


def test_oracle_losses_on_the_outlier_graph(losses):
    """The seed of ``case_losses`` is one for which the definition alone meets every condition of the GPU test."""
    case, squared, huber, cauchy, tree = losses
    assert case["outlier"].sum() == 10 and len(case["pairs"]) == 104   # 10 %
    err = {name: to.max_position_error(r["c"], case["centres"]) for name, r in
           (("squared", squared), ("huber", huber), ("cauchy", cauchy), ("cauchy from the tree", tree))}
    res = np.degrees(cauchy["residual"])
    print(err, "steps", squared["steps"], huber["steps"], cauchy["steps"], tree["steps"], "smallest planted residual",
          res[case["outlier"]].min(), "largest other", res[~case["outlier"]].max(), "costs", cauchy["final_cost"], tree["final_cost"])
    assert err["squared"] > 3.0 * err["huber"] and err["huber"] < 0.3      # measured 1.18 against 0.167, scene radius about 5
    assert set(np.nonzero(res > 5.0)[0]) == set(np.nonzero(case["outlier"])[0])
    assert res[case["outlier"]].min() > 20.0 and res[~case["outlier"]].max() < 2.5   # measured 32.3 and 1.51
    assert tree["final_cost"] > 1.5 * cauchy["final_cost"]                  # measured 0.189 against 0.0874
    assert huber["status"] == cauchy["status"] == to.CONVERGED


def test_oracle_small_properties():
    rng = np.random.default_rng(5)
    v = to.unit(rng.normal(size=(1, 3)))
    # one edge either way round: the other camera sits at +v or -v bit for bit, after one step that is exactly zero
    for pairs, want in (([[0, 1]], v[0]), ([[1, 0]], -v[0])):
        r = to.average_translations(2, np.array(pairs), v, warmup_steps=0)
        assert np.array_equal(r["c"][1], want) and r["steps"] == 1 and r["cg_iterations"] == 0 and r["status"] == to.CONVERGED
        assert r["residual"][0] == 0.0 and r["scale"][0] == 1.0
    r = to.average_translations(2, np.array([[0, 1]]), v, warmup_steps=3)   # no convergence during the warm-up
    assert r["steps"] == 4 and r["status"] == to.CONVERGED
    # bad indices and a self-pair
    for pairs in ([[0, 2], [0, 1]], [[-1, 0], [0, 1]], [[1, 1], [0, 1]]):
        r = to.average_translations(2, np.array(pairs), np.repeat(v, 2, axis=0))
        assert r["status"] == to.BAD_INDEX and np.isnan(r["c"]).all() and np.isnan(r["residual"]).all() and not r["registered"].any()
    # the world directions from (R, t) point from i to j
    case = to.case_registration()
    got = to.world_directions(case["pairs"], case["t"], np.nan_to_num(case["R"]))
    for q in (0, 1, 2, 3, 10):
        i, j = case["pairs"][q]
        assert np.allclose(got[q], to.unit(case["centres"][j] - case["centres"][i]), atol=1e-14)
    r = to.run_case(case, solver="dense")
    assert r["registered"].tolist() == case["registered"] and r["level"].tolist() == case["level"]
    assert (~np.isnan(r["residual"])).tolist() == case["used"] and np.isnan(r["c"][~r["registered"]]).all()
    # a reversed edge ends with the scale 0 and a residual next to 180 degrees; a camera all of whose edges are reversed does
    # not move (its row of the system is zero) and nothing is NaN
    case, q = to.case_reversed_edge()
    r = to.run_case(case, solver="pcg", warmup_steps=0, max_steps=30)
    assert r["scale"][q] == 0.0 and np.degrees(r["residual"][q]) > 175.0 and np.isfinite(r["c"]).all()
    case, camera, at = to.case_reversed_camera()
    for solver in ("dense", "pcg"):
        r = to.run_case(case, solver=solver, warmup_steps=0, max_steps=10, initial_positions=case["initial"])
        assert np.array_equal(r["c"][camera], case["initial"][camera]) and np.all(r["scale"][at] == 0.0)
        assert np.isfinite(r["c"]).all() and np.isfinite(r["residual"]).all() and np.degrees(r["residual"][at]).min() > 175.0
