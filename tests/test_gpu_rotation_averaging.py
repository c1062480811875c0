"""Rotation averaging over a view graph on the GPU (csrc/sfm_rotation_averaging.hip) against the NumPy
definition of tests/rotation_averaging_oracle.py: the smallest graphs, the spanning-tree start bit for bit, long chains, what is
registered, a hub, more cameras than a workgroup has threads, the three losses on a graph with wrong edges, determinism, refused
indices through the C ABI, and a view graph from ``verify_pairs`` through the app."""
import ctypes

import numpy as np
import pytest
import torch

import rotation_averaging_oracle as ro

pytestmark = pytest.mark.gpu

# Tolerance against the oracle, in radians, for converged runs and runs of an equal step count: 1 000 x the largest rotation
# difference between the oracle's dense variant and its PCG variant with reversed adjacency order over the cases below
# (measured on the CPU: chain 0, hub 2.36e-16, ring 1.87e-16, losses squared 3.55e-16, huber 7.98e-17, cauchy 1.09e-16),
# for the device's different reduction trees; it stays below the cap of 1e-8 rad.
ORACLE_SPREAD = 3.55e-16
TOL = min(1000 * ORACLE_SPREAD, 1e-8)
TIGHT = dict(step_tolerance=1e-12)   # converged runs stop well below TOL, whichever step count they stop at
ONE_DEG = np.radians(1.0)


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _device(case, **kw):
    from lib.multiview.rotation_averaging import average_rotations

    return average_rotations(case["C"], case["pairs"], case["relative"], case.get("weights"), root=case.get("root", 0), **kw)


def _oracle(case, loss_scale_deg=1.0, **kw):
    return ro.average_rotations(case["C"], case["pairs"], case["relative"], case.get("weights"), root=case.get("root", 0),
                                loss_scale=np.radians(loss_scale_deg), **kw)


def _assert_matches(got, want, where):
    """Registration, levels, step count and status equal; rotations, residuals and costs within the tolerance.  Where
    the oracle ran ``solver="pcg"`` and every one of its solves ended at ``max_cg_iterations`` (``cg_at_limit``), ``cg_iterations``
    equals too; a solve that stops at its tolerance may stop an iteration apart.  The public record carries no ``cg_max``:
    tests/test_gpu_averaging_edges.py compares it on the device's info record."""
    assert np.array_equal(got.registered, want["registered"]) and np.array_equal(got.level, want["level"]), where
    assert got.status == ro.STATUS[want["status"]] and got.steps == want["steps"], (where, got.status, got.steps, want["steps"])
    diff = ro.max_rotation_difference(got.R, want["R"], want["registered"])
    used = ~np.isnan(want["residual"])
    assert np.array_equal(np.isnan(got.residual_deg), ~used), where
    res = float(np.max(np.abs(np.radians(got.residual_deg[used]) - want["residual"][used]))) if used.any() else 0.0
    print(f"{where}: steps {got.steps} cg {got.cg_iterations} status {got.status}; rotations differ by {diff:.3g} rad, "
          f"residuals by {res:.3g} rad; cost {got.initial_cost:.6g} -> {got.final_cost:.6g}")
    assert np.isnan(got.R[~want["registered"]]).all(), where
    assert diff <= TOL and res <= 2 * TOL, (where, diff, res)   # a residual sees the rotations of both ends
    for a, b in ((got.initial_cost, want["initial_cost"]), (got.final_cost, want["final_cost"])):
        assert abs(a - b) <= 1e-9 * max(abs(b), 1e-12), (where, a, b)   # a sum of Q terms, each good to TOL
    if want.get("cg_at_limit"):
        assert got.cg_iterations == want["cg_iterations"], (where, got.cg_iterations, want["cg_iterations"])


# ---- 1. the smallest graphs --------------------------------------------------------------------------------------------------
def test_one_camera_no_edge(dev):
    from structure_from_motion_amd import device

    R, reg, level, residual, info = device.average_rotations(
        torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((0, 3, 3), dtype=torch.float64, device=dev),
        torch.zeros(0, dtype=torch.float64, device=dev), 1)
    rec = device.read_rotavg_info(info)
    assert np.array_equal(R.cpu().numpy(), np.eye(3)[None]) and reg.cpu().tolist() == [1] and level.cpu().tolist() == [0]
    assert residual.numel() == 0 and rec.status == device.ROTAVG_CONVERGED and rec.steps == 0 and rec.registered == 1
    assert rec.initial_cost == 0.0 and rec.final_cost == 0.0 and rec.cg_iterations == 0


@pytest.mark.parametrize("reverse", [False, True])
def test_two_cameras_one_edge(dev, reverse):
    Rq = ro.random_rotation(np.random.default_rng(11))
    case = dict(C=2, pairs=np.array([[1, 0]] if reverse else [[0, 1]]), relative=Rq[None])
    got = _device(case)   # the defaults: D = R_q^T R_q (or R_q R_q^T) is symmetric bit for bit, so the step is exactly zero
    want = Rq.T if reverse else Rq
    assert np.array_equal(_bits(got.R[1]), _bits(want)) and np.array_equal(got.R[0], np.eye(3))
    assert got.status == "converged" and got.steps == 1 and got.cg_iterations == 0 and got.registered.all()
    assert got.residual_deg[0] == 0.0 and got.level.tolist() == [0, 1]


# ---- 2. the spanning-tree start, bit for bit -------------------------------------------------------------------------------------
def _tree_cases():
    rng = np.random.default_rng(12)
    R_true = np.array([np.eye(3)] + [ro.random_rotation(rng) for _ in range(5)])
    pairs, rel = ro.noisy_edges(R_true, [(0, 1), (2, 1), (2, 3), (4, 3)], rng)
    yield "chain of 5, mixed orientations", dict(C=5, pairs=pairs, relative=rel, weights=np.array([1.0, 2.0, 0.5, 1.0]), root=0)
    # camera 3 touches cameras 1 and 2 (both level 1): the lighter edge comes first and is a random rotation
    pairs, rel = ro.noisy_edges(R_true, [(0, 1), (0, 2), (3, 1), (2, 3)], rng)
    rel[2] = ro.random_rotation(rng)
    yield "heavier edge", dict(C=4, pairs=pairs, relative=rel, weights=np.array([1.0, 1.0, 3.0, 7.0]), root=0)
    # equal weights: the lower half-edge index wins, here the edge (3, 1) with its own (wrong) rotation
    yield "weight tie", dict(C=4, pairs=pairs, relative=rel, weights=np.array([1.0, 1.0, 4.0, 4.0]), root=0)


@pytest.mark.parametrize("name,case", list(_tree_cases()), ids=[n for n, _ in _tree_cases()])
def test_tree_initialisation_bit_equal(dev, name, case):
    got = _device(case, max_steps=0)
    level, R = ro.levels_and_tree(case["C"], case["pairs"], case["relative"], case["weights"], case["root"])
    assert np.array_equal(got.level, level) and np.array_equal(got.registered, level >= 0)
    assert np.array_equal(_bits(got.R), _bits(R)), name
    assert got.status == "max_steps" and got.steps == 0 and got.initial_cost == got.final_cost
    want = _oracle(case, max_steps=0)
    assert np.array_equal(_bits(want["R"]), _bits(R))
    if name == "heavier edge":     # through (2, 3), not through the wrong (3, 1)
        assert np.array_equal(_bits(R[3]), _bits(ro.mul(case["relative"][3], R[2]))) and got.residual_deg[2] > 5.0
    if name == "weight tie":
        assert np.array_equal(_bits(R[3]), _bits(ro.mul(case["relative"][2].T, R[1])))


# ---- 3. a chain: one level round per camera ----------------------------------------------------------------------------------
def test_chain_of_300(dev):
    case = ro.case_chain()
    got = _device(case, max_cg_iterations=400, **TIGHT)
    assert got.status == "converged" and got.registered.all() and np.array_equal(got.level, np.arange(300))
    print("chain: steps", got.steps, "cg", got.cg_iterations, "largest residual (rad)", np.radians(got.residual_deg).max())
    assert np.radians(got.residual_deg).max() <= 1e-12   # a tree: every edge can be met exactly
    _assert_matches(got, _oracle(case, solver="dense", **TIGHT), "chain of 300")


# ---- 4. what is registered -----------------------------------------------------------------------------------------------------
def test_registration(dev):
    rng = np.random.default_rng(13)
    C = 9
    R_true = np.array([ro.random_rotation(rng) for _ in range(C)])
    #        component of the root 3         another component   7 only through weight 0, 8 only through a NaN rotation
    edges = [(3, 4), (5, 4), (0, 5), (3, 0), (1, 2), (2, 1),     (7, 3), (4, 8), (7, 8)]
    pairs, rel = ro.noisy_edges(R_true, edges, rng)
    w = np.array([1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0])
    rel[7, 1, 1] = np.nan
    case = dict(C=C, pairs=pairs, relative=rel, weights=w, root=3)
    got = _device(case, **TIGHT)
    assert got.registered.tolist() == [True, False, False, True, True, True, False, False, False]
    assert got.level.tolist() == [1, -1, -1, 0, 1, 2, -1, -1, -1]
    assert np.isnan(got.R[~got.registered]).all() and np.isfinite(got.R[got.registered]).all()
    assert np.isnan(got.residual_deg[4:]).all() and np.isfinite(got.residual_deg[:4]).all()
    gram = np.einsum("cki,ckj->cij", got.R[got.registered], got.R[got.registered]) - np.eye(3)
    assert np.max(np.abs(gram)) <= 1e-12 and np.array_equal(got.R[3], np.eye(3))
    _assert_matches(got, _oracle(case, solver="dense", **TIGHT), "registration")
    for bad in (-1.0, np.inf, np.nan):   # every weight that is not finite and positive switches its edge off
        w2 = w.copy()
        w2[2] = bad
        again = _device(dict(case, weights=w2), **TIGHT)
        assert np.isnan(again.residual_deg[2]) and again.registered[0] and again.level[5] == 2


# ---- 5. a hub and parallel edges ---------------------------------------------------------------------------------------------------
def test_hub_of_degree_750(dev):
    case = ro.case_hub()
    assert np.count_nonzero(case["pairs"] == 0) == 750
    got = _device(case, **TIGHT)
    assert got.status == "converged" and got.registered.all() and got.level[0] == 1 and got.level.max() == 2
    _assert_matches(got, _oracle(case, solver="dense", **TIGHT), "hub")


# ---- 6. more free cameras than a workgroup has threads --------------------------------------------------------------------------
def test_ring_of_1100(dev):
    case = ro.case_ring()
    got = _device(case, **TIGHT)
    assert got.status == "converged" and got.registered.all()
    _assert_matches(got, _oracle(case, solver="dense", **TIGHT), "ring of 1100")
    # against the truth: within what the spanning tree guarantees, the largest edge error times the deepest level
    Rt = case["R_true"]
    edge_err = max(ro.angle_between(case["relative"][q], Rt[j] @ Rt[i].T) for q, (i, j) in enumerate(case["pairs"]))
    err = np.radians(ro.max_error_deg(got.R, Rt))
    print("ring of 1100: largest error against the truth", err, "rad; largest edge error", edge_err, "deepest level", got.level.max())
    assert err <= edge_err * got.level.max()


# ---- 7. the losses on a graph with wrong edges ------------------------------------------------------------------------------------
FIXED = dict(max_steps=60, step_tolerance=1e-300, cg_tolerance=1e-10)   # an equal, fixed step count for the robust losses


@pytest.fixture(scope="module")
def losses(dev):
    case = ro.case_losses()
    squared = _device(case, **TIGHT)
    huber = _device(case, loss="huber", **FIXED)
    cauchy = _device(case, loss="cauchy", initial_rotations=huber.R, **FIXED)
    return case, squared, huber, cauchy


def test_losses_against_oracle(losses):
    case, squared, huber, cauchy = losses
    _assert_matches(squared, _oracle(case, solver="dense", **TIGHT), "squared")
    _assert_matches(huber, _oracle(case, loss="huber", **FIXED), "huber")
    _assert_matches(cauchy, _oracle(case, loss="cauchy", initial_rotations=huber.R, **FIXED), "cauchy from huber")


def test_losses_inequalities(losses):
    case, squared, huber, cauchy = losses
    clean = ~case["outlier"]
    alone = _device(dict(case, pairs=case["pairs"][clean], relative=case["relative"][clean], weights=None))
    err = {name: ro.max_error_deg(r.R, case["R_true"]) for name, r in
           (("squared", squared), ("huber", huber), ("cauchy", cauchy), ("clean edges alone", alone))}
    print("largest error in degrees:", err)
    assert err["squared"] > 20.0 and err["huber"] < 3.0 and err["cauchy"] <= 2.0 * err["clean edges alone"]
    from lib.multiview.rotation_averaging import inconsistent_pairs

    assert inconsistent_pairs(cauchy, 5.0).tolist() == np.nonzero(case["outlier"])[0].tolist()
    assert cauchy.final_cost <= cauchy.initial_cost and huber.final_cost <= huber.initial_cost


def test_half_turn_edge(dev):
    """D = diag(1, -1, -1) exactly: the branch of the logarithm at pi."""
    half = np.diag([1.0, -1.0, -1.0])
    case = dict(C=2, pairs=np.array([[0, 1]]), relative=half[None])
    start = _device(case, initial_rotations=np.array([np.eye(3), np.eye(3)]), max_steps=0)
    assert start.residual_deg[0] == pytest.approx(180.0, abs=1e-12) and np.array_equal(start.R[1], np.eye(3))
    assert start.initial_cost == pytest.approx(np.pi ** 2, rel=1e-15)
    moved = _device(case, initial_rotations=np.array([np.eye(3), np.eye(3)]))
    assert np.isfinite(moved.R).all() and moved.status == "converged" and moved.residual_deg[0] <= 1e-10
    assert ro.angle_between(moved.R[1], half) <= 1e-12
    _assert_matches(moved, _oracle(case, initial_rotations=np.array([np.eye(3), np.eye(3)])), "half turn")


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------------
def test_same_bytes_twice_and_permuted_edges(dev):
    from structure_from_motion_amd import device

    case = ro.case_losses()
    rng = np.random.default_rng(14)
    w = rng.uniform(0.5, 2.0, size=104)   # distinct weights: the tree does not depend on the order of the edges
    args = lambda idx: (device.to_device(case["pairs"][idx].astype(np.int32), torch.int32), device.to_device(case["relative"][idx]),   # noqa: E731
                        device.to_device(w[idx]), 24)
    kw = dict(loss="huber", loss_scale=ONE_DEG, max_steps=30)
    same = np.arange(104)
    first = [t.cpu().numpy().tobytes() for t in device.average_rotations(*args(same), **kw)]
    again = [t.cpu().numpy().tobytes() for t in device.average_rotations(*args(same), **kw)]
    assert first == again
    # another order of the edges is another order of every camera's sums: the same rotations up to rounding, not the same bits
    perm = rng.permutation(104)
    a = _device(dict(case, weights=w), step_tolerance=1e-13, max_steps=100)
    b = _device(dict(case, pairs=case["pairs"][perm], relative=case["relative"][perm], weights=w[perm]), step_tolerance=1e-13,
                max_steps=100)
    diff = ro.max_rotation_difference(a.R, b.R)
    print("permuted edges: steps", a.steps, b.steps, "rotations differ by", diff, "rad")
    assert a.status == b.status == "converged" and diff <= TOL
    assert np.max(np.abs(a.residual_deg[perm] - b.residual_deg)) <= np.degrees(2 * TOL)


# ---- 9. refused indices through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_pair", [(0, 6), (-1, 2), (3, 3), (2**31 - 1, 0)])
def test_bad_index_fills_every_output(dev, native_lib, bad_pair):
    from structure_from_motion_amd import _native, device

    C, Q, guard = 6, 5, 64
    rng = np.random.default_rng(15)
    pairs = np.array([(0, 1), (1, 2), bad_pair, (3, 4), (4, 5)], dtype=np.int32)
    rel = np.array([ro.random_rotation(rng) for _ in range(Q)])
    lib = native_lib
    bytes_ = lib.sfm_average_rotations_workspace_bytes(C, Q)
    ws = torch.zeros(bytes_ + guard, dtype=torch.uint8, device=dev)
    ws[bytes_:] = 0xA5
    # every output with a guard behind it and a pattern in it
    R = torch.full((9 * C + guard,), 7.0, dtype=torch.float64, device=dev)
    reg = torch.full((C + guard,), 9, dtype=torch.uint8, device=dev)
    level = torch.full((C + guard,), 77, dtype=torch.int32, device=dev)
    residual = torch.full((Q + guard,), 7.0, dtype=torch.float64, device=dev)
    info = torch.full((5 + guard,), 123, dtype=torch.int64, device=dev)
    opts = _native.RotavgOptions(0, _native.ROTAVG_INIT_TREE, 10, 50, 1.0, 1e-6, 1e-8)
    p, r, w = device.to_device(pairs, torch.int32), device.to_device(rel), device.to_device(np.ones(Q))
    rc = lib.sfm_average_rotations(C, Q, p.data_ptr(), r.data_ptr(), w.data_ptr(), 0, None, ctypes.byref(opts), R.data_ptr(),
                                   reg.data_ptr(), level.data_ptr(), residual.data_ptr(), info.data_ptr(), ws.data_ptr(), bytes_,
                                   None)
    torch.cuda.synchronize()
    assert rc == 0, lib.sfm_last_error()
    rec = device.read_rotavg_info(info[:5])
    assert rec.status == device.ROTAVG_BAD_INDEX and rec.steps == 0 and rec.registered == 0 and rec.cg_iterations == 0
    assert np.isnan(rec.initial_cost) and np.isnan(rec.final_cost)
    assert torch.isnan(R[:9 * C]).all() and torch.isnan(residual[:Q]).all()
    assert (reg[:C] == 0).all() and (level[:C] == -1).all()
    assert (R[9 * C:] == 7.0).all() and (residual[Q:] == 7.0).all() and (reg[C:] == 9).all() and (level[C:] == 77).all()
    assert (info[5:] == 123).all() and (ws[bytes_:] == 0xA5).all()


# ---- 10. a view graph from verify_pairs, and the app ---------------------------------------------------------------------------------
def _longest_tree_path(level):
    return int(level.max())


def test_view_graph_integration(dev):
    from lib.epipolar.view_graph import verify_pairs
    from lib.multiview.rotation_averaging import average_graph_rotations
    from structure_from_motion_amd import synthetic
    from structure_from_motion_amd.multiview.rotation_averaging import graph_edges

    views = 6
    scene = synthetic.multi_view_scene(views, 1500, 21, 0.5, 0.2, step_deg=5.0)
    pm = synthetic.pairwise_matches(scene, seed=21)
    graph = verify_pairs(scene["K"], pm["features"], pm["pairs"], pm["matches"], 6e-6, min_extra_fraction=0.4, max_iterations=500,
                         seed=5, relative_pose=True)
    got = average_graph_rotations(graph, views, **TIGHT)
    idx, pairs, R, w = graph_edges(graph)
    assert len(idx) >= views - 1 and got.registered.all() and got.status == "converged"
    root = int(pairs[int(np.argmax(w))].min())
    assert np.array_equal(got.R[root], np.eye(3)) and got.level[root] == 0
    want = ro.average_rotations(views, pairs, R, w, root=root, solver="dense", **TIGHT)
    sub = type(got)(**{**got.__dict__, "residual_deg": got.residual_deg[idx]})
    _assert_matches(sub, want, "view graph")
    assert np.isnan(np.delete(got.residual_deg, idx)).all()
    # the truth in the root's gauge; per-edge error of the graph's relative rotations
    Rt = scene["poses_true"][:, :9].reshape(-1, 3, 3)
    truth = np.array([Rt[v] @ Rt[root].T for v in range(views)])
    edge_err = max(ro.angle_between(R[k], Rt[j] @ Rt[i].T) for k, (i, j) in enumerate(pairs))
    bound = edge_err * _longest_tree_path(got.level)
    start = average_graph_rotations(graph, views, max_steps=0)
    err_start = max(ro.angle_between(start.R[v], truth[v]) for v in range(views))
    err = max(ro.angle_between(got.R[v], truth[v]) for v in range(views))
    print(f"view graph: {len(idx)} edges, largest edge error {edge_err:.3g} rad, deepest level {got.level.max()}, bound {bound:.3g}; "
          f"tree start {err_start:.3g} rad, averaged {err:.3g} rad")
    assert err_start <= bound and err <= bound


def test_app_global_rotations(dev):
    from apps import sfm_multi_view as app
    from test_gpu_view_graph_pose import PARENT_FIRST, PARENT_KEYS, _assert_same_values

    for kwargs in (dict(), dict(tracks="matches"), dict(verify="batched")):
        with pytest.raises(ValueError, match="needs tracks='matches' and verify='batched'"):
            app.run(rotations="global", **kwargs)
    with pytest.raises(ValueError, match="rotations"):
        app.run(rotations="best")
    plain = app.run(views=8, tracks="matches", verify="batched")
    _assert_same_values(plain, PARENT_FIRST)   # without the flag: the keys and the values of before
    assert set(plain) == PARENT_KEYS
    out = app.run(views=8, tracks="matches", verify="batched", rotations="global", details=True)
    glob = out["global_rotations"]
    print("global rotations:", glob)
    assert set(out) - {"_scene", "_status", "_graph"} == PARENT_KEYS | {"global_rotations"}
    assert sorted(glob["rotation_error_rad"]) == list(range(8)) and glob["views_registered"] == 8
    assert glob["status"] in ("converged", "max_steps") and glob["steps"] >= 1 and glob["pairs_dropped"] == 0
    # every view within the spanning tree's bound: the largest error of a used pair's rotation times the deepest level
    from structure_from_motion_amd.multiview.rotation_averaging import average_graph_rotations, graph_edges

    graph, Rt = out["_graph"], out["_scene"]["poses_true"][:, :9].reshape(-1, 3, 3)
    idx, pairs, R, w = graph_edges(graph)
    edge_err = max(ro.angle_between(R[k], Rt[j] @ Rt[i].T) for k, (i, j) in enumerate(pairs))
    depth = int(average_graph_rotations(graph, 8, max_steps=0).level.max())
    print("largest edge error", edge_err, "rad, deepest level", depth)
    assert max(glob["rotation_error_rad"].values()) <= edge_err * depth
    # a reported pair is a pair of the graph whose rotation is off by more than the limit less the two views' own errors
    worst = max(glob["rotation_error_rad"].values())
    where = {tuple(int(v) for v in p): k for k, p in enumerate(pairs)}
    for p in glob["inconsistent_pairs"]:
        i, j = p
        assert ro.angle_between(R[where[(i, j)]], Rt[j] @ Rt[i].T) > np.radians(5.0) - 2 * worst, p
    # reporting drops nothing: everything downstream is what it was
    _assert_same_values({k: v for k, v in out.items() if k in PARENT_KEYS}, PARENT_FIRST)
