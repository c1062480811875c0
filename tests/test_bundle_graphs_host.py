"""Irregular observation graphs, host side: the generator of tests/bundle_graphs.py keeps its promises (track lengths,
sparse cameras, duplicates, unobserved points, orders), and on such graphs the oracles' solvers agree with each other
(dense and Schur; tight PCG and Schur) and never raise, one-camera moving points included (no GPU)."""
import numpy as np
import pytest

import bundle_graphs as bg
import bundle_oracle as bo
import bundle_pcg_oracle as pco

K = bg.synthetic.BENCH_K


def _adjust(pr, **kw):
    return bo.adjust(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], **kw)


def _distinct_per_point(pr, P):
    pairs = np.unique(np.column_stack([pr["point_indices"], pr["camera_indices"]]), axis=0)
    return np.bincount(pairs[:, 0], minlength=P)


@pytest.mark.parametrize("order", bg.ORDERS)
def test_generator_track_lengths_duplicates_and_order(order):
    C, P = 12, 2000
    pr = bg.irregular_problem(C, P, 5, singles=150, one_camera=30, pairs=400, full=7, unobserved=60, mid=(3, 6),
                              duplicates=90, order=order)
    cam, pt = pr["camera_indices"].astype(np.int64), pr["point_indices"].astype(np.int64)
    assert pr["poses"].shape == (C, 12) and pr["points"].shape == (P, 3) and pr["pixels"].shape == (len(cam), 2)
    assert np.array_equal(pr["poses"][0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    # every point in front of every camera
    R, t = pr["poses_true"][:, :9].reshape(-1, 3, 3), pr["poses_true"][:, 9:]
    assert np.all(np.einsum("cij,pj->cpi", R, pr["points_true"])[..., 2] + t[:, None, 2] > 1.0)
    # track lengths (distinct cameras per point): 0, 1 (singles and one-camera points), 2, 3 .. 6 and C
    n = _distinct_per_point(pr, P)
    hist = np.bincount(n, minlength=C + 1)
    assert hist[0] == 60 and hist[1] == 180 and hist[2] == 400 and hist[C] == 7
    assert hist[3:7].sum() == P - 60 - 180 - 400 - 7 and hist[7:C].sum() == 0 and np.all(hist[3:7] > 0)
    # duplicates: 90 on multi-camera points, 30 making the one-camera points
    key = pt * C + cam
    _, counts = np.unique(key, return_counts=True)
    assert counts.max() == 2 and np.count_nonzero(counts == 2) == 120
    dup_pts = np.unique(key, return_counts=True)[0][counts == 2] // C
    obs = np.bincount(pt, minlength=P)
    assert np.count_nonzero(n[dup_pts] == 1) == 30 and np.all(obs[dup_pts[n[dup_pts] == 1]] == 2)
    assert np.count_nonzero(n[dup_pts] >= 2) == 90
    # duplicates carry their own pixel noise
    s = np.lexsort((np.arange(len(key)), key))
    same = key[s][1:] == key[s][:-1]
    assert np.all(np.any(pr["pixels"][s][1:][same] != pr["pixels"][s][:-1][same], axis=1))
    # the order
    if order == "camera-major":
        assert np.all(np.diff(cam * P + pt) >= 0)
    elif order == "point-major":
        assert np.all(np.diff(pt * C + cam) >= 0)
    elif order == "reversed":
        assert np.all(np.diff(cam * P + pt) <= 0)
    else:
        assert not np.all(np.diff(cam) >= 0) and not np.all(np.diff(pt) >= 0)
    # one seed is one graph: the orders permute the same observations
    base = bg.irregular_problem(C, P, 5, singles=150, one_camera=30, pairs=400, full=7, unobserved=60, mid=(3, 6),
                                duplicates=90, order="random")
    rows = lambda q: np.sort(np.column_stack([q["camera_indices"], q["point_indices"], q["pixels"]]).view(
        [("c", "f8"), ("p", "f8"), ("u", "f8"), ("v", "f8")]).ravel(), order=["c", "p", "u", "v"])
    assert np.array_equal(rows(pr), rows(base))
    assert np.array_equal(pr["poses"], base["poses"]) and np.array_equal(pr["points"], base["points"])


def test_generator_sparse_cameras_and_full_length():
    C, P = 10, 1500
    pr = bg.irregular_problem(C, P, 6, singles=100, pairs=300, full=5, duplicates=50, sparse={3: 9, 7: 0, 9: 12})
    cam, pt = pr["camera_indices"], pr["point_indices"]
    per_cam = np.bincount(cam, minlength=C)
    assert per_cam[3] == 9 and per_cam[7] == 0 and per_cam[9] == 12
    # sparse cameras see distinct points that at least two other cameras see
    n_other = _distinct_per_point(dict(pr, camera_indices=cam[~np.isin(cam, [3, 7, 9])],
                                       point_indices=pt[~np.isin(cam, [3, 7, 9])]), P)
    for c in (3, 9):
        seen = pt[cam == c]
        assert len(np.unique(seen)) == len(seen) and np.all(n_other[seen] >= 2)
    # full-length tracks run over every camera that is not sparse
    assert np.count_nonzero(n_other == C - 3) == 5
    # an explicit full length, and C = 70 000 stays cheap
    pr = bg.irregular_problem(300, 500, 7, full=3, full_length=299)
    assert np.count_nonzero(_distinct_per_point(pr, 500) == 299) == 3
    pr = bg.irregular_problem(70000, 20000, 8, pairs=5000, mid=(3, 4), sparse={1: 5, 65537: 5}, order="camera-major")
    assert np.bincount(pr["camera_indices"], minlength=70000)[[1, 65537]].tolist() == [5, 5]
    assert np.all(np.diff(pr["camera_indices"]) >= 0)


@pytest.mark.parametrize("C,P,fixed,order", [(3, 150, (0,), "random"), (5, 200, (1,), "camera-major"),
                                             (6, 200, (0, 3), "point-major"), (8, 240, (0, 2, 4), "reversed")])
def test_dense_and_schur_solvers_agree_on_irregular_graphs(C, P, fixed, order):
    """As test_dense_and_schur_solvers_agree, on graphs with duplicates, held, unobserved and one-camera moving points
    and a sparse free camera.  The one-camera points' depth has condition about 1 / lambda, so the two solvers drift
    apart as lambda falls (6e-6 in the points after 30 steps at 5 x 200): 3 steps, as on the device."""
    pr = bg.irregular_problem(C, P, C + P, singles=P // 10, unobserved=P // 20, pairs=P // 5, one_camera=3, full=2,
                              duplicates=P // 25, sparse={C - 1: 8}, order=order)
    dense = _adjust(pr, fixed=fixed, max_steps=3, solver="dense")
    schur = _adjust(pr, fixed=fixed, max_steps=3, solver="schur")
    assert dense["accepted"] == schur["accepted"] >= 2 and dense["steps"] == schur["steps"]
    assert abs(dense["final_cost"] - schur["final_cost"]) <= 1e-9 * dense["final_cost"]
    assert np.max(np.abs(dense["poses"] - schur["poses"])) <= 1e-9
    assert np.max(np.abs(dense["points"] - schur["points"])) <= 1e-9


@pytest.mark.parametrize("C,P,seed", [(4, 300, 1), (8, 2000, 2), (31, 2000, 3), (70, 3000, 4)])
def test_tight_pcg_step_equals_schur_step_on_irregular_graphs(C, P, seed):
    """As test_tight_pcg_step_equals_schur_step (cg_tolerance 1e-12 here, 6F iterations) on mixed graphs."""
    pr = bg.mixed(C, P, seed, full=C <= 32, one_camera=5)
    prob = pco.Problem(K, pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"], (0,))
    s = prob.system(pr["poses"], pr["points"])
    dc, dX = prob.solve_schur(s, 1e-3)
    (pdc, pdX), k = prob.solve_pcg(s, 1e-3, 1e-12, 6 * (C - 1))
    assert 1 <= k <= 6 * (C - 1)
    assert np.max(np.abs(pdc - dc)) <= 1e-8, np.max(np.abs(pdc - dc))
    assert np.max(np.abs(pdX - dX)) <= 1e-8, np.max(np.abs(pdX - dX))


def test_inverse3_is_the_cholesky_inverse():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(50, 3, 3))
    A = np.einsum("nij,nkj->nik", B, B) + 0.1 * np.eye(3)
    inv, ok = bo.inverse3(A)
    assert ok.all()
    assert np.max(np.abs(np.einsum("nij,njk->nik", inv, A) - np.eye(3))) <= 1e-10
    assert np.array_equal(inv, np.swapaxes(inv, 1, 2))
    # a rank-2 block with a tiny ridge still factors; a zero, an indefinite and a non-finite block do not
    v = np.array([1.0, 2.0, 3.0])
    rank2 = np.eye(3) - np.outer(v, v) / (v @ v)
    bad = np.stack([rank2 + 1e-12 * np.diag(np.diag(rank2)), np.zeros((3, 3)), np.diag([1.0, -1.0, 1.0]),
                    np.diag([1.0, np.nan, 1.0]), np.diag([np.inf, 1.0, 1.0])])
    inv, ok = bo.inverse3(bad)
    assert ok.tolist() == [True, False, False, False, False]
    assert np.all(np.isfinite(inv[0]))


@pytest.mark.parametrize("C,P", [(8, 1500), (32, 3000)])
def test_one_camera_moving_points_do_not_raise(C, P):
    """Points seen twice by one camera are moving points with V_p of rank 2: V_p* = V_p + lambda diag V_p factors for
    lambda > 0, and both oracles invert it as point_kernel does instead of raising.  They take the same LM path."""
    pr = bg.mixed(C, P, 9, one_camera=12, full=False)
    counts = np.bincount(pr["point_indices"], minlength=P)
    n = _distinct_per_point(pr, P)
    assert np.count_nonzero((counts == 2) & (n == 1)) == 12
    schur = _adjust(pr, max_steps=10)
    pcg = pco.adjust_pcg(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"],
                         max_steps=10, max_cg_iterations=6 * (C - 1), cg_tolerance=1e-12)
    assert schur["status"] == pcg["status"] == bo.OK
    assert schur["steps"] == pcg["steps"] and schur["accepted"] == pcg["accepted"] >= 3
    assert np.all(np.isfinite(schur["points"])) and np.all(np.isfinite(pcg["points"]))
    assert abs(schur["final_cost"] - pcg["final_cost"]) <= 1e-9 * schur["final_cost"]
    if C <= 8:
        dense = _adjust(pr, max_steps=10, solver="dense")
        assert (dense["status"], dense["steps"], dense["accepted"]) == (schur["status"], schur["steps"], schur["accepted"])


@pytest.mark.parametrize("kw", [dict(singles=200, unobserved=100), dict(unobserved=300), dict(sparse={5: 0})],
                         ids=["all-held", "no-observations", "camera-without-observations"])
def test_oracles_agree_on_degenerate_graphs(kw):
    """Graphs where no step or no point moves: both oracles report the same status and steps and do not raise."""
    pr = bg.irregular_problem(6, 300, 10, **kw)
    a = _adjust(pr, max_steps=30)
    b = pco.adjust_pcg(pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"],
                       max_steps=30)
    assert (a["status"], a["steps"], a["accepted"]) == (b["status"], b["steps"], b["accepted"])
    if a["accepted"] == 0:
        assert np.array_equal(a["poses"], pr["poses"]) and np.array_equal(a["points"], pr["points"])
