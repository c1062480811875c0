"""Refinement of a PnP winner on the MI355X (csrc/sfm_pnp_refine.hip): parity with the NumPy oracle of
tests/pnp_refine_oracle.py, accuracy against the raw DLT winner, batching, determinism, edge cases and the op layer."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import pnp_oracle as po
import pnp_refine_oracle as ro
from structure_from_motion_amd import synthetic
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.feature_matching.matching import Match

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
THR = 4.0
AGG = {"sum": 0, "square": 1, "mean": 2, "rms": 3}


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


def _pass(views, h, agg, seed, dev, min_extra=10):
    """A PnP pass over the views (list of (n, 5) arrays) with Philox samples: -> (workspace, pts on the device)."""
    from structure_from_motion_amd import device

    B, n = len(views), views[0].shape[0]
    pts = device.to_device(np.stack(views)).reshape(B, n, 5)
    ws = device.PnPWorkspace(B, n, h, dev)
    ws.run(pts, K, THR, min_extra, agg, philox=(seed, 0, 1000))
    return ws, pts


def _inputs(ws, b):
    """Host copies of view b's refinement inputs: (R, t, mask, err)."""
    from structure_from_motion_amd import device

    rec = device.read_select(ws.result)[b]
    assert rec.best_h >= 0
    m = ws.model[b, rec.best_h].cpu().numpy()
    return m[:9].reshape(3, 3), m[9:], ws.mask[b].cpu().numpy(), float(rec.best_err)


def _rotation_error(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0)))


@pytest.mark.parametrize("method", ["sum", "square", "mean", "rms"])
def test_parity_with_oracle(dev, method):
    from structure_from_motion_amd import device

    agg = AGG[method]
    views = [po.scene(2000, seed=100 + s, K=K, outlier_fraction=0.3, noise_px=0.5)[0] for s in range(3)]
    ws, pts = _pass(views, 400, agg, 5, dev)
    model, mask, info = ws.refine(pts, K, THR, agg, rounds=2, max_steps=20)
    model, mask, info = model.cpu().numpy(), mask.cpu().numpy(), device.read_pnp_refine_info(info)
    for b, view in enumerate(views):
        R0, t0, mask_in, err = _inputs(ws, b)
        ref = ro.refine(view, R0, t0, K, mask_in, err, THR, agg, rounds=2, max_steps=20)
        R, t = model[b, :9].reshape(3, 3), model[b, 9:]
        assert np.max(np.abs(R - ref["R"])) <= 1e-9, (b, np.max(np.abs(R - ref["R"])))
        assert np.max(np.abs(t - ref["t"])) <= 1e-9 * max(1.0, np.max(np.abs(ref["t"]))), b
        assert info[b].accepted == ref["accepted"] and info[b].accepted >= 1, (b, info[b])
        e = po.score_values(ref["R"], ref["t"], K, view)
        with np.errstate(invalid="ignore"):
            borderline = np.abs(e - THR) <= 1e-9 * THR
        assert np.array_equal(mask[b][~borderline], ref["mask"][~borderline]), b
        assert abs(info[b].count - ref["count"]) <= int(np.count_nonzero(borderline)), b
        if not borderline.any():
            assert info[b].count == ref["count"]
            assert abs(info[b].error - ref["error"]) <= 1e-9 * abs(ref["error"]), b


def test_refined_pose_beats_dlt_winner(dev):
    """The test that fails without the feature: over 10 noisy scenes, one round never raises the cost on the winner's
    inlier set, and the median rotation error to the ground truth drops."""
    scenes = [po.scene(1000, seed=200 + s, K=K, outlier_fraction=0.3, noise_px=0.5) for s in range(10)]
    ws, pts = _pass([s[0] for s in scenes], 500, AGG["rms"], 17, dev)
    model, _, _ = ws.refine(pts, K, THR, AGG["rms"], rounds=1)
    model = model.cpu().numpy()
    err_dlt, err_ref = [], []
    for b, (view, R_true, _) in enumerate(scenes):
        R0, t0, mask_in, _ = _inputs(ws, b)
        inl = view[mask_in != 0]
        R, t = model[b, :9].reshape(3, 3), model[b, 9:]
        assert ro.cost(R, t, K, inl) <= ro.cost(R0, t0, K, inl), b
        err_dlt.append(_rotation_error(R0, R_true))
        err_ref.append(_rotation_error(R, R_true))
    assert np.median(err_ref) < np.median(err_dlt), (err_ref, err_dlt)


def test_batch_equals_single_calls_and_is_deterministic(dev):
    from structure_from_motion_amd import device

    views = [po.scene(1500, seed=300 + s, K=K, outlier_fraction=0.3, noise_px=0.5)[0] for s in range(3)]
    ws, pts = _pass(views, 300, AGG["mean"], 9, dev)
    first = ws.refine(pts, K, THR, AGG["mean"], rounds=2)
    again = ws.refine(pts, K, THR, AGG["mean"], rounds=2)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    R_all = torch.arange(3, device=pts.device)
    model_in = ws.model[R_all, ws.result[:, 1].clamp(min=0)]
    err_in = ws.result[:, 2].contiguous().view(torch.float64)
    for b in range(3):
        one = device.pnp_refine(pts[b:b + 1].contiguous(), model_in[b:b + 1], ws.mask[b:b + 1], err_in[b:b + 1], K, THR,
                                AGG["mean"], 2, 20)
        for whole, single in zip(first, one):
            assert torch.equal(whole[b], single[0]), b


def test_zero_rounds_is_identity(dev):
    from structure_from_motion_amd import device

    views = [po.scene(800, seed=400 + s, K=K)[0] for s in range(2)]
    ws, pts = _pass(views, 200, AGG["rms"], 3, dev)
    R_all = torch.arange(2, device=pts.device)
    model_in = ws.model[R_all, ws.result[:, 1].clamp(min=0)].contiguous()   # a view without a winner keeps row 0
    model, mask, info = ws.refine(pts, K, THR, AGG["rms"], rounds=0)
    assert torch.equal(model, model_in)
    assert torch.equal(mask, (ws.mask != 0).to(torch.uint8))
    for b, rec in enumerate(device.read_pnp_refine_info(info)):
        assert rec.accepted == 0 and rec.lm_steps == 0
        assert rec.count == int((ws.mask[b] != 0).sum())
        assert rec.error == device.read_select(ws.result)[b].best_err


def test_six_items(dev):
    from structure_from_motion_amd import device

    view, _, _ = po.scene(6, seed=500, K=K, outlier_fraction=0.0, noise_px=0.5)
    ws, pts = _pass([view], 4, AGG["rms"], 1, dev, min_extra=0)
    R0, t0, mask_in, err = _inputs(ws, 0)
    model, mask, info = ws.refine(pts, K, THR, AGG["rms"], rounds=1)
    ref = ro.refine(view, R0, t0, K, mask_in, err, THR, AGG["rms"])
    rec = device.read_pnp_refine_info(info)[0]
    assert rec.accepted == ref["accepted"] and rec.count == ref["count"]
    m = model[0].cpu().numpy()
    assert np.max(np.abs(m[:9] - ref["R"].reshape(9))) <= 1e-9
    assert np.array_equal(mask[0].cpu().numpy(), ref["mask"])


def test_six_items_stop_where_the_oracle_stops(dev):
    """With a budget of 50 trial steps, LM on six noisy items ends on its own rules (a small decrease or a small step) long
    before the budget, on the device as in the oracle.  Once the pose has converged, the last bits of the two costs decide
    the relative-decrease test (the device and the oracle differ in summation order), so the two may stop one trial step
    apart in a round, as in test_gpu_tracks.py: the step counts agree to one per round, the poses to the file's 1e-9."""
    from structure_from_motion_amd import device

    view, _, _ = po.scene(6, seed=500, K=K, outlier_fraction=0.0, noise_px=0.5)
    ws, pts = _pass([view], 4, AGG["rms"], 1, dev, min_extra=0)
    R0, t0, mask_in, err = _inputs(ws, 0)
    for rounds in (1, 2):
        model, mask, info = ws.refine(pts, K, THR, AGG["rms"], rounds=rounds, max_steps=50)
        ref = ro.refine(view, R0, t0, K, mask_in, err, THR, AGG["rms"], rounds=rounds, max_steps=50)
        rec = device.read_pnp_refine_info(info)[0]
        print(f"six items, {rounds} round(s): device {rec.lm_steps} trial steps, oracle {ref['lm_steps']}")
        assert 1 <= rec.lm_steps < 50 and 1 <= ref["lm_steps"] < 50, (rec, ref["lm_steps"])
        assert abs(rec.lm_steps - ref["lm_steps"]) <= rounds, (rec, ref["lm_steps"])
        assert rec.accepted == ref["accepted"] and rec.count == ref["count"]
        assert np.max(np.abs(model[0].cpu().numpy()[:9] - ref["R"].reshape(9))) <= 1e-9


def test_view_without_model_is_unchanged(dev):
    from structure_from_motion_amd import device

    view = po.scene(500, seed=600, K=K)[0]
    pts = device.to_device(np.stack([view, view]))
    model_in = device.to_device(np.tile(np.concatenate([np.eye(3).reshape(9), [0.1, 0.2, 0.3]]), (2, 1)))
    mask_in = torch.zeros((2, 500), dtype=torch.uint8, device=dev)
    mask_in[0] = 1
    err = torch.tensor([np.inf, np.inf], dtype=torch.float64, device=dev)
    model, mask, info = device.pnp_refine(pts, model_in, mask_in, err, K, THR, AGG["rms"], 2, 20)
    rec = device.read_pnp_refine_info(info)
    assert rec[1].count == 0 and rec[1].accepted == 0 and rec[1].lm_steps == 0
    assert torch.equal(model[1], model_in[1])
    assert int(mask[1].sum()) == 0


def test_aliased_mask_is_refused(dev):
    from structure_from_motion_amd import _native, device

    lib = _native.load()
    n = 100
    pts = device.to_device(po.scene(n, seed=700, K=K)[0]).reshape(1, n, 5)
    model = device.to_device(np.concatenate([np.eye(3).reshape(9), np.zeros(3)])).reshape(1, 12)
    mask = torch.ones((1, n), dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.float64, device=dev)
    out = torch.empty_like(model)
    info = torch.empty((1, 3), dtype=torch.int64, device=dev)
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    rc = lib.sfm_pnp_refine(pts.data_ptr(), n, 1, C.cast(Kc, C.c_void_p), model.data_ptr(), mask.data_ptr(), err.data_ptr(),
                            THR, 3, 1, 20, out.data_ptr(), mask.data_ptr(), info.data_ptr(), None)
    assert rc == -1 and b"alias" in lib.sfm_last_error()


def test_degenerate_inlier_set_keeps_model(dev):
    from structure_from_motion_amd import device

    n = 300
    view, R, t = po.scene(n, seed=800, K=K, outlier_fraction=0.0, noise_px=0.0)
    view[:, :3] = view[0, :3]
    view[:, 3:] = view[0, 3:] + 0.5   # every item at one 3-D point, 0.7 px off
    e = po.score_values(R, t, K, view)
    model_in = device.to_device(np.concatenate([R.reshape(9), t])).reshape(1, 12)
    err = torch.tensor([ro.aggregate(ro.RMS, n, e)], dtype=torch.float64, device=dev)
    mask_in = torch.ones((1, n), dtype=torch.uint8, device=dev)
    model, mask, info = device.pnp_refine(device.to_device(view).reshape(1, n, 5), model_in, mask_in, err, K, THR, AGG["rms"],
                                          3, 20)
    rec = device.read_pnp_refine_info(info)[0]
    assert rec.accepted == 0 and rec.lm_steps == 0
    assert torch.equal(model, model_in)


def test_ops_opcheck(dev):
    from structure_from_motion_amd import ops

    op = ops.load()
    views = [po.scene(300, seed=900, K=K)[0]]
    ws, pts = _pass(views, 64, AGG["rms"], 2, dev)
    model = ws.model[0, ws.result[:, 1].clamp(min=0)].contiguous()
    err = ws.result[:, 2].contiguous().view(torch.float64)
    Kl = [float(v) for v in K.reshape(9)]
    args = (pts, model, ws.mask, err, Kl, THR, 3, 1, 20)
    torch.library.opcheck(op.pnp_refine.default, args)
    out = (torch.empty_like(model), torch.empty_like(ws.mask), torch.empty((1, 3), dtype=torch.int64, device=dev))
    torch.library.opcheck(op.pnp_refine_.default, args + out, test_utils=("test_schema", "test_faketensor"))


def test_refine_rounds_zero_is_the_unrefined_call(dev):
    from structure_from_motion_amd.pnp import pnp

    view, _, _ = po.scene(400, seed=1000, K=K, outlier_fraction=0.3, noise_px=0.5)
    points = [row[:3].copy() for row in view]
    feats = [Feature(float(row[3]), float(row[4])) for row in view]
    matches = [Match(i, i) for i in range(400)]
    random.seed(4)
    R, t, inl = pnp.estimate_pose_pnp_with_ransac(K, points, feats, matches, THR, max_iterations=200)
    random.seed(4)
    R0, t0, inl0 = pnp.estimate_pose_pnp_with_ransac(K, points, feats, matches, THR, max_iterations=200, refine_rounds=0)
    assert np.array_equal(R, R0) and np.array_equal(t, t0)
    assert [(a[1].x, a[1].y) for a in inl] == [(a[1].x, a[1].y) for a in inl0]
    random.seed(4)
    R1, t1, inl1 = pnp.estimate_pose_pnp_with_ransac(K, points, feats, matches, THR, max_iterations=200, refine_rounds=2)
    pixels = lambda items: [(a[1].x, a[1].y) for a in items]   # noqa: E731
    if not (np.array_equal(R1, R) and np.array_equal(t1, t) and pixels(inl1) == pixels(inl)):
        # a kept round: the inliers under the refined pose, in match order
        e = po.score_values(R1, t1, K, view)
        assert pixels(inl1) == [(feats[i].x, feats[i].y) for i in np.nonzero(e <= THR)[0]]
    # refine_pose_pnp on the refined pose finds nothing more to keep, or only a lower error
    R2, t2, inl2 = pnp.refine_pose_pnp(K, points, feats, matches, R1, t1, THR, rounds=1)
    assert len(inl2) >= len(inl1)


def test_three_view_refined_is_no_worse(dev):
    from apps import sfm_three_view

    # the default gates suit noise-free pixels: at 0.5 px the two-view SED gate of 1.5e-6 leaves no PnP winner
    out = sfm_three_view.run(n=400, seed=11, outlier_fraction=0.3, noise_px=0.5, sed_threshold=6e-6,
                             reprojection_threshold=16.0, refine=2)
    assert out["R3_error_rad"] <= out["R3_error_rad_unrefined"], out
    assert out["pnp_inliers"] >= 0.5 * out["triangulated"], out
