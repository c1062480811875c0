"""The ragged absolute-pose call without a GPU: the checks of ``register_views`` before any device work, the
stable sort by view and the way back to the caller's indices, the gate per view, the oracle's filler rules, the C entry point,
the ops, the app's refusals and the stream case."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import register_views_cases as cases
import register_views_oracle as rv
from structure_from_motion_amd import _native
from structure_from_motion_amd.pnp import registration as reg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = rv.K
SFM_EINVAL = -1   # include/sfm_hip.h


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def _valid():
    points, view, index, pixels = rv.observations(rv.fixture(0, sizes=(5, 0, 7)))
    return dict(camera_matrix=K, points_3d=points, view_indices=view, point_indices=index, pixels=pixels, reprojection_threshold=4.0)


@pytest.mark.parametrize("change", [
    dict(camera_matrix=np.eye(2)),
    dict(camera_matrix=np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 2.0]])),
    dict(points_3d=np.zeros((7, 2))),
    dict(view_indices=np.zeros((12, 1), dtype=np.int64)),
    dict(view_indices=np.zeros(12)),                       # floats
    dict(point_indices=np.zeros(12)),
    dict(point_indices=np.zeros(11, dtype=np.int64)),      # lengths differ
    dict(pixels=np.zeros((12, 3))),
    dict(view_indices=np.full(12, -1)),
    dict(view_indices=np.full(12, 3), num_views=3),
    dict(point_indices=np.full(12, 10**6)),
    dict(point_indices=np.full(12, -1)),
    dict(num_views=-1),
    dict(num_views=2.5),
    dict(reprojection_threshold=0.0),
    dict(reprojection_threshold=float("nan")),
    dict(reprojection_threshold=float("inf")),
    dict(max_iterations=0),
    dict(max_iterations=2.0),
    dict(refine_rounds=-1),
    dict(refine_rounds=True),
    dict(refine_max_steps=-1),
    dict(refine_max_steps=1.5),
    dict(min_extra_fraction=-0.1),
    dict(min_num_extra_inliers=np.zeros(2, dtype=np.int64)),   # one per view means three
    dict(min_num_extra_inliers=1.5),
    dict(max_hypotheses_per_call=0),
    dict(seed=1.5),
])
def test_arguments_are_checked_before_device_work(monkeypatch, change):
    _no_device(monkeypatch)
    args = _valid()
    assert len(args["view_indices"]) == 12
    args.update(change)
    with pytest.raises(ValueError):
        reg.register_views(**args)


def test_no_views_need_no_device(monkeypatch):
    _no_device(monkeypatch)
    out = reg.register_views(K, np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), 4.0)
    assert out.poses.shape == (0, 12) and out.status == [] and out.inliers == [] and len(out.inlier_count) == 0


def test_stable_sort_by_view_and_the_way_back():
    """On a shuffled input, position k of the ragged layout is observation order[k] of the caller: the views in order, each
    view's observations in the caller's order, and a mask over the ragged layout maps back to ascending caller indices."""
    fx = rv.fixture(3)
    _, view, index, pixels = rv.observations(fx, shuffle_seed=9)
    V = len(rv.SIZES)
    order, offset = reg.ragged_order(view, V)
    assert np.array_equal(np.diff(offset), np.bincount(view, minlength=V)) and offset[0] == 0 and offset[-1] == len(view)
    assert sorted(np.diff(offset).tolist()) == sorted(rv.SIZES)
    for v in range(V):
        mine = order[offset[v]:offset[v + 1]]
        assert np.all(view[mine] == v)
        assert np.all(np.diff(mine) > 0)                    # stable: the caller's order inside a view
        assert np.array_equal(mine, np.nonzero(view == v)[0])
    # the gathered items are the view's own
    pts = np.column_stack([fx["points"][index[order]], pixels[order]])
    for v, n in enumerate(np.diff(offset)):
        ref = np.column_stack([fx["points"][fx["views"][v]["index"]], fx["views"][v]["pixels"]])
        got = pts[offset[v]:offset[v + 1]]
        assert sorted(map(tuple, got)) == sorted(map(tuple, ref.reshape(-1, 5)))
    # a mask over the ragged layout -> caller indices, ascending
    mask = np.random.default_rng(1).random(len(view)) < 0.4
    for v in range(V):
        back = np.sort(order[offset[v]:offset[v + 1]][mask[offset[v]:offset[v + 1]]])
        assert np.all(view[back] == v) and np.all(np.diff(back) > 0)
        assert np.array_equal(back, np.nonzero((view == v) & mask[np.argsort(order)])[0])
    # a view nobody observes is empty, wherever it stands
    order, offset = reg.ragged_order(np.array([2, 0, 2]), 4)
    assert order.tolist() == [1, 0, 2] and offset.tolist() == [0, 1, 1, 3, 3]


def test_min_extra_per_view():
    from structure_from_motion_amd.epipolar.view_graph import pair_min_extra

    counts = np.array(rv.SIZES)
    assert np.array_equal(pair_min_extra(counts, 10, 0.0), np.full(len(counts), 10))
    got = pair_min_extra(counts, 10, 0.05)
    assert np.array_equal(got, np.maximum(10, np.floor(0.05 * counts).astype(np.int64)))
    assert got[rv.SIZES.index(1025)] == 51 and got[rv.SIZES.index(40)] == 10
    per_view = np.arange(len(counts))
    assert np.array_equal(pair_min_extra(counts, per_view, 0.0), per_view)
    # the fixture's own gates
    _, offset, min_extra = rv.ragged_arrays(rv.fixture(0))
    assert np.array_equal(np.diff(offset), counts)
    assert min_extra[rv.OUTLIER_VIEW] == rv.OUTLIER_GATE and min_extra[rv.SIZES.index(300)] == 20 and min_extra[2] == 0


def test_oracle_filler_rules():
    assert [rv.status_of(n, -1) for n in (0, 3, 4, 40)] == [rv.TOO_FEW, rv.TOO_FEW, rv.NO_MODEL, rv.NO_MODEL]
    assert rv.status_of(4, 0) == rv.OK and rv.status_of(3, 0) == rv.TOO_FEW
    assert rv.STATUS == _native.REGISTER_STATUS
    f = rv.pass_filler(5)
    assert np.all(f["S"] == -1) and f["S"].shape == (5, 8) and np.isnan(f["model"]).all() and f["model"].shape == (5, 12)
    assert np.all(f["flags"] == _native.FIT_DEGENERATE) and np.all(f["cnt"] == 0) and np.isnan(f["s1"]).all() and np.isnan(f["s2"]).all()
    # such tables select nothing, and every hypothesis is flagged
    assert rv.select(f["cnt"], f["s1"], f["s2"], f["flags"], 0.0) == (-1, np.inf)
    g = rv.no_model_filler(7)
    assert np.isnan(g["pose"]).all() and not g["mask"].any() and not g["mask_out"].any()
    assert (g["error"], g["count"], g["accepted"], g["lm_steps"]) == (np.inf, 0, 0, 0)
    # the mask and seed-mask rules on a hand-made view: item 3 of the sample leaves the seed, the rest of the sample stays
    pts, R, t = rv.po.scene(20, 1, K, 0.0, 0.0)
    model = np.concatenate([R.reshape(9), t])[None]
    S = np.array([[5, 1, 7, 2, 0, 0, 0, 0]], dtype=np.int32)
    pts[9, 3] += 50.0                                        # one outlier
    mask = rv.pnp_mask(pts, model, S, 0)
    assert mask[[5, 1, 7, 2]].tolist() == [2, 2, 2, 2] and mask[9] == 0 and np.count_nonzero(mask == 1) == 15
    assert not rv.pnp_mask(pts, model, S, -1).any()
    seed = rv.seed_mask(mask, S, 0)
    assert seed[2] == 0 and seed[[5, 1, 7]].tolist() == [1, 1, 1] and seed.sum() == 18 and set(np.unique(seed)) <= {0, 1}


def test_entry_point_signature_and_header(native_lib):
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint sfm_register_views\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m is not None
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    sig = _native.SIGNATURES["sfm_register_views"]
    assert len(params) == len(sig) == 27 and params[-1] == "void* stream"

    def ctype_of(p):
        if "*" in p:
            return C.c_void_p
        return {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}[p.split()[0]]
    assert [ctype_of(p) for p in params] == list(sig)
    assert [p.split()[-1].lstrip("*") for p in params[:14]] == ["seed", "seed_stride", "h_begin", "pts", "n_total", "offset", "views",
                                                                 "min_extra", "K", "h_count", "thr", "aggregation", "refine_rounds",
                                                                 "refine_max_steps"]
    for code, name in enumerate(("OK", "NO_MODEL", "TOO_FEW", "BAD_OFFSETS")):
        assert re.search(rf"#define SFM_REGISTER_{name} {code}\b", header)
    assert native_lib.sfm_register_views is not None and native_lib.sfm_abi_version() == 15
    from structure_from_motion_amd import build, device

    assert "sfm_register_views.hip" in build.SOURCES
    assert {"sfm_pnp_pass.h", "sfm_pnp_lm.h"} <= set(build.HEADERS)
    assert (device.REGISTER_OK, device.REGISTER_NO_MODEL, device.REGISTER_TOO_FEW, device.REGISTER_BAD_OFFSETS) == (0, 1, 2, 3)
    assert device.REGISTER_STATUS == ("ok", "no_model", "too_few", "bad_offsets")
    assert hasattr(device.RegisterViewsWorkspace, "buffers") and hasattr(device.RegisterViewsWorkspace, "run")
    assert callable(device.read_register_status)


def test_entry_point_refuses_bad_arguments_before_any_launch(native_lib):
    """Every refusal is an SFM_EINVAL with its reason, checked on the host: no GPU is needed to be refused."""
    lib = native_lib
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    bad_K = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 2)
    p = C.c_void_p(0x1000)   # never dereferenced: the call is refused first

    def call(seed=1, stride=1, h_begin=0, pts=p, n=10, offset=p, views=2, gate=p, Kp=Kc, h=8, thr=4.0, agg=3, rounds=2, steps=20,
             mask=p, mask_out=C.c_void_p(0x2000), status=p):
        return lib.sfm_register_views(seed, stride, h_begin, pts, n, offset, views, gate, Kp, h, thr, agg, rounds, steps, p, p, p, p, p, p,
                                      p, mask, p, mask_out, p, status, None)

    def refused(reason, **kw):
        assert call(**kw) == SFM_EINVAL
        assert reason in lib.sfm_last_error(), (reason, lib.sfm_last_error())
    refused(b"negative size", n=-1)
    refused(b"negative size", views=-1)
    refused(b"negative size", rounds=-1)
    refused(b"negative size", steps=-1)
    refused(b"2^31", n=2**31)
    refused(b"65535", views=65536)
    refused(b"at least one hypothesis", h=0)
    refused(b"one launch covers", h=2**40)
    refused(b"unknown aggregation", agg=4)
    refused(b"unknown aggregation", agg=-1)
    refused(b"row 2", Kp=bad_K)
    refused(b"null camera", Kp=None)
    refused(b"h_begin", h_begin=-1)
    refused(b"null pointer", offset=None)
    refused(b"null pointer", status=None)
    refused(b"null pointer", pts=None)
    refused(b"alias", mask_out=p)
    assert call(views=0) == _native.SFM_OK   # a no-op


def test_ops_are_registered(native_lib):
    import torch

    from structure_from_motion_amd import ops

    op = ops.load()
    assert ops.REGISTER_VIEWS_OPS == ("register_views", "register_views_")
    assert not set(ops.REGISTER_VIEWS_OPS) & set(ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS)
    schema = str(op.register_views.default._schema)
    assert schema == ("sfm_hip::register_views(Tensor pts, Tensor offset, Tensor min_extra, float[] K, int seed, int seed_stride, "
                      "int h_begin, int h, float thr, int aggregation, int refine_rounds, int refine_max_steps) -> "
                      "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    schema = str(op.register_views_.default._schema)
    assert "Tensor(a!) S, Tensor(b!) model" in schema and "Tensor(l!) status) -> ()" in schema and "int h," not in schema
    meta = dict(device="meta")
    V, N, h = 5, 700, 33
    pts, offset = torch.empty((N, 5), dtype=torch.float64, **meta), torch.empty((V + 1,), dtype=torch.int64, **meta)
    gate = torch.empty((V,), dtype=torch.float64, **meta)
    Kl = [float(v) for v in K.reshape(9)]
    pose, mask_out, info, status, mask, result = op.register_views(pts, offset, gate, Kl, 1, 1, 0, h, 4.0, 3, 2, 20)
    assert pose.shape == (V, 12) and pose.dtype == torch.float64 and pose.device.type == "meta"
    assert mask_out.shape == (N,) == mask.shape and mask.dtype == torch.uint8 == mask_out.dtype
    assert info.shape == (V, 3) and info.dtype == torch.int64 and status.shape == (V,) and status.dtype == torch.int32
    assert result.shape == (V, 5) and result.dtype == torch.int64


def test_app_refuses_dlt_and_unknown_routes_before_any_work(monkeypatch):
    from apps import sfm_multi_view as app
    from structure_from_motion_amd import synthetic

    def no_work(*args, **kwargs):
        raise AssertionError("work started")
    monkeypatch.setattr(synthetic, "multi_view_scene", no_work)
    _no_device(monkeypatch)
    assert "batched" in app.REGISTER_ROUTES
    with pytest.raises(ValueError, match="P3P"):
        app.run(views=8, register="batched", pnp_solver="dlt")
    with pytest.raises(ValueError, match="register must be one of"):
        app.run(views=8, register="ragged")
    # unset, the solver follows the route: the batched one gets as far as the scene, and so does the default
    for kw in (dict(register="batched"), dict(register="batched", pnp_solver="p3p"), dict()):
        with pytest.raises(AssertionError, match="work started"):
            app.run(views=8, **kw)
    script = os.path.join(REPO, "apps", "sfm_multi_view.py")
    for argv, reason in ((["--register", "batched", "--pnp-solver", "dlt"], "P3P"), (["--register", "ragged"], "invalid choice")):
        done = subprocess.run([sys.executable, script] + argv, capture_output=True, text=True)
        assert done.returncode == 2 and reason in done.stderr, (argv, done.stderr)


def test_stream_case_is_registered():
    assert cases.stream_cases.CASES["register_views"].entries == ("sfm_register_views",)
    assert "sfm_register_views" in cases.stream_cases.covered_entries()
    assert not cases.stream_cases.CASES["register_views"].synchronising


def test_drop_in_path():
    import lib.pnp.registration as drop_in

    assert drop_in.register_views is reg.register_views and drop_in.ViewRegistrations is reg.ViewRegistrations
    assert reg.ViewRegistrations._fields == ("poses", "status", "inlier_count", "inliers", "ransac_count", "error", "accepted", "lm_steps")
