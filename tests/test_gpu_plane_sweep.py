"""sfm_plane_sweep and sfm_filter_depth_maps on the GPU against their NumPy definition (tests/plane_sweep_oracle.py), byte for
byte, a NaN equal to any NaN: the definition uses only correctly rounded float64 operations in a fixed order.
The shapes are the smallest at which the kernels can go wrong: ragged tiles, every radius, every source and depth count that takes
another path, invalid geometry, invalid hypotheses and bad references."""
import numpy as np
import pytest

import plane_sweep_cases as cases   # registers the stream case of the two entry points (tests/test_gpu_streams.py runs it)
import plane_sweep_oracle as po

pytestmark = pytest.mark.gpu

SWEEP, FILTER = cases.SWEEP_NAMES, cases.FILTER_NAMES
POISON_F, POISON_I = 12345.0, 77   # what the outputs hold before a call: every element must be written


def _device():
    import torch

    from structure_from_motion_amd import device

    return torch, device


def _upload(inp):
    torch, device = _device()
    dtypes = dict(images=torch.uint8, refs=torch.int32, sources=torch.int32)
    return {k: device.to_device(np.ascontiguousarray(v), dtypes.get(k, torch.float64)) for k, v in inp.items()}


def run_sweep(inp, radius, top_k=0, min_sources=1, min_variance=1.0, volume=True, calls=1):
    torch, device = _device()
    t = _upload(inp)
    (V, H, W), R, D = inp["images"].shape, len(inp["refs"]), inp["depths"].shape[1]
    ws = device.PlaneSweepWorkspace(R, H, W, D, volume=volume)
    for _ in range(calls):
        for buf in ws.buffers():
            if buf is not None:
                buf.fill_(POISON_F if buf.dtype == torch.float64 else POISON_I)
        ws.run(t["images"], t["K"], t["poses"], t["refs"], t["sources"], t["depths"], radius, top_k, min_sources, min_variance)
    return {name: None if buf is None else buf.cpu().numpy() for name, buf in zip(SWEEP, ws.buffers())}


def want_sweep(inp, radius, top_k=0, min_sources=1, min_variance=1.0):
    return po.plane_sweep(inp["images"], inp["K"], inp["poses"], inp["refs"], inp["sources"], inp["depths"], radius, top_k, min_sources,
                          min_variance)


def assert_same(got, want, names, what=""):
    for name in names:
        if got[name] is None:
            continue
        assert po.same_bytes(got[name], want[name]), f"{what}: {name} differs from the definition in " \
                                                     f"{int(np.sum(~_equal(got[name], want[name])))} of {want[name].size} elements"


def _equal(a, b):
    if a.dtype.kind != "f":
        return a == b
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))


def check_sweep(inp, radius, **kw):
    got, want = run_sweep(inp, radius, **kw), want_sweep(inp, radius, **kw)
    assert_same(got, want, SWEEP, f"radius {radius} {kw}")
    return got, want


# ---- tiles and radii -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 45), (16, 16), (17, 33)])
def test_tile_edges(shape):
    inp = cases.sweep_inputs(cases.scene(*shape, views=3, seed=4), 5, 2)
    got, want = check_sweep(inp, 2)
    assert (want["index"] >= 0).mean() > 0.5   # the comparison is about winners, not about fillers


@pytest.mark.parametrize("radius,shape", [(1, (20, 23)), (3, (20, 23)), (4, (18, 19)), (5, (12, 12)), (5, (29, 27))])
def test_every_radius(radius, shape):
    inp = cases.sweep_inputs(cases.scene(*shape, views=3, seed=5), 4, 2)
    if shape == (12, 12):
        # the smallest image radius 5 allows has one pixel whose window avoids the last row and column, where no sample is valid: it
        # has a winner only under the identity warp, which two equal poses and a camera of powers of two give exactly
        image = np.random.default_rng(5).integers(0, 256, size=(12, 12)).astype(np.uint8)
        inp.update(images=np.stack([image] * 3), K=cases.exact_camera().reshape(9), poses=np.stack([cases.pose()] * 3))
    got, want = check_sweep(inp, radius)
    assert (want["index"] >= 0).any()
    if shape == (12, 12):
        assert np.array_equal(np.argwhere(want["index"][0] >= 0), [[5, 5]]) and want["cost"][0, 5, 5] == 0.0


# ---- sources, depths, aggregation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sources", [
    [[1], [0], [3], [-1]],                                                       # S = 1, and a reference without any source
    [[-1, 1, 0], [1, 2, 0], [9, 2, 3], [3, 3, 3]],                               # -1, the reference itself, a slot beyond the views
    [[1, 2, 3, 1, 2, 3, -1, 0], [0] * 8, [3, 1, 0, -1, -1, -1, -1, 4], [2, 1, 0, 2, 1, 0, 2, 1]],   # S = 8, repeated sources
])
def test_source_lists(sources):
    inp = cases.sweep_inputs(cases.scene(20, 23, views=4, seed=6), 3, 1)
    inp["sources"] = np.array(sources, dtype=np.int32)
    check_sweep(inp, 2)
    check_sweep(inp, 2, top_k=2, min_sources=2)


@pytest.mark.parametrize("count", [1, 2, 3, 33])
def test_depth_counts(count):
    inp = cases.sweep_inputs(cases.scene(20, 23, views=3, seed=7), count, 2)
    got, want = check_sweep(inp, 2)
    if count == 33:   # winners at both ends, in the middle, with and without the parabola step
        assert {0, 32} <= set(np.unique(want["index"])) and (want["depth"] != inp["depths"][0][np.clip(want["index"], 0, 32)]).any()


def test_duplicated_and_unordered_hypotheses():
    """A hypothesis repeated after the winner gives c+ == c0 (den is then c- - c0 > 0: den == 0 cannot be reached, as an equal cost
    before the winner would have won); repeated before it, the lower index wins and has no valid step on that side."""
    inp = cases.sweep_inputs(cases.scene(20, 23, views=3, seed=7), 5, 2)
    z = inp["depths"][0]
    inp["depths"] = np.ascontiguousarray(np.stack([[z[0], z[2], z[2], z[2], z[4]], [z[4], z[3], z[3], z[1], z[0]], [z[2]] * 5]))
    got, want = check_sweep(inp, 2)
    assert not np.any(want["index"][0] == 2) and not np.any(want["index"][0] == 3) and set(np.unique(want["index"][2])) <= {-1, 0}


@pytest.mark.parametrize("top_k", [0, 1, 2])
@pytest.mark.parametrize("min_sources", [1, 2])
def test_aggregation(top_k, min_sources):
    inp = cases.sweep_inputs(cases.scene(20, 23, views=4, seed=8), 3, 3)
    check_sweep(inp, 2, top_k=top_k, min_sources=min_sources)


# ---- invalid geometry and hypotheses -------------------------------------------------------------------------------------------------
def test_invalid_geometry():
    """Source 2 looks away (Wd <= 0 everywhere), source 3 stands far to the side (its warp leaves the image for a part of every
    tile row), and a flat block of the reference fails the variance gate."""
    sc = cases.scene(37, 45, views=4, seed=9)
    inp = cases.sweep_inputs(sc, 4, 3, refs=[0])
    images, poses = inp["images"].copy(), inp["poses"].copy()
    images[0, 10:24, 12:30] = 90
    away = np.diag([-1.0, 1.0, -1.0])
    poses[2] = cases.pose(away @ poses[2, :9].reshape(3, 3), away @ poses[2, 9:])
    poses[3, 9] += 0.35
    inp.update(images=images, poses=poses, sources=np.array([[1, 2, 3]], dtype=np.int32))
    got, want = check_sweep(inp, 2)
    alone = dict(inp, sources=np.array([[2, -1, -1]], dtype=np.int32))
    assert np.all(want_sweep(alone, 2)["index"] == -1)                        # the source that looks away scores nowhere
    side = want_sweep(dict(inp, sources=np.array([[3, -1, -1]], dtype=np.int32)), 2)["index"][0]
    assert (side[2:-2, 2:-2] >= 0).any() and (side[2:-2, 2:-2] < 0).any()      # the far one scores in a part of the image
    assert np.all(want["index"][0, 12:22, 14:28] == -1) and (want["index"][0] >= 0).any()   # the flat block has no winner
    check_sweep(inp, 2, min_variance=0.0)
    check_sweep(alone, 2)


def test_invalid_hypotheses():
    inp = cases.sweep_inputs(cases.scene(20, 23, views=3, seed=10), 6, 2)
    z = inp["depths"][0]
    inp["depths"] = np.ascontiguousarray(np.stack([[z[0], -z[1], np.nan, z[3], np.inf, 0.0], [np.nan] * 6, [-1.0, z[2], z[3], z[4], np.nan, z[5]]]))
    got, want = check_sweep(inp, 2)
    assert np.all(np.isnan(want["volume"][0, [1, 2, 4, 5]])) and np.all(want["index"][1] == -1)
    assert set(np.unique(want["index"][0])) <= {-1, 0, 3}


# ---- references, chunks, repeated calls -----------------------------------------------------------------------------------------------
def _three_references():
    sc = cases.scene(20, 23, views=4, seed=11)
    inp = cases.sweep_inputs(sc, 4, 2, refs=[1, 7, 0])
    inp["depths"] = np.ascontiguousarray(np.stack([cases.hypotheses(sc, 4), cases.hypotheses(sc, 7)[1:5], cases.hypotheses(sc, 4)[::-1]]))
    return inp


def test_three_references_one_of_them_bad():
    inp = _three_references()
    got, want = check_sweep(inp, 2)
    assert got["status"].tolist() == [cases.OK, cases.BAD_REFERENCE, cases.OK]
    assert np.all(got["index"][1] == -1) and np.all(np.isnan(got["depth"][1])) and np.all(np.isnan(got["volume"][1]))
    inp["refs"] = np.array([-1, 3, 4], dtype=np.int32)
    check_sweep(inp, 2)


def test_without_a_volume_twice_and_in_chunks():
    inp = _three_references()
    want = want_sweep(inp, 2)
    assert_same(run_sweep(inp, 2, volume=False), want, SWEEP, "volume NULL")
    assert_same(run_sweep(inp, 2, calls=2), want, SWEEP, "second call")
    for bounds in ([(0, 1), (1, 3)], [(0, 2), (2, 3)], [(0, 1), (1, 2), (2, 3)]):
        parts = [run_sweep({k: (v[a:b] if k in ("refs", "sources", "depths") else v) for k, v in inp.items()}, 2) for a, b in bounds]
        joined = {name: np.concatenate([p[name] for p in parts]) for name in SWEEP}
        assert_same(joined, want, SWEEP, f"chunks {bounds}")


def test_the_python_layer_matches_the_definition():
    from structure_from_motion_amd.stereo import depth_maps as dm

    sc = cases.scene(37, 45, views=4, seed=12, two_planes=True)
    z = cases.hypotheses(sc, 9)
    sources = cases.nearest_sources(4, 3)
    maps = dm.compute_depth_maps(sc["images"], sc["K"], sc["poses"], z, sources=sources, radius=2, top_k=2, return_volume=True,
                                 max_refs_per_call=3)
    want = po.plane_sweep(sc["images"], sc["K"], sc["poses"], np.arange(4), sources, np.broadcast_to(z, (4, 9)), 2, top_k=2)
    assert_same(dict(depth=maps.depth, index=maps.index, cost=maps.cost, volume=maps.volume), want, ("depth", "index", "cost", "volume"))
    kept = dm.filter_depth_maps(maps, sc["K"], sc["poses"], sources, 1.0, 0.02, 2)
    expect = po.filter_depth_maps(want["depth"], sc["K"], sc["poses"], np.arange(4), sources, 1.0, 0.02, 2)
    assert_same(dict(count=kept.count, filtered=kept.depth, points=kept.points), expect, ("count", "filtered", "points"))
    points, grey, view = dm.point_cloud(kept)
    assert len(points) == np.isfinite(expect["filtered"]).sum() > 0 and grey.dtype == np.uint8 and set(view) <= {0, 1, 2, 3}
    assert np.array_equal(grey, sc["images"][np.isfinite(expect["filtered"])])


def test_opcheck():
    torch, device = _device()
    from structure_from_motion_amd import ops

    op = ops.load()
    t = _upload(cases.sweep_inputs(cases.scene(16, 17, views=3, seed=13), 3, 2))
    args = (t["images"], t["K"], t["poses"], t["refs"], t["sources"], t["depths"])
    # not test_aot_dispatch_dynamic: it compares the eager and the traced outputs with assert_close, under which the NaNs that
    # every depth map holds along its border differ from themselves
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    for volume in (False, True):
        torch.library.opcheck(op.plane_sweep.default, args + (2, 0, 1, 1.0, volume), test_utils=tests)
    depth, index, cost, status, volume = op.plane_sweep(*args, 2, 0, 1, 1.0, True)
    torch.library.opcheck(op.filter_depth_maps.default, (depth, t["K"], t["poses"], t["refs"], t["sources"], 1.0, 0.05, 1), test_utils=tests)
    ws = device.PlaneSweepWorkspace(3, 16, 17, 3, volume=True)
    torch.library.opcheck(op.plane_sweep_.default, args + (2, 0, 1, 1.0) + ws.buffers(), test_utils=tests)
    ws.run(*args, 2, 0, 1, 1.0)
    for got, name in zip((depth, index, cost, status, volume), SWEEP):   # the functional and the in-place form agree
        assert po.same_bytes(got.cpu().numpy(), getattr(ws, name).cpu().numpy()), name


# ---- the filter ----------------------------------------------------------------------------------------------------------------------
def run_filter(depth, K, poses, refs, sources, *scalars):
    torch, device = _device()
    R, (V, H, W) = len(refs), depth.shape
    out = (torch.full((R, H, W), POISON_I, dtype=torch.int32, device="cuda"), torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"),
           torch.full((R, H, W, 3), POISON_F, dtype=torch.float64, device="cuda"), torch.full((R,), POISON_I, dtype=torch.int32, device="cuda"))
    device.filter_depth_maps(device.to_device(depth), device.to_device(np.ascontiguousarray(np.reshape(K, 9))), device.to_device(poses),
                             device.to_device(refs, torch.int32), device.to_device(sources, torch.int32), *scalars, out=out)
    return {name: buf.cpu().numpy() for name, buf in zip(FILTER, out)}


@pytest.mark.parametrize("min_consistent", [1, 3])
def test_filter_with_holes_and_a_source_behind_the_camera(min_consistent):
    sc = cases.scene(37, 45, views=4, seed=12, two_planes=True)
    z = cases.hypotheses(sc, 9)
    depth = po.plane_sweep(sc["images"], sc["K"], sc["poses"], np.arange(4), cases.nearest_sources(4, 3), np.broadcast_to(z, (4, 9)), 2)["depth"]
    depth[0, 5:9, 7:30] = np.nan
    depth[2, ::3, ::4] = np.nan
    poses = sc["poses"].copy()
    away = np.diag([-1.0, 1.0, -1.0])
    poses[3] = cases.pose(away @ poses[3, :9].reshape(3, 3), away @ poses[3, 9:])   # view 3 looks away: z_s <= 0 for every point
    refs = np.array([0, 1, 5, 2, 3], dtype=np.int32)
    sources = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 2], [-1, 1, 2], [0, 1, 7]], dtype=np.int32)
    args = (depth, sc["K"], poses, refs, sources, 1.0, 0.05, min_consistent)
    got, want = run_filter(*args), po.filter_depth_maps(*args)
    assert_same(got, want, FILTER, f"min_consistent {min_consistent}")
    assert want["status"].tolist() == [0, 0, 1, 0, 0] and want["count"][0].max() == 2 and want["count"][4].max() == 0
    assert np.isfinite(want["filtered"]).any() == (min_consistent == 1)


def test_filter_on_the_exact_boundary():
    case = cases.filter_boundary_case()
    args = (case["depth"], case["K"], case["poses"], case["refs"], case["sources"])
    for scalars in ((8.0, 0.5, 1), (float(np.nextafter(8.0, 0.0)), 0.5, 1), (8.0, float(np.nextafter(0.5, 0.0)), 1), (8.0, 0.5, 0)):
        got, want = run_filter(*args, *scalars), po.filter_depth_maps(*args, *scalars)
        assert_same(got, want, FILTER, f"{scalars}")
    got = run_filter(*args, 8.0, 0.5, 1)
    assert got["count"][0][case["on_boundary"]] == 1 and got["count"][0][case["beyond"]] == 0 and got["count"][0][case["hole"]] == 0


# ---- refused calls leave their outputs untouched -----------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    torch, device = _device()
    from structure_from_motion_amd import _native

    lib = _native.load()
    inp = cases.sweep_inputs(cases.scene(16, 17, views=3, seed=13), 3, 2)
    t = _upload(inp)
    V, H, W, R, S, D = 3, 16, 17, 3, 2, 3
    out = dict(depth=torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"), index=torch.full((R, H, W), POISON_I, dtype=torch.int32, device="cuda"),
               cost=torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"), status=torch.full((R,), POISON_I, dtype=torch.int32, device="cuda"),
               volume=torch.full((R, D, H, W), POISON_F, dtype=torch.float64, device="cuda"),
               count=torch.full((R, H, W), POISON_I, dtype=torch.int32, device="cuda"), filtered=torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"),
               points=torch.full((R, H, W, 3), POISON_F, dtype=torch.float64, device="cuda"), fstatus=torch.full((R,), POISON_I, dtype=torch.int32, device="cuda"))
    ws = torch.zeros(lib.sfm_plane_sweep_workspace_bytes(V, H, W, R, S, D) + 64, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in out.items()}
    p = {k: v.data_ptr() for k, v in {**t, **out}.items()}

    def sweep(**change):
        a = dict(images=p["images"], V=V, H=H, W=W, K=p["K"], poses=p["poses"], refs=p["refs"], R=R, sources=p["sources"], S=S, depths=p["depths"],
                 D=D, radius=2, top_k=0, min_sources=1, min_variance=1.0, depth=p["depth"], index=p["index"], cost=p["cost"], status=p["status"],
                 volume=p["volume"], ws=ws.data_ptr(), ws_bytes=ws.numel() - 64)
        a.update(change)
        return lib.sfm_plane_sweep(*a.values(), None)

    def keep(**change):
        a = dict(depth=p["depth"], V=V, H=H, W=W, K=p["K"], poses=p["poses"], refs=p["refs"], R=R, sources=p["sources"], S=S, mpe=1.0, rel=0.01,
                 mc=1, count=p["count"], filtered=p["filtered"], points=p["points"], status=p["fstatus"])
        a.update(change)
        return lib.sfm_filter_depth_maps(*a.values(), None)

    refused = [sweep(radius=0), sweep(radius=6), sweep(radius=5, H=11), sweep(H=5), sweep(W=5), sweep(V=0), sweep(S=0), sweep(S=9), sweep(D=0),
               sweep(D=4097), sweep(R=65536), sweep(R=-1), sweep(H=2**16, W=2**15), sweep(top_k=-1), sweep(min_sources=0),
               sweep(min_variance=-1.0), sweep(min_variance=float("nan")), sweep(min_variance=float("inf")), sweep(images=None), sweep(K=None),
               sweep(poses=None), sweep(refs=None), sweep(sources=None), sweep(depths=None), sweep(depth=None), sweep(index=None), sweep(cost=None),
               sweep(status=None), sweep(ws=None), sweep(depth=p["depth"] + 4), sweep(volume=p["volume"] + 4), sweep(index=p["index"] + 2),
               sweep(K=p["K"] + 1), sweep(ws=ws.data_ptr() + 8), sweep(ws_bytes=ws.numel() - 64 - 1), sweep(ws_bytes=0),
               keep(V=0), keep(H=0), keep(S=0), keep(S=9), keep(R=65536), keep(R=-1), keep(H=2**16, W=2**15), keep(mpe=-1.0),
               keep(mpe=float("nan")), keep(rel=-0.5), keep(rel=float("inf")), keep(mc=-1), keep(depth=None), keep(K=None), keep(poses=None),
               keep(refs=None), keep(sources=None), keep(count=None), keep(filtered=None), keep(points=None), keep(status=None),
               keep(filtered=p["filtered"] + 4), keep(count=p["count"] + 1), keep(poses=p["poses"] + 2)]
    assert all(rc == -1 for rc in refused), refused
    assert b"sfm_filter_depth_maps" in lib.sfm_last_error()
    assert sweep(R=0) == 0 and keep(R=0) == 0   # no reference: a no-op
    torch.cuda.synchronize()
    for name, tensor in out.items():
        assert torch.equal(tensor, before[name]), name
    assert sweep() == 0 and keep() == 0   # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in SWEEP}
    assert_same(got, want_sweep(inp, 2), SWEEP, "the C entry point")
