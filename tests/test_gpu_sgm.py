"""sfm_sgm_aggregate on the GPU against its NumPy definition (tests/sgm_oracle.py), byte for byte, a NaN equal to any NaN: the
definition uses only correctly rounded float64 operations and exact minima in a fixed order.  The shapes are the
smallest at which the kernels can go wrong: images narrower and wider than the 16 paths of a block and the tiles of the
horizontal kernel, the first and last depth count of every depth-group kernel, every kind of invalid entry."""
import numpy as np
import pytest

import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_cases as cases   # registers the stream case of the entry point (tests/test_gpu_streams.py runs it)
import sgm_oracle as so

pytestmark = pytest.mark.gpu

NAMES = cases.NAMES
POISON_F, POISON_I = 12345.0, 77   # what the outputs hold before a call: every element must be written


def _device():
    import torch

    from structure_from_motion_amd import device

    return torch, device


def run_sgm(volume, depths, p1=0.1, p2=0.8, invalid_cost=1.0, paths=8, aggregated=True, calls=1):
    torch, device = _device()
    R, D, H, W = volume.shape
    ws = device.SgmWorkspace(R, H, W, D, aggregated=aggregated)
    v, z = device.to_device(np.ascontiguousarray(volume)), device.to_device(np.ascontiguousarray(depths))
    for _ in range(calls):
        for buf in ws.buffers():
            if buf is not None:
                buf.fill_(POISON_F if buf.dtype == torch.float64 else POISON_I)
        ws.run(v, z, p1, p2, invalid_cost, paths)
    return {name: None if buf is None else buf.cpu().numpy() for name, buf in zip(NAMES, ws.buffers())}


def assert_same(got, want, what=""):
    for name in NAMES:
        if got.get(name) is None:
            continue
        a, b = got[name], want[name]
        equal = (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64)) if a.dtype.kind == "f" else a == b
        assert po.same_bytes(a, b), f"{what}: {name} differs from the definition in {int(np.sum(~equal))} of {b.size} elements, first at " \
                                    f"{tuple(np.argwhere(~equal)[0]) if a.shape == b.shape else (a.shape, b.shape)}"


def check(volume, depths, **kw):
    run_kw = {k: kw.pop(k) for k in ("aggregated", "calls") if k in kw}
    got, want = run_sgm(volume, depths, **kw, **run_kw), so.sgm_aggregate(volume, depths, **kw)
    assert_same(got, want, f"{volume.shape} {kw}")
    return got, want


# ---- image sizes and depth counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 6), (16, 16), (17, 19), (37, 45)])
@pytest.mark.parametrize("paths", [4, 8])
def test_image_sizes(shape, paths):
    volume, depths = cases.random_volume((2, 5) + shape, 40 + shape[0])
    got, want = check(volume, depths, paths=paths)
    assert (want["index"] >= 0).any()


@pytest.mark.parametrize("count", [1, 2, 3, 16, 17, 33, 65])
def test_depth_counts(count):
    volume, depths = cases.random_volume((2, count, 9, 21), 50 + count)
    for paths in (4, 8):
        got, want = check(volume, depths, paths=paths)
    if count >= 16:   # winners at both ends and in between, with and without the parabola step
        assert {0, count - 1} <= set(np.unique(want["index"])) and (want["depth"] != depths[0][np.clip(want["index"], 0, count - 1)]).any()


@pytest.mark.parametrize("count", sorted({1, cases.MAX_DEPTHS} | {16 * g for g in cases.DEPTH_GROUPS} | {16 * g + 1 for g in cases.DEPTH_GROUPS[:-1]}))
def test_first_and_last_depth_count_of_every_kernel(count):
    volume, depths = cases.random_volume((1, count, 3, 18), 60 + count)
    check(volume, depths, paths=8)


@pytest.mark.parametrize("paths", [4, 8])
def test_the_winner_rule_on_hand_made_columns(paths):
    """One crafted column of 5 hypotheses per reference on a 1 x 1 image, where every path restarts and the winner kernel sees
    paths times the column (tests/sgm_cases.py): every branch of the rule, against the definition and against the table."""
    volume, depths, (index, depth, cost) = cases.winner_columns()
    got, want = check(volume, depths, paths=paths)
    assert po.same_bytes(got["index"][:, 0, 0], index) and po.same_bytes(got["depth"][:, 0, 0], depth)
    assert po.same_bytes(got["cost"][:, 0, 0], paths * cost)


# ---- settings ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p1,p2,invalid_cost", [(0.0, 0.8, 1.0), (0.5, 0.5, 1.0), (0.0, 0.0, 1.0), (0.1, 0.8, 0.0), (0.1, 0.8, 2.0)])
def test_penalties_and_invalid_cost(p1, p2, invalid_cost):
    volume, depths = cases.random_volume((2, 7, 11, 19), 70)
    for paths in (4, 8):
        check(volume, depths, p1=p1, p2=p2, invalid_cost=invalid_cost, paths=paths)


# ---- volumes -------------------------------------------------------------------------------------------------------------------------
def test_nan_pixels_a_nan_reference_and_infinite_entries():
    volume, depths = cases.random_volume((3, 6, 10, 21), 71)
    volume[0, :, 3:5, 2:19] = np.nan            # whole pixels without a cost
    volume[1] = np.nan                          # what the sweep writes for a bad reference
    volume[2, 1, ::2, ::3], volume[2, 4, 1::3, ::2] = np.inf, -np.inf
    got, want = check(volume, depths)
    assert np.all(got["index"][1] == -1) and np.all(np.isnan(got["depth"][1])) and np.all(np.isnan(got["cost"][1]))
    assert np.all(got["index"][0, 3:5, 2:19] == -1) and np.all(np.isfinite(got["aggregated"]))
    assert not np.any(got["index"][2, ::2, ::3] == 1) and (got["index"][2] == 1).any()


def test_invalid_and_duplicated_depths():
    volume, _ = cases.random_volume((3, 6, 10, 21), 72, nan_share=0.1)
    volume[:, 2] = volume[:, 2] * 0.01          # the lowest sums lie at d = 2 ...
    z = np.array([[2.0, 3.0, -4.0, 5.0, np.inf, 0.0], [np.nan] * 6, [3.0, 3.0, 3.0, 2.0, 2.0, 4.0]])   # ... which reference 0 cannot choose
    got, want = check(volume, z)
    assert set(np.unique(got["index"][0])) <= {-1, 0, 1, 3} and np.all(got["index"][1] == -1) and (got["index"][2] == 2).any()


def test_a_constant_volume():
    got, _ = check(np.full((1, 20, 6, 23), 0.25), np.linspace(2.0, 6.0, 20)[None])
    assert np.all(got["index"] == 0)


def test_the_volume_of_a_real_sweep():
    volume, depths = cases.sweep_volume()
    for paths in (4, 8):
        got, want = check(volume, depths, paths=paths)
    assert (want["index"] >= 0).mean() > 0.5 and np.isnan(volume).any()


# ---- outputs, workspace, repeated calls ----------------------------------------------------------------------------------------------
def _c_call(lib, volume_t, depths_t, buffers, workspace, keep=True, /, **change):
    """sfm_sgm_aggregate on device tensors, 8 paths; ``change`` replaces arguments by the names of the dict below."""
    R, D, H, W = volume_t.shape
    a = dict(volume=volume_t.data_ptr(), R=R, D=D, H=H, W=W, depths=depths_t.data_ptr(), p1=0.1, p2=0.8, invalid=1.0, paths=8,
             depth=buffers["depth"].data_ptr(), index=buffers["index"].data_ptr(), cost=buffers["cost"].data_ptr(),
             aggregated=buffers["aggregated"].data_ptr() if keep else None, ws=workspace.data_ptr(), ws_bytes=workspace.numel())
    a.update(change)
    return lib.sfm_sgm_aggregate(*a.values(), None)


def _poisoned(shape):
    torch, _ = _device()
    R, D, H, W = shape
    return dict(depth=torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"), index=torch.full((R, H, W), POISON_I, dtype=torch.int32, device="cuda"),
                cost=torch.full((R, H, W), POISON_F, dtype=torch.float64, device="cuda"),
                aggregated=torch.full((R, D, H, W), POISON_F, dtype=torch.float64, device="cuda"))


def test_without_aggregated_with_a_poisoned_workspace_and_twice():
    torch, device = _device()
    from structure_from_motion_amd import _native

    lib = _native.load()
    volume, depths = cases.random_volume((2, 19, 9, 21), 73)
    want = so.sgm_aggregate(volume, depths)
    assert_same(run_sgm(volume, depths, aggregated=False), want, "aggregated NULL")
    assert_same(run_sgm(volume, depths, calls=2), want, "second call")
    v, z = device.to_device(volume), device.to_device(depths)
    out = _poisoned(volume.shape)
    nbytes = lib.sfm_sgm_workspace_bytes(2, 19, 9, 21, 0)
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")   # a NaN left in the sum would spread
    assert _c_call(lib, v, z, out, ws.view(torch.uint8), False) == 0
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in out.items()}
    assert np.all(got.pop("aggregated") == POISON_F)   # not given: not touched
    assert_same(got, want, "the C entry point, aggregated NULL")
    assert po.same_bytes(ws[:volume.size].cpu().numpy().reshape(volume.shape), want["aggregated"])   # the workspace held the sum


def test_no_reference_is_a_no_op():
    got = run_sgm(np.zeros((0, 5, 4, 6)), np.zeros((0, 5)))
    assert got["depth"].shape == (0, 4, 6) and got["aggregated"].shape == (0, 5, 4, 6)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_every_chunk_split_of_regularize_depth_maps():
    from structure_from_motion_amd.stereo import depth_maps as dm

    volume, depths = cases.sweep_volume()
    want = so.sgm_aggregate(volume, depths, 0.2, 0.6, 0.9, 4)
    for per_call in (1, 2, 3, 4, 64):
        maps = dm.regularize_depth_maps(volume, depths, 0.2, 0.6, 0.9, 4, return_aggregated=True, max_refs_per_call=per_call)
        assert_same(dict(depth=maps.depth, index=maps.index, cost=maps.cost, aggregated=maps.volume), want, f"{per_call} references a call")
    maps = dm.regularize_depth_maps(volume[:, :, :5], depths[0], 0.2, 0.6, 0.9, 4)   # (D,) hypotheses, no aggregated volume
    assert maps.volume is None and po.same_bytes(maps.index, so.sgm_aggregate(volume[:, :, :5], depths, 0.2, 0.6, 0.9, 4)["index"])


def test_compute_depth_maps_with_and_without_smoothness():
    from structure_from_motion_amd.stereo import depth_maps as dm

    sc = sweep_cases.scene(37, 45, views=4, seed=12, two_planes=True)
    z = sweep_cases.hypotheses(sc, 9)
    sources = sweep_cases.nearest_sources(4, 3)
    args = (sc["images"], sc["K"], sc["poses"], z)
    kw = dict(sources=sources, radius=2, top_k=2, max_refs_per_call=3)
    plain = dm.compute_depth_maps(*args, return_volume=True, **kw)
    want = po.plane_sweep(sc["images"], sc["K"], sc["poses"], np.arange(4), sources, np.broadcast_to(z, (4, 9)), 2, top_k=2)
    for name in ("depth", "index", "cost", "volume"):   # smoothness=None: today's result
        assert po.same_bytes(getattr(plain, name), want[name]), name
        assert po.same_bytes(getattr(dm.compute_depth_maps(*args, return_volume=True, smoothness=None, **kw), name), want[name]), name
    smooth = dm.regularize_depth_maps(plain, z, 0.1, 0.8)
    assert_same(dict(depth=smooth.depth, index=smooth.index, cost=smooth.cost), so.sgm_aggregate(want["volume"], z, 0.1, 0.8, 1.0, 8), "regularize")
    assert np.array_equal(smooth.refs, plain.refs) and smooth.images is plain.images and smooth.volume is None
    for return_volume in (False, True):
        fused = dm.compute_depth_maps(*args, return_volume=return_volume, smoothness=(0.1, 0.8), **kw)
        for name in ("depth", "index", "cost"):
            assert po.same_bytes(getattr(fused, name), getattr(smooth, name)), name
        assert fused.volume is None if not return_volume else po.same_bytes(fused.volume, want["volume"])
    assert not np.array_equal(smooth.index, plain.index)


# ---- refused calls leave their outputs untouched -----------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    torch, device = _device()
    from structure_from_motion_amd import _native

    lib = _native.load()
    volume, depths = cases.random_volume((2, 5, 6, 17), 74)
    v, z = device.to_device(volume), device.to_device(depths)
    out = _poisoned(volume.shape)
    before = {k: t.clone() for k, t in out.items()}
    ws = torch.zeros(lib.sfm_sgm_workspace_bytes(2, 5, 6, 17, 0) + 64, dtype=torch.uint8, device="cuda")
    need = ws.numel() - 64

    def call(keep=True, /, **change):
        return _c_call(lib, v, z, out, ws, keep, **{"ws_bytes": need, **change})

    nan, inf = float("nan"), float("inf")
    refused = [call(R=-1), call(R=65536), call(D=0), call(D=257), call(H=0), call(W=0), call(H=2**16, W=2**15), call(paths=0), call(paths=6),
               call(paths=16), call(p1=-0.1), call(p1=0.9), call(p1=nan), call(p2=nan), call(p2=inf), call(p1=inf, p2=inf), call(invalid=nan),
               call(invalid=inf), call(invalid=-inf), call(volume=None), call(depths=None), call(depth=None), call(index=None), call(cost=None),
               call(ws=None), call(volume=v.data_ptr() + 4), call(depths=z.data_ptr() + 4), call(depth=out["depth"].data_ptr() + 4),
               call(cost=out["cost"].data_ptr() + 4), call(index=out["index"].data_ptr() + 2), call(aggregated=out["aggregated"].data_ptr() + 4),
               call(aggregated=v.data_ptr()), call(ws=ws.data_ptr() + 8), call(False, ws_bytes=need - 1), call(False, ws_bytes=0)]
    assert all(rc == -1 for rc in refused), refused
    assert b"sfm_sgm_aggregate" in lib.sfm_last_error()
    assert call(R=0) == 0 and call(False, R=0, ws_bytes=0) == 0   # no reference: a no-op
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(out[name], before[name]), name
    assert call(ws_bytes=0) == 0   # the same arguments are accepted; with `aggregated` the workspace may be empty
    torch.cuda.synchronize()
    assert_same({k: t.cpu().numpy() for k, t in out.items()}, so.sgm_aggregate(volume, depths), "the C entry point")


def test_opcheck():
    torch, device = _device()
    from structure_from_motion_amd import ops

    op = ops.load()
    volume, depths = cases.random_volume((2, 5, 6, 17), 75)
    v, z = device.to_device(volume), device.to_device(depths)
    # not test_aot_dispatch_dynamic, as for the sweep: its assert_close takes the NaNs of pixels without a winner for a difference
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    for keep in (False, True):
        torch.library.opcheck(op.sgm_aggregate.default, (v, z, 0.1, 0.8, 1.0, 8, keep), test_utils=tests)
    ws = device.SgmWorkspace(2, 6, 17, 5, aggregated=True)
    torch.library.opcheck(op.sgm_aggregate_.default, (v, z, 0.1, 0.8, 1.0, 8) + ws.buffers(), test_utils=tests)
    none = device.SgmWorkspace(2, 6, 17, 5)
    torch.library.opcheck(op.sgm_aggregate_.default, (v, z, 0.1, 0.8, 1.0, 8) + none.buffers(), test_utils=tests)
    ws.run(v, z)
    for got, name in zip(op.sgm_aggregate(v, z, 0.1, 0.8, 1.0, 8, True), NAMES):   # the functional and the in-place form agree
        assert po.same_bytes(got.cpu().numpy(), getattr(ws, name).cpu().numpy()), name
    assert op.sgm_aggregate(v, z, 0.1, 0.8, 1.0, 8, False)[3].numel() == 0
