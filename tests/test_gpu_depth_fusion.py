"""sfm_tsdf_integrate and sfm_tsdf_extract_mesh on the GPU against their NumPy definition (tests/tsdf_oracle.py), byte for byte, a
NaN equal to any NaN: the definition uses only correctly rounded float64 operations in a fixed order.  The shapes
are the smallest at which the kernels can go wrong: volumes ragged against the block, every way a view can miss a voxel, states
with holes, zero corners, no crossing at all, one cell, and more cells than one tile of the scan."""
import numpy as np
import pytest

import tsdf_cases as cases   # registers the stream case of the two entry points (tests/test_gpu_streams.py runs it)
import tsdf_oracle as to

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = 12345.0, 77   # what the outputs hold before a call: every element must be written


def _device():
    import torch

    from structure_from_motion_amd import device

    return torch, device


def _state_up(state):
    torch, device = _device()
    total, count, grey = state
    return (device.to_device(total), device.to_device(count, torch.int32), None if grey is None else device.to_device(grey, torch.int32))


def _state_down(state):
    return tuple(None if t is None else t.cpu().numpy() for t in state)


def run_integrate(state, sc, views, origin, voxel_size, truncation, with_grey=True, splits=None):
    """The in-place wrapper on a copy of ``state``; ``splits``: the bounds of several calls over the view list."""
    torch, device = _device()
    dev_state = _state_up(state)
    depth, K, poses = device.to_device(sc["depth"]), device.to_device(sc["K"]), device.to_device(sc["poses"])
    images = device.to_device(sc["images"], torch.uint8) if with_grey else None
    views = np.asarray(views, dtype=np.int32)
    status = []
    for a, b in splits or [(0, len(views))]:
        part = torch.full((b - a,), POISON_I, dtype=torch.int32, device="cuda")
        device.tsdf_integrate(dev_state, depth, images, K, poses, device.to_device(views[a:b], torch.int32), origin, voxel_size, truncation,
                              status=part)
        status.append(part.cpu().numpy())
    return _state_down(dev_state) + (np.concatenate(status),)


def assert_state(got, want, what=""):
    for name, g, w in zip(("sum", "count", "grey_sum", "status"), got, want):
        if w is None:
            assert g is None, name
            continue
        assert to.same_bytes(g, w), f"{what}: {name} differs from the definition in {int(np.sum(g != w))} of {w.size} elements"


def check_integrate(dims, views, with_grey=True, state=None, splits=None):
    sc = cases.integrate_scene()
    origin, s, trunc = cases.integrate_volume(dims)
    state = cases.empty_state(dims, with_grey) if state is None else state
    got = run_integrate(state, sc, views, origin, s, trunc, with_grey, splits)
    want = to.integrate(state, sc["depth"], sc["images"] if with_grey else None, sc["K"], sc["poses"], views, origin, s, trunc)
    assert_state(got, want, f"dims {dims} views {views}")
    return want


# ---- integration ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 6, 7), (17, 9, 4), (33, 2, 2)])
@pytest.mark.parametrize("views", [[], [1], [0, 1, 3]])
def test_integrate_ragged_volumes(dims, views):
    want = check_integrate(dims, views)
    if len(views) == 3 and dims != (1, 1, 1):
        assert want[1].max() == 3 and want[1].min() == 0   # voxels that every view sees, and voxels that none does
    if dims == (33, 2, 2) and views:
        assert np.all(want[1][:, :, 0] == 0) and np.all(want[1][:, :, -1] == 0)   # they project outside the image


def test_integrate_a_view_that_looks_away_and_a_bad_index_between_two_good_ones():
    want = check_integrate((17, 9, 4), [0, 7, 2, -1, 3])
    assert want[3].tolist() == [0, 1, 0, 1, 0]
    alone = check_integrate((17, 9, 4), [2])
    assert np.all(alone[1] == 0) and alone[3].tolist() == [0]   # z <= 0 for every voxel
    both = check_integrate((17, 9, 4), [0, 3])
    assert to.same_bytes(both[0], want[0]) and np.array_equal(both[1], want[1])   # the skipped entries add nothing


def test_integrate_skips_depths_that_are_none():
    """NaN, infinite, zero and negative depths (cases.integrate_scene): the voxels that look at them count fewer views."""
    sc = cases.integrate_scene()
    clean = dict(sc, depth=np.where(np.isfinite(sc["depth"]) & (sc["depth"] > 0), sc["depth"], 5.0))
    dims = (17, 9, 4)
    origin, s, trunc = cases.integrate_volume(dims)
    want = check_integrate(dims, [0, 1, 3])
    full = to.integrate(cases.empty_state(dims), clean["depth"], clean["images"], clean["K"], clean["poses"], [0, 1, 3], origin, s, trunc)
    assert (want[1] < full[1]).any() and not (want[1] > full[1]).any()


def test_integrate_without_images_from_a_state_and_in_two_calls():
    dims = (5, 6, 7)
    check_integrate(dims, [0, 1, 3], with_grey=False)
    rng = np.random.default_rng(0)
    state = (rng.normal(size=dims[::-1]), rng.integers(0, 9, size=dims[::-1]).astype(np.int32),
             rng.integers(0, 999, size=dims[::-1]).astype(np.int32))
    started = check_integrate(dims, [3, 0], state=state)
    assert not to.same_bytes(started[0], state[0])
    whole = check_integrate(dims, [0, 1, 3, 1, 0])
    for splits in ([(0, 2), (2, 5)], [(0, 1), (1, 4), (4, 5)], [(0, 0), (0, 5)]):
        check_integrate(dims, [0, 1, 3, 1, 0], splits=splits)   # the same bytes as one call, which `whole` is
    assert whole[1].max() == 5


def test_integrate_on_the_truncation_bounds_and_on_half_a_pixel():
    column = cases.exact_column_case()
    sc = dict(depth=column["depth"], K=column["K"], poses=column["poses"], images=None)
    got = run_integrate(cases.empty_state(column["dims"], False), sc, [0], column["origin"], column["voxel_size"], column["truncation"], False)
    assert got[0][:, 0, 0].tolist() == [1.0] * 7 + [0.5, 0.0, -0.5, -1.0, 0.0] and got[1][:, 0, 0].tolist() == [1] * 11 + [0]
    voxel = cases.exact_voxel_case()
    y, x = voxel["pixel"]
    for d, at, want in ((1.75, (y, x), (-1.0, 1)), (float(np.nextafter(1.75, 0.0)), (y, x), (0.0, 0)), (2.25, (y, x), (1.0, 1)),
                        (2.0, (y, x - 1), (0.0, 0)), (2.125, (y, x), (0.5, 1))):
        depth = np.full((1, 8, 40), np.nan)
        depth[0][at] = d
        sc = dict(depth=depth, K=voxel["K"], poses=voxel["poses"], images=None)
        got = run_integrate(cases.empty_state((1, 1, 1), False), sc, [0], voxel["origin"], voxel["voxel_size"], voxel["truncation"], False)
        assert (float(got[0][0, 0, 0]), int(got[1][0, 0, 0])) == want, (d, at)


def test_integrate_the_slanted_plane():
    sc = cases.plane_scene()
    sc = dict(depth=sc["depth"], images=sc["images"], K=np.ascontiguousarray(sc["K"].reshape(9)), poses=sc["poses"])
    got = run_integrate(cases.empty_state(cases.PLANE_DIMS), sc, np.arange(5), cases.PLANE_ORIGIN, cases.PLANE_VOXEL, cases.PLANE_TRUNCATION)
    assert_state(got, cases.fused_plane(), "the slanted plane")


# ---- extraction -----------------------------------------------------------------------------------------------------------------------
def run_extract(state, origin, voxel_size, min_count, max_triangles):
    torch, device = _device()
    dev_state = _state_up(state)
    out = (torch.full((max_triangles, 3, 3), POISON_F, dtype=torch.float64, device="cuda"),
           None if state[2] is None else torch.full((max_triangles, 3), POISON_F, dtype=torch.float64, device="cuda"),
           torch.full((1,), POISON_I, dtype=torch.int64, device="cuda"))
    device.tsdf_extract_mesh(dev_state, origin, voxel_size, min_count, out=out)
    return out[0].cpu().numpy(), None if out[1] is None else out[1].cpu().numpy(), int(out[2].cpu().numpy()[0])


def check_extract(state, origin, voxel_size, min_count=1):
    """The mesh with max_triangles of 0, of less than the total, of the total and of more, each against the definition."""
    full = to.extract_mesh(*state, origin, voxel_size, min_count)
    found = full[2]
    for rows in sorted({0, found // 2, max(found - 1, 0), found, found + 5}):
        got = run_extract(state, origin, voxel_size, min_count, rows)
        want = to.extract_mesh(*state, origin, voxel_size, min_count, rows)
        assert got[2] == want[2] == found, (rows, got[2], found)
        assert to.same_bytes(got[0], want[0]), f"max_triangles {rows}: vertices differ"
        if state[2] is None:
            assert got[1] is None
        else:
            assert to.same_bytes(got[1], want[1]), f"max_triangles {rows}: grey differs"
        assert not np.any(got[0] == POISON_F) and np.all(np.isnan(got[0][found:]))   # every element was written
    return full


def test_extract_the_sphere():
    total, count = cases.sphere_state()
    full = check_extract((total, count, None), cases.SPHERE["origin"], cases.SPHERE["voxel_size"])
    assert full[2] == 1496
    check_extract((total, count, (count * 100).astype(np.int32)), cases.SPHERE["origin"], cases.SPHERE["voxel_size"])   # a constant grey


@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_extract_a_state_with_holes(min_count):
    total, count, grey, origin, s = cases.holes_state()
    found = [to.extract_mesh(total, count, grey, origin, s, m)[2] for m in (1, 2, 3)]
    assert found[0] > found[1] > found[2] > 0   # each min_count leaves other cells
    check_extract((total, count, grey), origin, s, min_count)
    if min_count == 2:
        check_extract((total, count, None), origin, s, min_count)


def test_extract_corners_that_are_exactly_zero():
    total, count, grey, origin, s = cases.zero_corner_state()
    full = check_extract((total, count, grey), origin, s)
    assert (np.linalg.norm(cases.normals(full[0]), axis=1) == 0.0).any()


def test_extract_no_crossing_and_one_cell():
    total, count = cases.sphere_state()
    nothing = check_extract((np.abs(total) + 1.0, count, None), cases.SPHERE["origin"], cases.SPHERE["voxel_size"])
    assert nothing[2] == 0
    assert check_extract((total, np.zeros_like(count), None), cases.SPHERE["origin"], cases.SPHERE["voxel_size"])[2] == 0   # no valid cell
    one = (np.array([-1.0, -1.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]).reshape(2, 2, 2), np.ones((2, 2, 2), dtype=np.int32),
           np.arange(8, dtype=np.int32).reshape(2, 2, 2) * 30)
    assert check_extract(one, (-0.5, -0.5, -0.5), 1.0)[2] == 8


def test_extract_across_scan_tiles():
    total, count, _, origin, s = cases.two_tile_state()
    assert total.shape == (17, 17, 18) and 16 * 16 * 17 == 4352 > 4096   # more cells than one tile of the scan
    full = check_extract((total, count, None), origin, s)
    # triangles on both sides of cell 4096, the first of the second tile: the offsets of the later ones carry the first tile's sum
    cell = np.floor((full[0].mean(axis=1) - (np.array(origin) + 0.5 * s)) / s).astype(np.int64)
    linear = (cell[:, 2] * 16 + cell[:, 1]) * 17 + cell[:, 0]
    assert np.all(np.diff(linear) >= 0) and (linear < 4096).sum() > 1000 and (linear >= 4096).sum() > 20


def test_the_python_layer_and_the_ops_match_the_definition():
    torch, device = _device()
    from structure_from_motion_amd import ops
    from structure_from_motion_amd.stereo import depth_maps as dm
    from structure_from_motion_amd.stereo import fusion

    sc = cases.plane_scene()
    volume = fusion.TsdfVolume(cases.PLANE_ORIGIN, cases.PLANE_VOXEL, cases.PLANE_DIMS, with_grey=True)
    assert volume.truncation == 4 * cases.PLANE_VOXEL == cases.PLANE_TRUNCATION
    volume.integrate(sc["depth"], sc["K"], sc["poses"], views=[0, 1], images=sc["images"])
    volume.integrate(sc["depth"], sc["K"], sc["poses"], views=[2, 3, 4], images=sc["images"])
    want = cases.fused_plane()
    assert_state(volume.to_host(), want[:3], "TsdfVolume")
    mesh = volume.extract_mesh(3)
    expect = to.extract_mesh(*want[:3], cases.PLANE_ORIGIN, cases.PLANE_VOXEL, 3)
    assert to.same_bytes(mesh.vertices, expect[0]) and to.same_bytes(mesh.grey, expect[1]) and len(mesh.vertices) == 2992
    points, faces, grey = mesh.weld()
    assert len(points) < 3 * len(faces) and cases.plane_distance(points).max() <= 0.25
    # fuse_depth_maps: the same maps as a FilteredDepthMaps, bounds given
    filtered = dm.FilteredDepthMaps(sc["depth"], np.zeros(sc["depth"].shape, np.int32), np.zeros(sc["depth"].shape + (3,)), np.arange(5),
                                    sc["images"])
    high = tuple(o + n * cases.PLANE_VOXEL for o, n in zip(cases.PLANE_ORIGIN, cases.PLANE_DIMS))
    fused = fusion.fuse_depth_maps(filtered, sc["K"], sc["poses"], cases.PLANE_VOXEL, min_count=3, bounds=(cases.PLANE_ORIGIN, high))
    assert len(fused.vertices) > 2000 and cases.plane_distance(fused.vertices).max() <= 0.25
    # the functional ops leave the state as it is
    op = ops.load()
    state = _state_up(cases.empty_state(cases.PLANE_DIMS))
    args = (device.to_device(sc["depth"]), device.to_device(sc["images"], torch.uint8), device.to_device(sc["K"].reshape(9)),
            device.to_device(sc["poses"]), device.to_device(np.arange(5), torch.int32), *cases.PLANE_ORIGIN, cases.PLANE_VOXEL,
            cases.PLANE_TRUNCATION)
    new = op.tsdf_integrate(*state, *args)
    assert all(float(t.abs().sum()) == 0.0 for t in state)
    assert_state(tuple(t.cpu().numpy() for t in new), want, "tsdf_integrate")
    vertices, shade, found = op.tsdf_extract_mesh(new[0], new[1], new[2], *cases.PLANE_ORIGIN, cases.PLANE_VOXEL, 3, 3000)
    assert int(found.item()) == 2992 and to.same_bytes(vertices.cpu().numpy()[:2992], expect[0]) and to.same_bytes(shade.cpu().numpy()[:2992], expect[1])
    plain = op.tsdf_extract_mesh(new[0], new[1], None, *cases.PLANE_ORIGIN, cases.PLANE_VOXEL, 3, 10)
    assert plain[1].numel() == 0 and to.same_bytes(plain[0].cpu().numpy(), expect[0][:10])


def test_opcheck():
    torch, device = _device()
    from structure_from_motion_amd import ops

    op = ops.load()
    sc = cases.integrate_scene()
    dims = (5, 6, 7)
    origin, s, trunc = cases.integrate_volume(dims)
    state = _state_up(cases.empty_state(dims))
    inputs = (device.to_device(sc["depth"]), device.to_device(sc["images"], torch.uint8), device.to_device(sc["K"]), device.to_device(sc["poses"]),
              device.to_device(np.array([0, 1, 3]), torch.int32))
    # not test_aot_dispatch_dynamic: it compares the eager and the traced outputs with assert_close, under which the NaNs behind a
    # mesh's last triangle differ from themselves
    tests = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(op.tsdf_integrate.default, state + inputs + (*origin, s, trunc), test_utils=tests)
    torch.library.opcheck(op.tsdf_integrate.default, (state[0], state[1], None, inputs[0], None) + inputs[2:] + (*origin, s, trunc), test_utils=tests)
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.library.opcheck(op.tsdf_integrate_.default, state + inputs + (*origin, s, trunc, status), test_utils=tests)
    fused = op.tsdf_integrate(*state, *inputs, *origin, s, trunc)
    for grey_sum in (fused[2], None):
        torch.library.opcheck(op.tsdf_extract_mesh.default, (fused[0], fused[1], grey_sum, *origin, s, 1, 64), test_utils=tests)
        out = (torch.zeros((64, 3, 3), dtype=torch.float64, device="cuda"),
               None if grey_sum is None else torch.zeros((64, 3), dtype=torch.float64, device="cuda"),
               torch.zeros(1, dtype=torch.int64, device="cuda"))
        torch.library.opcheck(op.tsdf_extract_mesh_.default, (fused[0], fused[1], grey_sum, *origin, s, 1) + out, test_utils=tests)


# ---- the C entry points: refused calls leave their outputs untouched ---------------------------------------------------------------
def test_the_entry_points_and_refused_calls():
    torch, device = _device()
    from structure_from_motion_amd import _native

    lib = _native.load()
    sc = cases.integrate_scene()
    dims = (5, 6, 7)
    nx, ny, nz = dims
    (ox, oy, oz), s, trunc = cases.integrate_volume(dims)
    V, H, W, N, T = 4, 12, 16, 3, 400
    state = _state_up(cases.empty_state(dims))
    t = dict(sum=state[0], count=state[1], grey_sum=state[2], depth=device.to_device(sc["depth"]), images=device.to_device(sc["images"], torch.uint8),
             K=device.to_device(sc["K"]), poses=device.to_device(sc["poses"]), views=device.to_device(np.array([0, 1, 3]), torch.int32),
             status=torch.full((N,), POISON_I, dtype=torch.int32, device="cuda"),
             vertices=torch.full((T, 3, 3), POISON_F, dtype=torch.float64, device="cuda"),
             grey=torch.full((T, 3), POISON_F, dtype=torch.float64, device="cuda"), total=torch.full((1,), POISON_I, dtype=torch.int64, device="cuda"))
    ws = torch.zeros(lib.sfm_tsdf_mesh_workspace_bytes(nx, ny, nz) + 64, dtype=torch.uint8, device="cuda")
    before = {k: v.clone() for k, v in t.items()}
    p = {k: v.data_ptr() for k, v in t.items()}

    def fuse(**change):
        a = dict(sum=p["sum"], count=p["count"], grey_sum=p["grey_sum"], nx=nx, ny=ny, nz=nz, ox=ox, oy=oy, oz=oz, s=s, trunc=trunc, depth=p["depth"],
                 images=p["images"], V=V, H=H, W=W, K=p["K"], poses=p["poses"], views=p["views"], N=N, status=p["status"])
        a.update(change)
        return lib.sfm_tsdf_integrate(*a.values(), None)

    def mesh(**change):
        a = dict(sum=p["sum"], count=p["count"], grey_sum=p["grey_sum"], nx=nx, ny=ny, nz=nz, ox=ox, oy=oy, oz=oz, s=s, min_count=1, T=T,
                 vertices=p["vertices"], grey=p["grey"], total=p["total"], ws=ws.data_ptr(), ws_bytes=ws.numel() - 64)
        a.update(change)
        return lib.sfm_tsdf_extract_mesh(*a.values(), None)

    nan, inf = float("nan"), float("inf")
    refused = [fuse(nx=0), fuse(ny=-1), fuse(nz=0), fuse(nx=2 ** 11, ny=2 ** 10, nz=2 ** 10), fuse(nx=2 ** 40), fuse(ox=nan), fuse(oz=inf), fuse(s=0.0),
               fuse(s=-1.0), fuse(s=nan), fuse(trunc=0.0), fuse(trunc=inf), fuse(V=0), fuse(H=0), fuse(W=0), fuse(H=2 ** 16, W=2 ** 15), fuse(N=-1),
               fuse(images=None), fuse(grey_sum=None), fuse(sum=None), fuse(count=None), fuse(depth=None), fuse(K=None), fuse(poses=None),
               fuse(views=None), fuse(status=None), fuse(sum=p["sum"] + 4), fuse(count=p["count"] + 2), fuse(K=p["K"] + 1), fuse(views=p["views"] + 1),
               mesh(nx=1), mesh(ny=1), mesh(nz=0), mesh(nx=565, ny=565, nz=565), mesh(ox=nan), mesh(s=0.0), mesh(s=inf), mesh(min_count=0), mesh(T=-1),
               mesh(grey=None), mesh(grey_sum=None), mesh(sum=None), mesh(count=None), mesh(total=None), mesh(vertices=None), mesh(ws=None),
               mesh(vertices=p["vertices"] + 4), mesh(total=p["total"] + 4), mesh(ws=ws.data_ptr() + 8), mesh(ws_bytes=ws.numel() - 64 - 1),
               mesh(ws_bytes=0)]
    assert all(rc == -1 for rc in refused), refused
    assert b"sfm_tsdf_extract_mesh" in lib.sfm_last_error()
    assert fuse(N=0) == 0 and fuse(N=0, views=None, status=None) == 0   # no view: a no-op
    torch.cuda.synchronize()
    for name in ("sum", "count", "grey_sum", "status", "vertices", "grey", "total"):   # the state and the outputs
        assert torch.equal(t[name], before[name]), name
    assert fuse() == 0 and mesh() == 0   # the same arguments unchanged are accepted
    assert mesh(T=0, vertices=None, grey=None) == 0   # the total alone
    torch.cuda.synchronize()
    origin = (ox, oy, oz)
    want = to.integrate(cases.empty_state(dims), sc["depth"], sc["images"], sc["K"], sc["poses"], [0, 1, 3], origin, s, trunc)
    assert_state(tuple(t[k].cpu().numpy() for k in ("sum", "count", "grey_sum", "status")), want, "the C entry point")
    expect = to.extract_mesh(*want[:3], origin, s, 1, T)
    assert 0 < expect[2] < T == len(expect[0])
    assert int(t["total"].item()) == expect[2] and to.same_bytes(t["vertices"].cpu().numpy(), expect[0]) and to.same_bytes(t["grey"].cpu().numpy(), expect[1])
