"""The fusion stage without a GPU (csrc/sfm_tsdf.hip): the header, the binding and the op tuples agree; the
workspace size; every ValueError of the Python layer; welding and PLY files; the definition (tests/tsdf_oracle.py) on hand-computed
cases, on an analytic sphere and on the exact depth maps of a slanted plane."""
import numpy as np
import pytest

import stream_cases
import tsdf_cases as cases   # registers the stream case of the two entry points (see that module)
import tsdf_oracle as to
from structure_from_motion_amd import _native, ops
from structure_from_motion_amd.stereo import depth_maps as dm
from structure_from_motion_amd.stereo import fusion


# ---- the layers agree -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_ops_agree():
    import test_stream_cases_host as header

    functions = header.declared()
    for name in ("sfm_tsdf_integrate", "sfm_tsdf_extract_mesh"):
        params, comment = functions[name]
        assert name in _native.SIGNATURES and params.endswith("void* stream")
        assert len(_native.SIGNATURES[name]) == params.count(",") + 1
        assert comment and header.SYNC_PHRASE not in comment
        assert name in stream_cases.covered_entries()
    assert "sfm_tsdf_mesh_workspace_bytes" in functions and "sfm_tsdf_mesh_workspace_bytes" in _native.OTHER_SYMBOLS
    with open(header.HEADER) as f:
        text = f.read()
    assert "#define SFM_TSDF_OK 0" in text and "#define SFM_TSDF_BAD_VIEW 1" in text
    assert _native.TSDF_STATUS == ("ok", "bad_view") and _native.ABI_VERSION == 15
    lib = _native.load()
    for name in ("sfm_tsdf_integrate", "sfm_tsdf_extract_mesh", "sfm_tsdf_mesh_workspace_bytes"):
        assert hasattr(lib, name)
    import lib.stereo.fusion as drop_in

    for name in ("Mesh", "TsdfVolume", "fuse_depth_maps", "save_ply", "suggest_voxel_size", "volume_bounds"):
        assert getattr(drop_in, name) is getattr(fusion, name)


def test_the_fusion_ops_are_listed_beside_the_pinned_tuples():
    assert ops.FUSION_OPS == ("tsdf_integrate", "tsdf_integrate_", "tsdf_extract_mesh", "tsdf_extract_mesh_")
    assert ops.DEPTH_MAP_OPS == ("plane_sweep", "plane_sweep_", "filter_depth_maps", "filter_depth_maps_")
    others = (ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS + ops.REGISTER_VIEWS_OPS + ops.SIMILARITY_OPS +
              ops.ALIGN_MODELS_OPS + ops.DEPTH_MAP_OPS)
    assert not set(ops.FUSION_OPS) & set(others)
    with open(ops.OPS_LIB_PATH.replace("libsfm_torch_ops.so", "sfm_torch_ops.cpp")) as f:
        source = f.read()
    for name in ops.FUSION_OPS:
        assert f'm.def("{name}(' in source and source.count(f'm.impl("{name}",') == 2   # the device kernel and the Meta kernel


def test_the_stream_case_runs_both_entry_points():
    case = stream_cases.CASES["tsdf_fusion"]
    assert case.entries == ("sfm_tsdf_integrate", "sfm_tsdf_extract_mesh") and case.ops == () and not case.synchronising


# ---- the workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_are_monotone_and_refused_sizes_give_minus_one():
    size = _native.load().sfm_tsdf_mesh_workspace_bytes
    base = (23, 18, 22)
    cells = 22 * 17 * 21
    assert size(*base) >= 4 * (cells + 1) and size(*base) % 256 == 0
    assert size(2, 2, 2) > 0
    for at in range(3):
        bigger = list(base)
        bigger[at] += 40
        assert size(*bigger) > size(*base)
    assert size(257, 257, 257) >= 4 * 256 ** 3
    assert size(564, 564, 564) > 0                       # 12 * 563^3 < 2^31
    refused = [(1, 18, 22), (23, 1, 22), (23, 18, 1), (0, 0, 0), (-23, -18, 22), (565, 565, 565), (2 ** 31, 2, 2), (2 ** 16, 2 ** 16, 2),
               (2 ** 40, 2 ** 40, 2 ** 40)]
    for sizes in refused:
        assert size(*sizes) == -1, sizes


# ---- the Python layer refuses before any device work -------------------------------------------------------------------------------
@pytest.mark.parametrize("change", [
    dict(origin=(0.0, 0.0)), dict(origin=(0.0, np.nan, 0.0)), dict(origin="abc"), dict(voxel_size=0.0), dict(voxel_size=-1.0),
    dict(voxel_size=np.inf), dict(voxel_size="1"), dict(voxel_size=True), dict(dims=(4, 4)), dict(dims=(4, 0, 4)), dict(dims=(4.0, 4.0, 4.0)),
    dict(dims=(-1, 4, 4)), dict(truncation=0.0), dict(truncation=-0.1), dict(truncation=np.nan), dict(with_grey=1),
    dict(dims=(512, 512, 513)), dict(dims=(10, 10, 11), max_voxels=1000), dict(max_voxels=0), dict(dims=(2 ** 11, 2 ** 10, 2 ** 10), max_voxels=2 ** 40),
])
def test_tsdf_volume_refuses(change):
    args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 4, 4))
    with pytest.raises(ValueError):
        fusion.TsdfVolume(**{**args, **change})


class _HostVolume(fusion.TsdfVolume):
    """A volume whose state was never allocated: what ``integrate`` and ``extract_mesh`` refuse, they refuse before touching it."""

    def __init__(self, dims=(4, 4, 4), with_grey=False):
        self.origin, self.voxel_size, self.truncation, self.dims, self.with_grey = (0.0, 0.0, 0.0), 0.1, 0.4, dims, with_grey
        self.sum = self.count = self.grey_sum = None


@pytest.mark.parametrize("change", [
    dict(depth=np.zeros((8, 10))), dict(depth=np.zeros((0, 8, 10))), dict(depth=np.zeros((2, 0, 10))), dict(K=np.eye(2)),
    dict(K=np.array([[1.0, 0, 0], [0.5, 1, 0], [0, 0, 1]])), dict(poses=np.zeros((3, 12))), dict(poses=np.full((2, 12), np.nan)),
    dict(views=[2]), dict(views=[-1]), dict(views=[[0, 1]]), dict(views=[0.5]), dict(images=np.zeros((2, 8, 10), dtype=np.uint8)),
])
def test_integrate_refuses(change):
    args = dict(depth=np.full((2, 8, 10), 3.0), K=np.eye(3), poses=np.tile(cases.sweep_cases.pose(), (2, 1)))
    with pytest.raises(ValueError):
        _HostVolume().integrate(**{**args, **change})


@pytest.mark.parametrize("images", [None, np.zeros((2, 8, 10), dtype=np.float32), np.zeros((2, 8, 11), dtype=np.uint8)])
def test_integrate_with_grey_refuses(images):
    with pytest.raises(ValueError):
        _HostVolume(with_grey=True).integrate(np.full((2, 8, 10), 3.0), np.eye(3), np.tile(cases.sweep_cases.pose(), (2, 1)), images=images)


def test_extract_mesh_refuses():
    for bad in (0, -1, 1.0, True, "1"):
        with pytest.raises(ValueError):
            _HostVolume().extract_mesh(bad)
    with pytest.raises(ValueError):
        _HostVolume(dims=(4, 1, 4)).extract_mesh()


def _filtered():
    points = np.full((2, 4, 5, 3), np.nan)
    points[0, 1, 1], points[1, 2, 3] = (0.0, -1.0, 4.0), (2.0, 1.0, 6.0)
    depth = np.full((2, 4, 5), np.nan)
    depth[0, 1, 1], depth[1, 2, 3], depth[1, 0, 0] = 4.0, 6.0, 8.0
    return dm.FilteredDepthMaps(depth, np.zeros((2, 4, 5), np.int32), points, np.arange(2), np.zeros((2, 4, 5), np.uint8))


@pytest.mark.parametrize("change", [
    dict(filtered=np.zeros((2, 4, 5))), dict(K=np.eye(4)), dict(poses=np.zeros((3, 12))), dict(voxel_size=0.0), dict(voxel_size=np.nan),
    dict(truncation=-1.0), dict(min_count=0), dict(min_count=1.5), dict(bounds=((0, 0, 0), (1, 1))), dict(bounds=((0, 0, 0), (1, 1, 0))),
    dict(bounds=((0, 0, 0), (1, np.inf, 1))), dict(voxel_size=1e-4),
])
def test_fuse_depth_maps_refuses(change):
    args = dict(filtered=_filtered(), K=np.eye(3), poses=np.tile(cases.sweep_cases.pose(), (2, 1)), voxel_size=0.5)
    with pytest.raises(ValueError):
        fusion.fuse_depth_maps(**{**args, **change})
    empty = _filtered()
    empty.points[:] = np.nan
    with pytest.raises(ValueError):
        fusion.fuse_depth_maps(**{**args, "filtered": empty})


def test_volume_bounds_and_voxel_size():
    low, high = fusion.volume_bounds(_filtered(), 0.5)
    assert np.array_equal(low, [-0.5, -1.5, 3.5]) and np.array_equal(high, [2.5, 1.5, 6.5])
    low, high = fusion.volume_bounds(np.array([[1.0, 2.0, 3.0], [np.inf, 0.0, 0.0]]))
    assert np.array_equal(low, [1.0, 2.0, 3.0]) and np.array_equal(high, low)
    for bad in ((np.zeros((3, 2)), 0.0), (np.full((3, 3), np.nan), 0.0), (np.zeros((3, 3)), -1.0), (np.zeros((3, 3)), np.nan)):
        with pytest.raises(ValueError):
            fusion.volume_bounds(*bad)
    K = np.array([[100.0, 0.0, 2.0], [0.0, 100.0, 2.0], [0.0, 0.0, 1.0]])
    assert fusion.suggest_voxel_size(_filtered(), K) == 2.0 * 6.0 / 100.0 and fusion.suggest_voxel_size(_filtered(), K, 1) == 0.06
    for bad in (dict(filtered=np.zeros((2, 4, 5))), dict(K=np.eye(2)), dict(pixels=0.0), dict(pixels=np.inf)):
        with pytest.raises(ValueError):
            fusion.suggest_voxel_size(**{**dict(filtered=_filtered(), K=K), **bad})


# ---- welding and PLY files ---------------------------------------------------------------------------------------------------------
def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    points = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    faces = int(next(h for h in header if h.startswith("element face")).split()[-1])
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if "property uchar red" in header else [])
    vertex = np.frombuffer(data, dtype=fields, count=points, offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=faces, offset=end + vertex.nbytes)
    assert end + vertex.nbytes + face.nbytes == len(data)
    return vertex, face


def test_weld_and_save_ply_round_trip(tmp_path):
    a, b, c, d = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, -0.0)
    vertices = np.array([[a, b, c], [b, d, c], [d, b, (1.0, 1.0, 0.0)]])   # -0.0 and 0.0 differ as bytes
    grey = np.array([[10.0, 20.5, 30.0], [20.5, 40.0, 30.0], [40.0, 20.5, 300.0]])
    points, faces, shade = fusion.Mesh(vertices, grey).weld()
    assert faces.dtype == np.int32 and faces.tolist() == [[0, 1, 2], [1, 3, 2], [3, 1, 4]]
    assert np.array_equal(points, [a, b, c, d, (1.0, 1.0, 0.0)]) and np.signbit(points[3, 2]) and not np.signbit(points[4, 2])
    assert shade.tolist() == [10.0, 20.5, 30.0, 40.0, 300.0]
    assert np.array_equal(points[faces], vertices)
    assert fusion.Mesh(vertices).weld()[2] is None
    nothing = fusion.Mesh(np.zeros((0, 3, 3)), np.zeros((0, 3))).weld()
    assert nothing[0].shape == (0, 3) and nothing[1].shape == (0, 3) and nothing[2].shape == (0,)
    fusion.save_ply(tmp_path / "grey.ply", fusion.Mesh(vertices, grey))
    vertex, face = _read_ply(tmp_path / "grey.ply")
    assert np.array_equal(np.stack([vertex["x"], vertex["y"], vertex["z"]], axis=1).view(np.uint64), points.view(np.uint64))
    assert vertex["red"].tolist() == [10, 20, 30, 40, 255] and np.array_equal(vertex["red"], vertex["blue"])
    assert np.all(face["n"] == 3) and np.array_equal(face["v"], faces)
    fusion.save_ply(tmp_path / "plain.ply", fusion.Mesh(vertices))
    vertex, face = _read_ply(tmp_path / "plain.ply")
    assert vertex.dtype.names == ("x", "y", "z") and np.array_equal(face["v"], faces)
    fusion.save_ply(tmp_path / "empty.ply", fusion.Mesh(np.zeros((0, 3, 3))))
    assert len(_read_ply(tmp_path / "empty.ply")[0]) == 0
    with pytest.raises(ValueError):
        fusion.save_ply(tmp_path / "bad.ply", vertices)


# ---- the definition on hand-computed cases -----------------------------------------------------------------------------------------
def _integrate(case, depth, images=None, views=(0,), state=None):
    state = cases.empty_state(case["dims"], images is not None) if state is None else state
    return to.integrate(state, depth, images, case["K"], case["poses"], views, case["origin"], case["voxel_size"], case["truncation"])


def test_oracle_one_voxel_on_the_truncation_bounds_and_on_half_a_pixel():
    case = cases.exact_voxel_case()
    assert [c.tolist() for c in to.centres(case["dims"], case["origin"], case["voxel_size"])] == [[1.0 / 64.0], [0.0], [2.0]]
    y, x = case["pixel"]

    def one(d, at=(y, x)):
        depth = np.full((1, 8, 40), np.nan)
        depth[0][at] = d
        images = np.zeros((1, 8, 40), dtype=np.uint8)
        images[0][at] = 200
        total, count, grey, status = _integrate(case, depth, images)
        assert status.tolist() == [0]
        return float(total[0, 0, 0]), int(count[0, 0, 0]), int(grey[0, 0, 0])

    assert one(1.75) == (-1.0, 1, 200)                          # sdf = -truncation exactly: kept
    assert one(np.nextafter(1.75, 0.0)) == (0.0, 0, 0)          # just below: hidden
    assert one(2.25) == (1.0, 1, 200)                           # sdf = truncation exactly
    assert one(9.0) == (1.0, 1, 200) and one(2.125) == (0.5, 1, 200) and one(2.0) == (0.0, 1, 200)
    assert one(2.0, at=(y, x - 1)) == (0.0, 0, 0)               # u = 16.5 rounds up to 17, not down to 16
    for none in (np.nan, np.inf, -np.inf, 0.0, -2.0):
        assert one(none) == (0.0, 0, 0)
    depth = np.full((1, 8, 40), 2.125)
    total, count, _, status = _integrate(case, depth, views=(0, 1, 0, -1))
    assert status.tolist() == [0, 1, 0, 1] and total[0, 0, 0] == 1.0 and count[0, 0, 0] == 2
    behind = dict(case, poses=cases.sweep_cases.pose(np.diag([-1.0, 1.0, -1.0]))[None])   # z = -2
    assert _integrate(behind, depth)[1][0, 0, 0] == 0


def test_oracle_column_under_a_constant_depth():
    case = cases.exact_column_case()
    total, count, _, _ = _integrate(case, case["depth"])
    assert to.centres(case["dims"], case["origin"], case["voxel_size"])[2].tolist() == [1.0 + k / 8.0 for k in range(12)]
    assert count[:, 0, 0].tolist() == [1] * 11 + [0]
    assert total[:, 0, 0].tolist() == [1.0] * 7 + [0.5, 0.0, -0.5, -1.0, 0.0]
    again = _integrate(case, case["depth"], state=(total, count, None))   # the state is in-out: a second view adds to it
    assert again[0][:, 0, 0].tolist() == [2.0] * 7 + [1.0, 0.0, -1.0, -2.0, 0.0] and again[1][:, 0, 0].tolist() == [2] * 11 + [0]


def _one_cell(values, grey=None, min_count=1):
    total = np.array(values, dtype=np.float64).reshape(2, 2, 2)   # corner q at [q >> 2, (q >> 1) & 1, q & 1]
    shade = None if grey is None else np.array(grey, dtype=np.int32).reshape(2, 2, 2)
    return to.extract_mesh(total, np.ones((2, 2, 2), dtype=np.int32), shade, (-0.5, -0.5, -0.5), 1.0, min_count)


def test_oracle_one_cell_with_one_negative_corner():
    # corner 0 at (0, 0, 0) is -1, all others +1: each of the six tetrahedra has corner 0, one triangle each, at the edge midpoints
    vertices, grey, total = _one_cell([-1, 1, 1, 1, 1, 1, 1, 1], grey=[0, 10, 20, 30, 40, 50, 60, 70])
    assert total == 6 and grey.shape == (6, 3)
    corner = [np.array([q & 1, (q >> 1) & 1, (q >> 2) & 1], dtype=np.float64) for q in range(8)]
    for t, tet in enumerate(to.TETRAHEDRA):
        want = [0.5 * corner[q] for q in tet[1:]]
        assert sorted(map(tuple, vertices[t])) == sorted(map(tuple, want))
        assert np.array_equal(vertices[t, 0], want[0])                          # (ab, ac, ad), b and c swapped or not
        assert sorted(grey[t].tolist()) == sorted(5.0 * q for q in tet[1:])     # half way from grey 0 to grey 10 q
        assert np.dot(cases.normals(vertices)[t], [1.0, 1.0, 1.0]) > 0          # away from the negative corner
    assert _one_cell([-1, 1, 1, 1, 1, 1, 1, 1], min_count=2)[2] == 0            # a corner below min_count: no cell


def test_oracle_one_cell_with_two_negative_corners():
    # corners 0 and 1 (the edge along x at y = z = 0) at -1, the others at +3: the vertices sit a quarter of the way along their edges
    vertices, _, total = _one_cell([-1, -1, 3, 3, 3, 3, 3, 3])
    # (0,1,3,7) and (0,5,1,7) hold both: two triangles each; the other four hold corner 0 alone
    assert total == 2 + 1 + 1 + 1 + 1 + 2
    first = vertices[:2]                      # tetrahedron (0,1,3,7): negatives a, b = 0, 1; others c, d = 3, 7
    ac, ad, bd, bc = (0.25, 0.25, 0.0), (0.25, 0.25, 0.25), (1.0, 0.25, 0.25), (1.0, 0.25, 0.0)
    assert np.array_equal(first[0, 0], ac) and sorted(map(tuple, first[0])) == sorted([ac, ad, bd])
    assert np.array_equal(first[1, 0], ac) and sorted(map(tuple, first[1])) == sorted([ac, bd, bc])
    n = cases.normals(vertices)
    assert np.all(n @ np.array([0.0, 1.0, 1.0]) > 0)   # away from the negative edge y = z = 0


def test_oracle_one_cell_with_three_negative_corners():
    # tetrahedron (0,1,3,7) with corners 0, 1, 3 negative and 7 positive: a = 7, (ab, ac, ad) = (7-0, 7-1, 7-3), t from the low corner
    vertices, _, total = _one_cell([-1, -1, 1, -1, 1, 1, 1, 3])
    first = vertices[0]
    want = [(0.25, 0.25, 0.25), (1.0, 0.25, 0.25), (1.0, 1.0, 0.25)]   # t = -1 / (-1 - 3) = 0.25 from corners 0, 1 and 3 towards 7
    assert np.array_equal(first[0], want[0]) and sorted(map(tuple, first)) == sorted(want)
    assert cases.normals(vertices)[0] @ np.array([0.0, 0.0, 1.0]) > 0 and total >= 1


def test_oracle_zero_corners_give_degenerate_triangles_all_the_same():
    total, count, grey, origin, s = cases.zero_corner_state()
    vertices, shade, found = to.extract_mesh(total, count, grey, origin, s)
    assert found > 0 and np.all(np.isfinite(vertices)) and np.all(np.isfinite(shade))
    areas = np.linalg.norm(cases.normals(vertices), axis=1)
    assert (areas == 0.0).any() and (areas > 0.0).any()


def test_oracle_output_order_and_truncated_output():
    total, count = cases.sphere_state()
    full, _, found = to.extract_mesh(total, count, None, cases.SPHERE["origin"], cases.SPHERE["voxel_size"])
    short, _, found_short = to.extract_mesh(total, count, None, cases.SPHERE["origin"], cases.SPHERE["voxel_size"], max_triangles=100)
    longer, _, _ = to.extract_mesh(total, count, None, cases.SPHERE["origin"], cases.SPHERE["voxel_size"], max_triangles=found + 7)
    assert found_short == found and to.same_bytes(short, full[:100])
    assert to.same_bytes(longer[:found], full) and np.all(np.isnan(longer[found:]))
    # cells in linear order, x fastest: the cell of a triangle, recovered from its centroid, never decreases
    cell = np.floor((full.mean(axis=1) - (np.array(cases.SPHERE["origin"]) + 0.5 * 0.25)) / 0.25).astype(np.int64)
    linear = (cell[:, 2] * 11 + cell[:, 1]) * 11 + cell[:, 0]
    assert np.all(np.diff(linear) >= 0)


# ---- the sphere ----------------------------------------------------------------------------------------------------------------------
def test_oracle_sphere_is_a_closed_oriented_manifold():
    total, count = cases.sphere_state()
    vertices, _, found = to.extract_mesh(total, count, None, cases.SPHERE["origin"], cases.SPHERE["voxel_size"])
    assert found == len(vertices) == 1496   # what the definition gives; DESIGN.md §6aj quotes it
    points, faces, _ = fusion.Mesh(vertices).weld()
    edges = cases.directed_edges(faces)
    assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)   # every directed edge once, its reverse once
    assert len(points) - len(edges) // 2 + len(faces) == 2                                  # Euler characteristic of a sphere
    centre = np.array(cases.SPHERE["centre"])
    assert np.all(np.einsum("ij,ij->i", cases.normals(vertices), vertices.mean(axis=1) - centre) > 0)   # outward
    radial = np.abs(np.linalg.norm(points - centre, axis=1) - cases.SPHERE["radius"]) / cases.SPHERE["voxel_size"]
    print("sphere: largest radial error in voxels", radial.max())
    assert radial.max() <= 0.5   # what linear interpolation of a distance field inside a cell cannot exceed


# ---- the slanted plane --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,min_count", [(1, 1), (1, 3), (7, 1), (7, 3)])
def test_oracle_slanted_plane(seed, min_count):
    total, count, grey, status = cases.fused_plane(seed)
    assert status.tolist() == [0] * 5 and count.max() == 5
    vertices, shade, found = to.extract_mesh(total, count, grey, cases.PLANE_ORIGIN, cases.PLANE_VOXEL, min_count)
    distance = cases.plane_distance(vertices)
    print("plane: triangles", found, "largest distance in voxels", distance.max())
    assert found > 2000 and distance.max() <= 0.25
    assert np.all(cases.normals(vertices)[:, 2] < 0)          # towards the cameras, which look along +z
    assert np.all((shade >= 0.0) & (shade <= 255.0))
    if seed == 1:
        assert found == 2992   # what the definition gives; DESIGN.md §6aj quotes it


def test_oracle_views_in_two_calls_equal_one_call():
    sc = cases.plane_scene()
    args = (sc["depth"], sc["images"], sc["K"], sc["poses"])
    scalars = (cases.PLANE_ORIGIN, cases.PLANE_VOXEL, cases.PLANE_TRUNCATION)
    first = to.integrate(cases.empty_state(cases.PLANE_DIMS), *args, [0, 1], *scalars)
    second = to.integrate(first[:3], *args, [2, 3, 4], *scalars)
    whole = cases.fused_plane()
    assert to.same_bytes(second[0], whole[0]) and np.array_equal(second[1], whole[1]) and np.array_equal(second[2], whole[2])
    assert not to.same_bytes(first[0], whole[0])
