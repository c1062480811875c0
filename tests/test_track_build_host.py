"""Tracks from pairwise matches without a GPU: the plain-Python oracle against a BFS labelling and the contract's
invariants, the argument checks of the public API, the C ABI's refusals, the op registration and Meta shapes, the
synthetic generators and the lib re-export."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch

import track_build_oracle as tbo
from structure_from_motion_amd import synthetic

EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h


def _random_graph(seed, images=6, max_features=12, pairs=10, max_matches=8):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_features, images)
    ps, ms = [], []
    for _ in range(pairs):
        a, b = rng.choice(images, 2, replace=False)
        k = int(rng.integers(0, max_matches)) if counts[a] and counts[b] else 0
        ps.append((a, b))
        ms.append(np.column_stack([rng.integers(0, max(counts[a], 1), k), rng.integers(0, max(counts[b], 1), k)]))
    return counts, ps, ms


def _bfs_components(F, edges):
    adj = [[] for _ in range(F)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    label = [-1] * F
    for s in range(F):
        if label[s] >= 0:
            continue
        members, queue = [s], deque([s])
        label[s] = s
        while queue:
            v = queue.popleft()
            for w in adj[v]:
                if label[w] < 0:
                    label[w] = s
                    members.append(w)
                    queue.append(w)
    return np.array(label, dtype=np.int64)


@pytest.mark.parametrize("seed", range(20))
def test_oracle_matches_bfs_and_invariants(seed):
    counts, ps, ms = _random_graph(seed)
    args = tbo.from_lists(counts, ps, ms)
    r = tbo.build_tracks(*args)
    F = int(np.sum(counts))
    edges = tbo.global_edges(*args)
    label = _bfs_components(F, edges.tolist())   # BFS from increasing start: the label is the smallest id
    assert np.array_equal(r["component"], label)
    image = np.repeat(np.arange(len(counts)), counts)
    M = r["info"][3]
    cam, pt, fid = r["camera_index"][:M], r["point_index"][:M], r["feature_index"][:M]
    assert np.all(r["camera_index"][M:] == -1) and np.all(r["feature_index"][M:] == -1)
    assert np.array_equal(cam, image[fid])
    # by track, then strictly increasing global id (so strictly increasing image) inside a track
    for a in range(M - 1):
        assert (pt[a], fid[a]) < (pt[a + 1], fid[a + 1])
        if pt[a] == pt[a + 1]:
            assert cam[a] < cam[a + 1]
    # tracks numbered by increasing component id, every track of two features or more
    first = fid[np.r_[True, pt[1:] != pt[:-1]]] if M else fid
    assert np.all(np.diff(r["component"][first]) > 0)
    assert np.all(np.bincount(pt) >= 2) if M else True
    ok = r["status"] == tbo.OK
    assert np.array_equal(np.sort(fid), np.nonzero(ok)[0])
    assert np.all(r["track"][~ok] == -1)
    sizes = np.bincount(label, minlength=F)
    assert np.all((r["status"] == tbo.UNMATCHED) == (sizes[label] == 1))
    assert r["info"][5] == np.count_nonzero(sizes[label] == 1)


def test_oracle_conflict_and_bad_index():
    # image 0 features 0, 1; image 1 feature 2: 0-2 and 1-2 put two features of image 0 in one component
    r = tbo.build_tracks(*tbo.from_lists([2, 1, 2], [(0, 1), (1, 0), (2, 1)], [[(0, 0)], [(0, 1)], [(0, 0)]]))
    assert list(r["status"]) == [tbo.CONFLICT, tbo.CONFLICT, tbo.CONFLICT, tbo.CONFLICT, tbo.UNMATCHED]
    assert r["info"] == (0, 1, 0, 0, 1, 1)
    bad = tbo.build_tracks(*tbo.from_lists([2, 1], [(0, 1)], [[(2, 0)]]))
    assert bad["info"][0] == 1 and np.all(bad["status"] == tbo.BAD_INDEX)


def test_public_api_rejects_bad_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd import device
    from structure_from_motion_amd.multiview.tracks import build_tracks

    def no_device(*_a, **_k):
        raise AssertionError("device work before the checks")

    monkeypatch.setattr(device, "require_gpu", no_device)
    feats = [np.zeros((3, 2)), np.zeros((2, 2)), np.zeros((0, 2))]
    bad = [
        (feats, [(0, 0)], [np.zeros((0, 2), dtype=int)]),                  # equal images
        (feats, [(0, 3)], [np.zeros((0, 2), dtype=int)]),                  # image out of range
        (feats, [(0, 1)], [np.array([[3, 0]])]),                            # local index out of range
        (feats, [(0, 1)], [np.array([[0, 2]])]),
        (feats, [(0, 1)], [np.array([[-1, 0]])]),
        (feats, [(0, 1)], [np.array([[0, 0, 0]])]),                         # wrong shape
        (feats, [(0, 1)], []),                                              # one entry per pair
        (feats, [(0, 1, 2)], [np.zeros((0, 2), dtype=int)]),
        (feats, [(0, 1)], [np.array([[0.5, 0.0]])]),                        # not integers
        ([np.zeros((3, 3))], [], []),                                       # pixels not (n, 2)
        (feats, [(0, 2)], [np.array([[0, 0]])]),                            # image 2 has no features
    ]
    for f, p, m in bad:
        with pytest.raises(ValueError):
            build_tracks(f, p, m)


def test_abi_exports_and_refusals(native_lib):
    from structure_from_motion_amd import _native

    lib = _native.load()
    assert "sfm_build_tracks" in _native.SIGNATURES
    assert "sfm_build_tracks_workspace_bytes" in _native.OTHER_SYMBOLS
    ws = lib.sfm_build_tracks_workspace_bytes
    assert ws(3, 100, 50) > 0 and ws(0, 0, 0) > 0
    for args in [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (2**31 - 1, 0, 0), (0, 2**31 - 1, 0), (0, 0, 2**31)]:
        assert ws(*args) == -1
    info = (C.c_int64 * 6)()
    buf = (C.c_int64 * 64)()   # host memory: a refused call never touches it
    dummy = C.cast(buf, C.c_void_p)
    call = lib.sfm_build_tracks
    # negative sizes, too large, matches without pairs, null pointers, workspace too small: SFM_EINVAL before any launch
    assert call(-1, 0, 0, 0, dummy, dummy, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, info, dummy, 512, None) \
        == EINVAL
    assert call(1, 2**31 - 1, 0, 0, dummy, dummy, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, info, dummy, 512,
                None) == EINVAL
    assert call(1, 4, 0, 3, dummy, dummy, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, info, dummy, 512, None) \
        == EINVAL
    assert call(1, 4, 1, 3, dummy, dummy, None, dummy, None, dummy, dummy, dummy, dummy, dummy, info, dummy, 512, None) \
        == EINVAL
    assert call(1, 4, 1, 3, dummy, dummy, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, None, dummy, 512, None) \
        == EINVAL
    assert call(1, 10**6, 1, 3, dummy, dummy, dummy, dummy, None, dummy, dummy, dummy, dummy, dummy, info, dummy, 512,
                None) == EINVAL
    assert b"workspace" in lib.sfm_last_error()


def test_op_registration_and_meta_shapes(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    assert "build_tracks" in ops.FUNCTIONAL_OPS and "build_tracks_" in ops.INPLACE_OPS
    assert "Tensor(a!) component" in str(op.build_tracks_.default._schema)
    meta = dict(device="meta", dtype=torch.int32)
    out = op.build_tracks(torch.empty(5, **meta), torch.empty((7, 2), **meta), torch.empty(8, **meta),
                          torch.empty((40, 2), **meta), 123)
    assert len(out) == 7
    for t in out[:2] + out[3:6]:
        assert t.shape == (123,) and t.dtype == torch.int32 and t.device.type == "meta"
    assert out[2].shape == (123,) and out[2].dtype == torch.uint8
    assert out[6].shape == (6,) and out[6].dtype == torch.int64
    with pytest.raises(Exception):
        op.build_tracks(torch.empty(5, **meta), torch.empty((7, 3), **meta), torch.empty(8, **meta),
                        torch.empty((40, 2), **meta), 123)
    with pytest.raises(Exception):
        op.build_tracks(torch.empty(5, **meta), torch.empty((7, 2), **meta), torch.empty(7, **meta),
                        torch.empty((40, 2), **meta), 123)


def test_pairwise_matches_invariants():
    scene = synthetic.multi_view_scene(6, 300, seed=4)
    pm = synthetic.pairwise_matches(scene, window=2, wrong_fraction=0.0, seed=1)
    V = 6
    assert [tuple(p) for p in pm["pairs"]] == [(i, j) for i in range(V) for j in range(i + 1, min(V, i + 3))]
    cam, pt = scene["camera_indices"], scene["point_indices"]
    for v in range(V):
        assert len(pm["features"][v]) == np.count_nonzero(cam == v)
        assert sorted(pm["feature_points"][v]) == sorted(pt[cam == v])
    for (i, j), m in zip(pm["pairs"], pm["matches"]):
        assert np.array_equal(pm["feature_points"][i][m[:, 0]], pm["feature_points"][j][m[:, 1]])
        assert len(m) == len(np.intersect1d(pt[cam == i], pt[cam == j]))
    noisy = synthetic.pairwise_matches(scene, window=2, wrong_fraction=0.3, seed=1)
    wrong = np.concatenate(noisy["wrong"])
    assert 0.2 < wrong.mean() < 0.4
    for (i, j), m, w in zip(noisy["pairs"], noisy["matches"], noisy["wrong"]):
        same = noisy["feature_points"][i][m[:, 0]] == noisy["feature_points"][j][m[:, 1]]
        assert np.array_equal(same, ~w)


def test_match_graph_invariants():
    g = synthetic.match_graph(20, 400, 3, 50, wrong_fraction=0.0, seed=2)
    assert g["pairs"].shape == (60, 2) and g["match_index"].shape == (3000, 2)
    assert np.array_equal(g["image_offset"], np.arange(21) * 400)
    owner = np.repeat(np.arange(60), 50)
    ga = g["image_offset"][g["pairs"][owner, 0]] + g["match_index"][:, 0]
    gb = g["image_offset"][g["pairs"][owner, 1]] + g["match_index"][:, 1]
    assert np.array_equal(g["feature_points"][ga], g["feature_points"][gb])   # clean matches join one latent point
    for i in range(20):   # an image never sees a point twice
        fp = g["feature_points"][i * 400:(i + 1) * 400]
        assert len(np.unique(fp)) == 400


def test_lib_reexport():
    from lib.multiview import tracks as lib_tracks
    from structure_from_motion_amd.multiview import tracks

    assert lib_tracks.build_tracks is tracks.build_tracks
    assert lib_tracks.TrackBuildResult is tracks.TrackBuildResult
