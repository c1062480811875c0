"""Host side of the view-graph feature: the exports, the argument checks of ``sfm_verify_pairs`` and of
``verify_pairs``, the per-pair gate, the chunk boundaries and ``choose_seed_pair``.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import view_graph_oracle as vo
from structure_from_motion_amd.epipolar import view_graph as vg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = vo.ho.synthetic.BENCH_K
EINVAL = -1   # SFM_EINVAL


def test_exports_and_op_schema(native_lib):
    from structure_from_motion_amd import _native, build, device, ops

    assert "sfm_view_graph.hip" in build.SOURCES
    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15   # the change is additive
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint sfm_verify_pairs\s*\(", header) and "typedef struct sfm_pair_verdict" in header
    assert "sfm_verify_pairs" in _native.SIGNATURES and native_lib.sfm_verify_pairs is not None
    assert C.sizeof(_native.PairVerdict) == 24 and device.VERDICT_BYTES == 24
    assert device.PAIR_KINDS == ("none", "essential", "homography", "bad_offsets")
    assert hasattr(device, "ViewGraphWorkspace")
    op = ops.load()
    assert "verify_pairs_" in ops.INPLACE_OPS
    schema = str(op.verify_pairs_.default._schema)
    assert schema.startswith("sfm_hip::verify_pairs_(") and "Tensor(a!) S" in schema and "Tensor(p!) verdict" in schema
    import lib.epipolar.view_graph as drop_in

    assert drop_in.verify_pairs is vg.verify_pairs and drop_in.choose_seed_pair is vg.choose_seed_pair
    assert drop_in.ViewGraph is vg.ViewGraph


def _call(lib, n_total=100, pairs=3, h=10, aggregation=3, h_begin=0):
    return lib.sfm_verify_pairs(0, 1, h_begin, None, n_total, None, pairs, None, h, 1.0, aggregation, 0.8, *([None] * 17))


def test_entry_refuses_bad_arguments_before_any_launch(native_lib):
    lib = native_lib
    for kwargs in (dict(n_total=-1), dict(pairs=-1), dict(h=-1), dict(pairs=65536), dict(n_total=2**31), dict(h=2**31)):
        assert _call(lib, **kwargs) == EINVAL, kwargs
    assert _call(lib, pairs=65536) == EINVAL and b"65535" in lib.sfm_last_error()
    assert _call(lib, aggregation=7) == EINVAL and b"aggregation" in lib.sfm_last_error()
    assert _call(lib, aggregation=-1) == EINVAL
    assert _call(lib, h_begin=-1) == EINVAL and b"h_begin" in lib.sfm_last_error()
    assert _call(lib) == EINVAL and b"null pointer" in lib.sfm_last_error()
    assert _call(lib, pairs=0) == 0   # no pairs: a no-op


def test_zero_hypotheses_per_entry_point(native_lib):
    """The one parameter of the size checks that the three ragged calls share (csrc/sfm_ragged_pass.h): ``sfm_verify_pairs`` takes
    h_count = 0 (its selection then runs over zero rows) and is refused only for what comes behind the size checks;
    ``sfm_register_views`` and ``sfm_align_models`` refuse it."""
    lib = native_lib
    assert _call(lib, h=0) == EINVAL and b"null pointer" in lib.sfm_last_error()
    assert _call(lib, h=0, pairs=0) == 0
    assert _call(lib, h=-1) == EINVAL and b"negative size" in lib.sfm_last_error()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: the calls are refused first
    Kc = (C.c_double * 9)(*[float(v) for v in K.reshape(9)])
    for h in (0, -1):
        assert lib.sfm_register_views(1, 1, 0, p, 10, p, 2, p, Kc, h, 4.0, 3, 2, 20, p, p, p, p, p, p, p, p, p, q, p, p, None) == EINVAL
        assert b"at least one hypothesis" in lib.sfm_last_error()
        assert lib.sfm_align_models(1, 1, 0, p, 10, p, 2, 10, p, p, h, 3, 2, p, p, p, p, p, p, p, p, p, q, p, p, p, 1 << 30, None) == EINVAL
        assert b"at least one hypothesis" in lib.sfm_last_error()


def _graph(sizes=(10, 12)):
    rng = np.random.default_rng(3)
    features, pairs, matches = [], [], []
    for q, n in enumerate(sizes):
        features += [rng.uniform(0, 600, (n, 2)), rng.uniform(0, 600, (n, 2))]
        pairs.append((2 * q, 2 * q + 1))
        matches.append(np.column_stack([np.arange(n), np.arange(n)]))
    return features, pairs, matches


def test_verify_pairs_refuses_bad_arguments_before_device_work():
    features, pairs, matches = _graph()
    for bad_K in (np.eye(2), np.diag([0.0, 1.0, 1.0]), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="camera matrix"):
            vg.verify_pairs(bad_K, features, pairs, matches, 2e-5)
    with pytest.raises(ValueError, match="one entry per pair"):
        vg.verify_pairs(K, features, pairs, matches[:1], 2e-5)
    with pytest.raises(ValueError, match=r"shape \(Q, 2\)"):
        vg.verify_pairs(K, features, [0, 1, 2], matches, 2e-5)
    with pytest.raises(ValueError, match="index images"):
        vg.verify_pairs(K, features, [(0, 1), (2, 4)], matches, 2e-5)
    with pytest.raises(ValueError, match="two different images"):
        vg.verify_pairs(K, features, [(0, 1), (2, 2)], matches, 2e-5)
    outside = [matches[0], matches[1].copy()]
    outside[1][3, 1] = 12
    with pytest.raises(ValueError, match="outside its image"):
        vg.verify_pairs(K, features, pairs, outside, 2e-5)
    outside[1][3, 1] = -1
    with pytest.raises(ValueError, match="outside its image"):
        vg.verify_pairs(K, features, pairs, outside, 2e-5)
    with pytest.raises(ValueError, match="must hold integers"):
        vg.verify_pairs(K, features, pairs, [matches[0], matches[1].astype(np.float64)], 2e-5)
    for fraction in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_extra_fraction"):
            vg.verify_pairs(K, features, pairs, matches, 2e-5, min_extra_fraction=fraction)
    with pytest.raises(ValueError, match="one int per pair"):
        vg.verify_pairs(K, features, pairs, matches, 2e-5, min_num_extra_inliers=[1, 2, 3])
    with pytest.raises(ValueError, match="max_hypotheses_per_call"):
        vg.verify_pairs(K, features, pairs, matches, 2e-5, max_hypotheses_per_call=0)
    # no pairs: an empty graph, no device
    empty = vg.verify_pairs(K, features, [], [], 2e-5)
    assert empty.kind == [] and empty.E.shape == (0, 3, 3) and empty.inlier_matches == []


def test_per_pair_gate():
    counts = [0, 3, 10, 99, 100, 1025]
    assert vg.pair_min_extra(counts).tolist() == [0] * 6
    assert vg.pair_min_extra(counts, 8).tolist() == [8] * 6
    assert vg.pair_min_extra(counts, None, 0.4).tolist() == [0, 1, 4, 39, 40, 410]
    assert vg.pair_min_extra(counts, 8, 0.4).tolist() == [8, 8, 8, 39, 40, 410]
    assert vg.pair_min_extra(counts, [50, 0, 0, 0, 41, 0], 0.4).tolist() == [50, 1, 4, 39, 41, 410]
    assert vg.pair_min_extra([], 8, 0.4).tolist() == []
    with pytest.raises(ValueError):
        vg.pair_min_extra(counts, 1.5)
    with pytest.raises(ValueError):
        vg.pair_min_extra(counts, [1, 2])


def test_chunk_boundaries():
    assert vg.chunk_bounds(12, 64, 2**21) == [(0, 12)]
    assert vg.chunk_bounds(12, 64, 256) == [(0, 4), (4, 8), (8, 12)]
    assert vg.chunk_bounds(12, 64, 255) == [(0, 3), (3, 6), (6, 9), (9, 12)]
    assert vg.chunk_bounds(3, 2000, 100) == [(0, 1), (1, 2), (2, 3)]   # never fewer than one pair per call
    assert vg.chunk_bounds(0, 64, 256) == []
    assert vg.chunk_bounds(5, 0, 256) == [(0, 5)]
    big = vg.chunk_bounds(70000, 1, 2**21)   # a call takes at most 65 535 pairs
    assert big == [(0, 65535), (65535, 70000)]
    bounds = vg.chunk_bounds(285, 2000, 2**21)   # 1048 pairs per call
    assert bounds == [(0, 285)]
    assert vg.BYTES_PER_PAIR_HYPOTHESIS == 8 * 4 + 2 * 9 * 8 + 2 * (4 + 4 + 8 + 8)


def _table(kinds, e_counts, ratios):
    Q = len(kinds)
    none = np.full((Q, 3, 3), np.nan)
    return vg.ViewGraph(np.zeros((Q, 2), dtype=np.int64), list(kinds), none, none, np.array(e_counts, dtype=np.int64),
                        np.zeros(Q, dtype=np.int64), np.array(ratios, dtype=np.float64), [None] * Q, [None] * Q, [None] * Q)


def test_choose_seed_pair():
    # the pan has the most essential inliers and is not eligible
    g = _table(["homography", "homography", "essential", "essential", "none"], [283, 251, 187, 75, 0], [0.99, 0.99, 0.15, 0.1, np.inf])
    assert vg.choose_seed_pair(g) == 2
    assert vg.choose_seed_pair(g, min_count=187) == 2
    with pytest.raises(ValueError, match="no pair"):
        vg.choose_seed_pair(g, min_count=188)
    # ties on the count: the lower ratio; then the lower index
    g = _table(["essential"] * 4, [100, 120, 120, 120], [0.1, 0.5, 0.3, 0.3])
    assert vg.choose_seed_pair(g) == 2
    g = _table(["essential"] * 3, [120, 120, 120], [0.3, 0.3, 0.3])
    assert vg.choose_seed_pair(g) == 0
    with pytest.raises(ValueError, match="no pair"):
        vg.choose_seed_pair(_table(["homography", "none"], [50, 0], [1.0, np.inf]))
    with pytest.raises(ValueError, match="no pair"):
        vg.choose_seed_pair(_table([], [], []))


def test_fixture_covers_the_small_pairs_and_the_tile():
    scenes = vo.ragged_scenes()
    corr, offset, min_extra = vo.ragged_arrays(scenes)
    assert np.diff(offset).tolist() == list(vo.SIZES) and corr.shape == (offset[-1], 4)
    assert min_extra.tolist() == [n // 15 for n in vo.SIZES]
    features, pairs, matches = vo.match_graph(scenes)
    assert len(features) == 24 and pairs.shape == (12, 2) and [len(m) for m in matches] == list(vo.SIZES)
    assert vo.verdict(-1, 0, -1, 0, 0.8) == (vo.NONE, 0, 0, float("inf"))
    assert vo.verdict(3, 10, -1, 0, 0.8) == (vo.HOMOGRAPHY, 14, 0, float("inf"))
    assert vo.verdict(3, 76, 5, 94, 0.8)[0] == vo.ESSENTIAL and vo.verdict(3, 77, 5, 94, 0.8)[0] == vo.HOMOGRAPHY   # 80 / 100, 81 / 100
