"""Guided matching without a GPU: the NumPy definition against a plain triple-loop restatement, its identities, the exports
and bindings, the C ABI's refusals, the argument checks of the public API, the calls that need no device, the generator, the
lib re-export and the accuracy conditions of DESIGN.md section 6ad on the NumPy chain."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import graph_matching_oracle as gmo
import guided_matching_cases as gc
import guided_matching_oracle as go
import homography_oracle as ho
from oracle import sfm_oracle as orc
from structure_from_motion_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h


def _small_image(rng, n, values, share=0.75):
    bits = np.zeros((n, 32), dtype=np.uint8)
    if values is None:
        bits = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    else:
        bits[:, 0] = rng.choice(values, n)      # distances 0 .. 3: ties for best and second
    return bits, rng.random(n) < share, rng.uniform(-0.2, 0.2, (n, 2))


def _triple_loop(bits_a, valid_a, bits_b, valid_b, adm, max_distance, ratio, cross_check):
    """The definition restated with loops over rows, columns and descriptor bytes and nothing else; ``adm(a, b)`` is asked
    with image i's feature first in both summaries."""

    def d(a, b):
        return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(bits_a[a], bits_b[b]))

    def summary(n_self, n_other, dist, admitted):
        out = []
        for s in range(n_self):
            best = arg = second = None
            for o in range(n_other):
                if admitted(s, o) and (best is None or dist(s, o) < best):
                    best, arg = dist(s, o), o
            for o in range(n_other):
                if admitted(s, o) and o != arg and (second is None or dist(s, o) < second):
                    second = dist(s, o)
            out.append((best, arg, second))
        return out

    def distinct(dist, runner_up):
        return ratio is None or runner_up is None or float(dist) <= ratio * float(runner_up)

    ok = lambda a, b: bool(valid_a[a] and valid_b[b] and adm(a, b))   # noqa: E731
    rows = summary(len(bits_a), len(bits_b), d, ok)
    cols = summary(len(bits_b), len(bits_a), lambda b, a: d(a, b), lambda b, a: ok(a, b))
    partner, distance = [], []
    for a, (best, arg, second) in enumerate(rows):
        keep = best is not None and best <= max_distance and distinct(best, second)
        if keep and cross_check:
            keep = cols[arg][1] == a and distinct(best, cols[arg][2])
        partner.append(arg if keep else -1)
        distance.append(best if keep else -1)
    return np.array(partner, dtype=np.int32), np.array(distance, dtype=np.int32)


@pytest.mark.parametrize("seed", range(12))
def test_oracle_equals_the_triple_loop(seed):
    rng = np.random.default_rng(seed)
    n_a, n_b = int(rng.integers(0, 7)), int(rng.integers(0, 8))            # at most 6 x 7
    values = None if seed % 3 == 0 else [0, 1, 3, 7]
    a, b = _small_image(rng, n_a, values), _small_image(rng, n_b, values)
    if seed == 5:
        b[1][:] = False                                                     # no valid column at all
    # a hand-made admissibility pattern first: whatever the geometry would say
    pattern = rng.random((n_a, n_b)) < 0.6
    if seed == 7 and n_b:
        pattern[:, 1:] = False                                              # one admissible column: no runner-up
    d = gmo.distances(a[0], b[0])
    for max_distance in (0, 2, 256):
        for ratio in (None, 0.5, 0.8, 1.0):
            for cross_check in (False, True):
                want = _triple_loop(a[0], a[1], b[0], b[1], lambda x, y: pattern[x, y], max_distance, ratio, cross_check)
                adm = pattern & a[1][:, None] & b[1][None, :]
                got = gmo.decide(go.Summaries(d, adm), max_distance, ratio, cross_check)
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # then the two models: admissibility one scalar evaluation of the named error function per (a, b), a first
    for kind, name in ((go.KIND_ESSENTIAL, "bench"), (go.KIND_HOMOGRAPHY, "plane_bench")):
        model = gc.motion_model(name, kind)
        e = go.errors(model, kind, a[2], b[2])
        threshold = float(np.median(e)) if e.size else 1.0

        def adm_scalar(x, y):
            corr = np.array([[a[2][x, 0], a[2][x, 1], b[2][y, 0], b[2][y, 1]]])
            value = orc.sed_values(model, corr)[0] if kind == go.KIND_ESSENTIAL else ho.transfer_error(model, corr)[0]
            assert value.tobytes() == e[x, y].tobytes()
            return value <= threshold

        want = _triple_loop(a[0], a[1], b[0], b[1], adm_scalar, 256, 0.8, True)
        got = go.match_pair(a, b, model, kind, threshold, 256, 0.8, True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _images(seed, sizes=(23, 0, 40, 17), values=None):
    rng = np.random.default_rng(seed)
    return [_small_image(rng, n, values, 0.8) for n in sizes]


@pytest.mark.parametrize("seed", range(4))
def test_identity_homography_with_infinite_threshold_is_the_graph_matcher(seed):
    images = _images(200 + seed, values=None if seed % 2 else [0, 1, 3, 7, 15])
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    Q = len(pairs)
    for ratio, max_distance, cross_check in ((0.8, 256, True), (None, 2, False), (1.0, 256, True)):
        want = gmo.match_graph([im[:2] for im in images], pairs, max_distance, ratio, cross_check)
        got = go.match_graph(images, pairs, np.tile(np.eye(3), (Q, 1, 1)), [go.KIND_HOMOGRAPHY] * Q, [np.inf] * Q, max_distance,
                             ratio, cross_check)
        for q in range(Q):
            assert np.array_equal(got[0][q], want[0][q]) and np.array_equal(got[1][q], want[1][q])
            assert got[0][q].dtype == np.int64 and got[1][q].dtype == np.int32


def test_nothing_admitted_gives_all_minus_one_and_unknown_kinds_are_refused():
    a, b = _images(7, (9, 11))
    E = gc.motion_model("bench", go.KIND_ESSENTIAL)
    nan_model, one_nan = np.full((3, 3), np.nan), E.copy()
    one_nan[1, 2] = np.nan
    # (a homography with some NaN entries still maps a point with p2 <= 0 to the error +inf, which a threshold of +inf admits:
    # transfer_error's rule; at any finite threshold it admits nothing either)
    for model, kind, threshold in ((E, go.KIND_NONE, np.inf), (nan_model, go.KIND_ESSENTIAL, np.inf),
                                   (one_nan, go.KIND_ESSENTIAL, np.inf), (one_nan, go.KIND_HOMOGRAPHY, 1e300),
                                   (nan_model, go.KIND_HOMOGRAPHY, np.inf), (E, go.KIND_ESSENTIAL, np.nan),
                                   (np.eye(3), go.KIND_HOMOGRAPHY, np.nan)):
        partner, distance = go.match_pair(a, b, model, kind, threshold, 256, None, False)
        assert partner.tolist() == [-1] * 9 and distance.tolist() == [-1] * 9
    assert np.count_nonzero(go.match_pair(a, b, E, go.KIND_ESSENTIAL, np.inf, 256, None, False)[0] >= 0) == int(a[1].sum())
    nan_xy = (a[0], a[1], np.full((9, 2), np.nan))
    assert not (go.match_pair(nan_xy, b, E, go.KIND_ESSENTIAL, np.inf, 256, None, False)[0] >= 0).any()
    for kind in (3, -1, 2**31 - 1):
        with pytest.raises(ValueError):
            go.match_pair(a, b, E, kind, 1.0)


@pytest.mark.parametrize("seed", range(4))
def test_no_feature_twice_and_a_pair_depends_on_its_own_inputs(seed):
    images = _images(300 + seed, values=None if seed % 2 else [0, 1, 3, 7, 15])
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    Q = len(pairs)
    kinds = [gc.KIND_CYCLE[q % 2] for q in range(Q)]
    models = np.array([gc.motion_model(("bench", "plane_bench")[q % 2], kinds[q]) for q in range(Q)])
    thresholds = [1e-3 if q % 3 else np.inf for q in range(Q)]
    total = 0
    for ratio in (None, 0.8, 1.0):
        matches, distances = go.match_graph(images, pairs, models, kinds, thresholds, 256, ratio, True)
        for m, d in zip(matches, distances):
            assert m.dtype == np.int64 and m.shape == (len(d), 2) and np.all(np.diff(m[:, 0]) > 0)
            assert len(np.unique(m[:, 1])) == len(m)
            total += len(m)
    assert total > 50
    full, _ = go.match_graph(images, pairs, models, kinds, thresholds, 256, 0.8, True)
    q = pairs.index((2, 0))
    alone, _ = go.match_graph(images, [(2, 0)], models[q:q + 1], kinds[q:q + 1], thresholds[q:q + 1], 256, 0.8, True)
    assert np.array_equal(alone[0], full[q])


def test_symbols_are_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native, build, device
    from structure_from_motion_amd.feature_matching import guided_matching

    lib = _native.load()
    assert "sfm_match_pairs_guided" in _native.SIGNATURES and len(_native.SIGNATURES["sfm_match_pairs_guided"]) == 21
    assert hasattr(lib, "sfm_match_pairs_guided") and "sfm_match_pairs.hip" in build.SOURCES
    assert callable(device.match_pairs_guided)
    assert callable(guided_matching.guided_match_models) and callable(guided_matching.guided_match_pairs)
    parameters = inspect.signature(guided_matching.guided_match_models).parameters
    assert list(parameters)[:7] == ["descriptors", "features", "camera_matrix", "pairs", "models", "kinds", "thresholds"]
    assert {k: parameters[k].default for k in ("max_distance", "ratio", "cross_check", "max_pairs_per_call")} == \
        dict(max_distance=64, ratio=0.8, cross_check=True, max_pairs_per_call=65535)
    assert all(parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("max_distance", "ratio", "cross_check"))
    assert inspect.signature(guided_matching.guided_match_pairs).parameters["use_pose"].default is False
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header and lib.sfm_abi_version() == 15
    declaration = header[header.index("int sfm_match_pairs_guided("):]
    declaration = " ".join(declaration[:declaration.index(";")].split())
    for text in ("const double* xy", "const double* model", "const int32_t* model_kind", "const double* threshold",
                 "const sfm_match_pairs_options* options", "void* stream)"):
        assert text in declaration
    assert "tests/guided_matching_oracle.py" in header


def test_c_abi_refuses_bad_arguments_without_a_gpu(native_lib):
    from structure_from_motion_amd import _native

    lib = _native.load()
    ws = lib.sfm_match_pairs_workspace_bytes
    buf = (C.c_int64 * 64)()   # host memory: a refused call never touches it
    base = C.addressof(buf)
    base += (-base) % 16
    dummy = C.c_void_p(base)
    good = _native.MatchPairsOptions(64, 1, 1, 0, 0.8)
    call = lib.sfm_match_pairs_guided

    def refused(images=2, features=8, pairs=1, rows=4, max_n=4, image_offset=dummy, desc=dummy, ok=dummy, xy=dummy,
                pair_images=dummy, row_offset=dummy, model=dummy, kind=dummy, threshold=dummy, options=good, partner=dummy,
                distance=dummy, pair_status=dummy, workspace=dummy, workspace_bytes=1 << 20):
        return call(images, features, pairs, rows, max_n, image_offset, desc, ok, xy, pair_images, row_offset, model, kind,
                    threshold, None if options is None else C.byref(options), partner, distance, pair_status, workspace,
                    workspace_bytes, None) == EINVAL

    # sizes
    for name in ("images", "features", "pairs", "rows", "max_n"):
        assert refused(**{name: -1}), name
    assert refused(pairs=65536)
    assert refused(features=2**31) and refused(rows=2**31) and refused(max_n=2**31) and refused(images=2**31 - 1)
    assert refused(pairs=0, rows=4) and b"sfm_match_pairs_guided: rows without pairs" in lib.sfm_last_error()
    # null pointers
    for name in ("image_offset", "desc", "ok", "xy", "pair_images", "row_offset", "model", "kind", "threshold", "options",
                 "partner", "distance", "pair_status", "workspace"):
        assert refused(**{name: None}), name
    # alignment
    assert refused(desc=C.c_void_p(base + 8)) and refused(workspace=C.c_void_p(base + 8))
    assert refused(row_offset=C.c_void_p(base + 4)) and refused(partner=C.c_void_p(base + 2))
    assert refused(image_offset=C.c_void_p(base + 1)) and refused(pair_status=C.c_void_p(base + 2))
    assert refused(xy=C.c_void_p(base + 4)) and b"8-byte" in lib.sfm_last_error()
    assert refused(model=C.c_void_p(base + 4)) and refused(threshold=C.c_void_p(base + 4)) and refused(kind=C.c_void_p(base + 2))
    # options
    M = _native.MatchPairsOptions
    for bad in (M(-1, 1, 1, 0, 0.8), M(257, 1, 1, 0, 0.8), M(64, 2, 1, 0, 0.8), M(64, 1, 2, 0, 0.8), M(64, 1, 1, 1, 0.8),
                M(64, 1, 1, 0, 0.0), M(64, 1, 1, 0, -0.5), M(64, 1, 1, 0, float("nan")), M(64, 1, 1, 0, float("inf"))):
        assert refused(options=bad)
    assert refused(options=M(64, 1, 1, 7, 0.8)) and b"reserved" in lib.sfm_last_error()
    # workspace: the layout is sfm_match_pairs's
    assert refused(workspace_bytes=ws(1, 4, 4) - 1) and b"workspace" in lib.sfm_last_error()
    # no pairs: nothing to do, nothing touched
    assert call(2, 8, 0, 0, 4, dummy, dummy, dummy, dummy, None, None, None, None, None, C.byref(good), None, None, None, None, 0,
                None) == 0
    # the unguided entry point keeps its own name in its messages
    assert lib.sfm_match_pairs(2, 8, 0, 4, 4, dummy, dummy, dummy, dummy, dummy, C.byref(good), dummy, dummy, dummy, dummy, 1 << 20,
                               None) == EINVAL
    assert lib.sfm_last_error() == b"sfm_match_pairs: rows without pairs"


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*_a, **_k):
        raise AssertionError("device work before the checks")

    monkeypatch.setattr(device, "require_gpu", no_device)


K = synthetic.BENCH_K


def _good():
    rng = np.random.default_rng(0)
    descriptors = [(rng.integers(0, 256, (n, 32), dtype=np.uint8), np.ones(n, bool)) for n in (3, 2, 0)]
    features = [rng.uniform(0, 400, (n, 2)) for n in (3, 2, 0)]
    return dict(descriptors=descriptors, features=features, camera_matrix=K, pairs=[(0, 1)], models=np.eye(3)[None],
                kinds=["homography"], thresholds=1e-5)


def test_guided_match_models_rejects_bad_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd.feature_matching.guided_matching import guided_match_models

    _no_device(monkeypatch)
    good = _good()
    value_errors = [
        dict(pairs=[(0, 0)]), dict(pairs=[(0, 3)]), dict(pairs=[(-1, 1)]), dict(pairs=[(0, 1, 2)]), dict(pairs=[(0.0, 1.0)]),
        dict(max_distance=-1), dict(max_distance=257), dict(max_distance=6.0), dict(ratio=0.0), dict(ratio=float("nan")),
        dict(max_pairs_per_call=0), dict(max_pairs_per_call=65536),
        dict(camera_matrix=np.eye(4)), dict(camera_matrix=np.zeros((3, 3))), dict(camera_matrix=np.full((3, 3), np.nan)),
        dict(features=good["features"][:2]),                                        # one entry per image
        dict(features=[good["features"][0][:2], good["features"][1], good["features"][2]]),   # not the descriptors' length
        dict(features=[np.zeros((3, 3)), good["features"][1], good["features"][2]]),           # not (n, 2)
        dict(models=np.eye(3)), dict(models=np.zeros((2, 3, 3))), dict(models=np.zeros((1, 9))),
        dict(kinds=[]), dict(kinds=["essential", "none"]), dict(kinds=["fundamental"]), dict(kinds=[3]), dict(kinds=[-1]),
        dict(thresholds=[1e-5, 1e-5]), dict(thresholds=np.zeros((1, 1))),
    ]
    for change in value_errors:
        with pytest.raises(ValueError):
            guided_match_models(**{**good, **change})
    type_errors = [
        dict(descriptors=[np.zeros((3, 32), np.uint8)] * 3), dict(ratio="0.8"), dict(cross_check=1),
        dict(kinds="homography"), dict(kinds=[1.0]), dict(kinds=[True]), dict(kinds=[None]),
        dict(thresholds="1e-5"), dict(thresholds=[True]),
    ]
    for change in type_errors:
        with pytest.raises(TypeError):
            guided_match_models(**{**good, **change})
    with pytest.raises(TypeError):
        guided_match_models(*good.values(), 64)                                     # the options are keyword-only


class _Graph:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def test_guided_match_pairs_rejects_bad_arguments_and_forms_the_models(monkeypatch):
    from structure_from_motion_amd.feature_matching.guided_matching import essential_from_pose, graph_models, guided_match_pairs

    _no_device(monkeypatch)
    good = _good()
    args = (good["descriptors"], good["features"], K)
    rng = np.random.default_rng(1)
    E, H = rng.normal(size=(3, 3, 3)), rng.normal(size=(3, 3, 3))
    R = np.array([gc.motion_model(n, go.KIND_HOMOGRAPHY) for n in ("pan10", "gen12", "pan10")])
    t = rng.normal(size=(3, 3))
    pose = _Graph(R=R, t=t, status=["ok", "no_vote", "ok"])
    graph = _Graph(pairs=np.array([(0, 1), (1, 0), (0, 2)]), kind=["essential", "essential", "homography"], E=E, H=H, pose=pose)
    models, kinds = graph_models(graph)
    assert kinds == graph.kind and np.array_equal(models[:2], E[:2]) and np.array_equal(models[2], H[2])
    models, _ = graph_models(graph, use_pose=True)
    want = essential_from_pose(R, t)
    assert np.array_equal(models[0], want[0]) and np.array_equal(models[1], E[1]) and np.array_equal(models[2], H[2])
    # each entry two products and one subtraction
    assert want[0, 0, 1] == t[0, 1] * R[0, 2, 1] - t[0, 2] * R[0, 1, 1] and want[0, 2, 0] == t[0, 0] * R[0, 1, 0] - t[0, 1] * R[0, 0, 0]
    assert np.allclose(want[0], gc.skew(t[0]) @ R[0], rtol=0, atol=1e-15)
    none = _Graph(pairs=graph.pairs, kind=["none"] * 3, E=E, H=H)
    assert np.isnan(graph_models(none)[0]).all()
    with pytest.raises(TypeError):
        guided_match_pairs(*args, object(), 1e-5)
    with pytest.raises(TypeError):
        guided_match_pairs(*args, graph, 1e-5, use_pose=1)
    with pytest.raises(ValueError):
        guided_match_pairs(*args, _Graph(pairs=graph.pairs, kind=graph.kind, E=E, H=H, pose=None), 1e-5, use_pose=True)
    with pytest.raises(ValueError):
        guided_match_pairs(*args, _Graph(pairs=graph.pairs, kind=graph.kind, E=E[:2], H=H), 1e-5)
    with pytest.raises(ValueError):
        guided_match_pairs(*args, graph, [1e-5, 1e-5])                              # one threshold per pair, or one
    with pytest.raises(ValueError):
        guided_match_pairs(*args, _Graph(pairs=graph.pairs, kind=["essential", "fundamental", "none"], E=E, H=H), 1e-5)
    with pytest.raises(ValueError):
        guided_match_pairs(*args, graph, 1e-5, max_distance=300)


def test_no_pairs_and_empty_first_images_need_no_device(monkeypatch):
    from structure_from_motion_amd.feature_matching.graph_matching import PairMatches
    from structure_from_motion_amd.feature_matching.guided_matching import guided_match_models, guided_match_pairs

    _no_device(monkeypatch)
    good = _good()
    r = guided_match_models(good["descriptors"], good["features"], K, [], np.zeros((0, 3, 3)), [], 1e-5)
    assert isinstance(r, PairMatches) and r.pairs.shape == (0, 2) and r.matches == [] and r.distances == []
    r = guided_match_models(good["descriptors"], good["features"], K, [], [], [], [])
    assert r.matches == []
    r = guided_match_models(good["descriptors"], good["features"], K, np.array([[2, 0], [2, 1]], dtype=np.int32),
                            np.zeros((2, 3, 3)), [1, 0], [1e-5, np.nan])
    assert r.pairs.dtype == np.int64 and r.pairs.tolist() == [[2, 0], [2, 1]]
    assert [m.shape for m in r.matches] == [(0, 2)] * 2 and all(m.dtype == np.int64 for m in r.matches)
    assert [d.shape for d in r.distances] == [(0,)] * 2 and all(d.dtype == np.int32 for d in r.distances)
    empty = _Graph(pairs=np.zeros((0, 2), np.int64), kind=[], E=np.zeros((0, 3, 3)), H=np.zeros((0, 3, 3)))
    assert guided_match_pairs(good["descriptors"], good["features"], K, empty, 1e-5).matches == []


def test_normalized_coordinates_are_the_normalize_kernels():
    from structure_from_motion_amd.feature_matching.guided_matching import normalized_coordinates

    pixels = np.random.default_rng(3).uniform(0, 600, (50, 2))
    got = normalized_coordinates(K, pixels)
    assert np.array_equal(got, orc.to_normalized_image_coords(pixels, K)[:, :2])
    assert np.array_equal(got[:, 0], (pixels[:, 0] - K[0, 2]) / K[0, 0]) and got.flags.c_contiguous


def test_repeated_structure_views():
    views, points, unique, groups, extra = 3, 90, 50, 8, 11
    sc = synthetic.repeated_structure_views(views, points, unique, groups, extra, seed=5)
    again = synthetic.repeated_structure_views(views, points, unique, groups, extra, seed=5)
    other = synthetic.repeated_structure_views(views, points, unique, groups, extra, seed=6)
    base = synthetic.multi_view_scene(views, points, 5, 0.5, 0.0, 5.0)
    assert np.array_equal(sc["K"], synthetic.BENCH_K) and np.array_equal(sc["poses_true"], base["poses_true"])
    assert len(sc["pixels"]) == len(sc["descriptors"]) == len(sc["ids"]) == views
    prototypes = {}
    for v in range(views):
        pix, (bits, valid), ids = sc["pixels"][v], sc["descriptors"][v], sc["ids"][v]
        n = len(ids)
        assert pix.shape == (n, 2) and pix.dtype == np.float64 and bits.shape == (n, 32) and bits.dtype == np.uint8
        assert valid.shape == (n,) and valid.dtype == np.bool_ and valid.all() and ids.dtype == np.int64
        assert np.array_equal(pix, again["pixels"][v]) and np.array_equal(bits, again["descriptors"][v][0])
        assert np.array_equal(ids, again["ids"][v]) and not np.array_equal(bits[:20], other["descriptors"][v][0][:20])
        assert np.count_nonzero(ids == -1) == extra
        seen = base["point_indices"][base["camera_indices"] == v]
        assert sorted(ids[ids >= 0].tolist()) == sorted(seen.tolist())            # every observation once, no outliers
        order = np.argsort(ids[ids >= 0])
        assert not np.array_equal(order, np.arange(len(order)))                    # shuffled
        assert np.array_equal(pix[ids >= 0][order], base["pixels"][base["camera_indices"] == v][np.argsort(seen)])
        for k, b in zip(ids.tolist(), bits):
            if k >= 0:
                prototypes.setdefault(k, []).append(b)
    # observations of one point are within 2 * flips bits of each other; look-alikes of a group too; strangers are far
    def distance(x, y):
        return int(gmo.distances(x[None], y[None])[0, 0])
    first = {k: v[0] for k, v in prototypes.items()}
    assert all(distance(v[0], w) <= 40 for v in prototypes.values() for w in v[1:])
    alike = [k for k in first if k >= unique]
    for k in alike:
        for m in alike:
            same_group = (k - unique) % groups == (m - unique) % groups
            assert (distance(first[k], first[m]) <= 40) == same_group
    assert all(distance(first[k], first[m]) > 64 for k in first for m in first if k < m and k < unique)
    with pytest.raises(ValueError):
        synthetic.repeated_structure_views(3, 90, 91, 8, 11, seed=5)
    with pytest.raises(ValueError):
        synthetic.repeated_structure_views(3, 90, 50, 0, 11, seed=5)


def test_lib_reexport():
    from lib.feature_matching import guided_matching as lib_gm
    from structure_from_motion_amd.feature_matching import guided_matching as gm

    assert lib_gm.guided_match_models is gm.guided_match_models and lib_gm.guided_match_pairs is gm.guided_match_pairs


@pytest.mark.parametrize("seed", (21, 22))
def test_accuracy_conditions_on_the_numpy_chain(seed):
    """With the true essential matrices at 6e-6, on each of the twelve ordered pairs: strictly more right matches than the first
    pass, at no lower precision.  The figures of DESIGN.md section 6ad."""
    chain = gc.repeated_chain(seed)
    assert len(chain["rows"]) == 12
    for (i, j), (common, kept_1, right_1, kept_2, right_2) in zip(chain["pairs"].tolist(), chain["rows"]):
        print(f"seed {seed} pair {(i, j)}: common {common}, first pass {right_1} right of {kept_1}, guided {right_2} right of {kept_2}")
        assert right_2 > right_1
        assert right_2 / kept_2 >= right_1 / kept_1
        assert right_2 >= 0.97 * common > 0.7 * common >= right_1              # what DESIGN.md states for every pair
    for q in range(12):
        m = chain["guided"][q]
        assert len(np.unique(m[:, 0])) == len(m) == len(np.unique(m[:, 1]))


def test_the_stream_case_is_registered():
    import stream_cases

    case = stream_cases.CASES["match_pairs_guided"]
    assert case.entries == ("sfm_match_pairs_guided",) and case.ops == () and not case.synchronising
