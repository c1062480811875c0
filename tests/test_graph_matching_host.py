"""The graph matcher without a GPU: the NumPy definition against a plain double-loop restatement and its three properties,
the exports and bindings, the C ABI's refusals, the argument checks of the public API, the calls that need no device, the
generator, the lib re-export and the quality table of DESIGN.md section 6w."""
import ctypes as C
import os

import numpy as np
import pytest

import brief_oracle as bo
import graph_matching_oracle as gmo
from structure_from_motion_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h


def _small_descriptors(rng, n, values=None):
    """n descriptors that differ in their first byte only when ``values`` is given (ties everywhere), else random bits."""
    if values is None:
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    bits = np.zeros((n, 32), dtype=np.uint8)
    bits[:, 0] = rng.choice(values, n)
    return bits


def _double_loop(bits_a, valid_a, bits_b, valid_b, max_distance, ratio, cross_check):
    """The definition restated with loops over rows and columns and nothing else."""

    def d(a, b):
        return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(bits_a[a], bits_b[b]))

    def summary(n_self, n_other, valid_self, valid_other, dist):
        out = []
        for a in range(n_self):
            best = arg = second = None
            if valid_self[a]:
                for b in range(n_other):
                    if valid_other[b] and (best is None or dist(a, b) < best):
                        best, arg = dist(a, b), b
                for b in range(n_other):
                    if valid_other[b] and b != arg and (second is None or dist(a, b) < second):
                        second = dist(a, b)
            out.append((best, arg, second))
        return out

    def distinct(dist, runner_up):
        return ratio is None or runner_up is None or float(dist) <= ratio * float(runner_up)

    rows = summary(len(bits_a), len(bits_b), valid_a, valid_b, d)
    cols = summary(len(bits_b), len(bits_a), valid_b, valid_a, lambda b, a: d(a, b))
    partner, distance = [], []
    for a, (best, arg, second) in enumerate(rows):
        keep = best is not None and best <= max_distance and distinct(best, second)
        if keep and cross_check:
            keep = cols[arg][1] == a and distinct(best, cols[arg][2])
        partner.append(arg if keep else -1)
        distance.append(best if keep else -1)
    return np.array(partner, dtype=np.int32), np.array(distance, dtype=np.int32)


@pytest.mark.parametrize("seed", range(12))
def test_oracle_equals_the_double_loop(seed):
    rng = np.random.default_rng(seed)
    n_a, n_b = int(rng.integers(0, 7)), int(rng.integers(0, 8))            # at most 6 x 7
    values = None if seed % 3 == 0 else [0, 1, 3, 7]                        # distances 0 .. 3: ties for best and second
    bits_a, bits_b = _small_descriptors(rng, n_a, values), _small_descriptors(rng, n_b, values)
    valid_a, valid_b = rng.random(n_a) < 0.75, rng.random(n_b) < 0.75
    if seed == 5:
        valid_b[:] = False                                                  # no valid column at all
    if seed == 7 and n_b:
        valid_b[:] = False
        valid_b[0] = True                                                   # one valid column: no runner-up
    for max_distance in (0, 2, 256):
        for ratio in (None, 0.5, 0.8, 1.0):
            for cross_check in (False, True):
                want = _double_loop(bits_a, valid_a, bits_b, valid_b, max_distance, ratio, cross_check)
                got = gmo.match_pair(bits_a, valid_a, bits_b, valid_b, max_distance, ratio, cross_check)
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_oracle_named_cases():
    zero, one, three = np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8)
    one[0, 0], three[0, 0] = 1, 3
    yes = np.ones(1, bool)
    # a tie for the best: second == best, so every ratio below 1 refuses and ratio 1 keeps the smallest column
    b = np.concatenate([one, one])
    assert list(gmo.match_pair(zero, yes, b, np.ones(2, bool), 256, 0.99, False)[0]) == [-1]
    assert list(gmo.match_pair(zero, yes, b, np.ones(2, bool), 256, 1.0, False)[0]) == [0]
    # distance 0 against runner-up 0: 0 <= ratio * 0 holds
    assert list(gmo.match_pair(zero, yes, np.concatenate([zero, zero]), np.ones(2, bool), 0, 0.5, False)[1]) == [0]
    # the only valid column has no runner-up: distinctive whatever the ratio; an invalid one is nobody's runner-up
    assert list(gmo.match_pair(zero, yes, np.concatenate([three, zero]), np.array([True, False]), 256, 0.1, True)[0]) == [0]
    # an invalid row matches nothing and claims no column
    p, _ = gmo.match_pair(np.concatenate([zero, zero]), np.array([False, True]), zero, yes, 256, None, True)
    assert list(p) == [-1, 0]
    # cross-check: both rows' nearest is column 0, the column's nearest is row 1
    a = np.concatenate([three, one])
    assert list(gmo.match_pair(a, np.ones(2, bool), zero, yes, 256, None, False)[0]) == [0, 0]
    assert list(gmo.match_pair(a, np.ones(2, bool), zero, yes, 256, None, True)[0]) == [-1, 0]
    # ... and the column's side must be distinctive too: rows at distances 1 and 1 of it are not
    a = np.concatenate([one, one])
    assert list(gmo.match_pair(a, np.ones(2, bool), zero, yes, 256, 0.8, True)[0]) == [-1, -1]
    assert list(gmo.match_pair(a, np.ones(2, bool), zero, yes, 256, 0.8, False)[0]) == [0, 0]


@pytest.mark.parametrize("seed", range(6))
def test_transposition_and_no_duplicates(seed):
    rng = np.random.default_rng(100 + seed)
    values = None if seed % 2 else [0, 1, 3, 7, 15]
    images = []
    for n in (23, 0, 40, 17):
        images.append((_small_descriptors(rng, n, values), rng.random(n) < 0.8))
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    for ratio in (None, 0.8, 1.0):
        for max_distance in (2, 256):
            matches, distances = gmo.match_graph(images, pairs, max_distance, ratio, True)
            by_pair = dict(zip(pairs, zip(matches, distances)))
            for (i, j), (m, d) in by_pair.items():
                assert m.dtype == np.int64 and m.shape == (len(d), 2)
                assert np.all(np.diff(m[:, 0]) > 0)                                     # ascending a
                assert len(np.unique(m[:, 1])) == len(m)                                # no feature twice
                back, back_d = by_pair[j, i]
                order = np.argsort(m[:, 1], kind="stable")
                assert np.array_equal(m[order][:, ::-1], back) and np.array_equal(d[order], back_d)
    # the result of a pair depends on its two images alone
    alone, _ = gmo.match_graph(images, [(2, 0)], 256, 0.8, True)
    full, _ = gmo.match_graph(images, pairs, 256, 0.8, True)
    assert np.array_equal(alone[0], full[pairs.index((2, 0))])


def test_symbols_are_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native, build, device
    from structure_from_motion_amd.feature_matching import graph_matching

    lib = _native.load()
    assert "sfm_match_pairs" in _native.SIGNATURES and len(_native.SIGNATURES["sfm_match_pairs"]) == 17
    assert "sfm_match_pairs_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(lib, "sfm_match_pairs") and hasattr(lib, "sfm_match_pairs_workspace_bytes")
    assert "sfm_match_pairs.hip" in build.SOURCES
    assert C.sizeof(_native.MatchPairsOptions) == 24
    assert callable(device.match_pairs) and callable(graph_matching.match_image_pairs)
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header and _native.ABI_VERSION == 15 and lib.sfm_abi_version() == 15
    for name in ("sfm_match_pairs_options", "sfm_match_pairs_workspace_bytes", "int sfm_match_pairs("):
        assert name in header
    options = device.match_pairs_options(64, None, True)
    assert (options.max_distance, options.cross_check, options.use_ratio, options.reserved) == (64, 1, 0, 0)
    assert device.match_pairs_options(3, 0.75, False).ratio == 0.75


def test_c_abi_refuses_bad_arguments_without_a_gpu(native_lib):
    from structure_from_motion_amd import _native

    lib = _native.load()
    ws = lib.sfm_match_pairs_workspace_bytes
    assert ws(0, 0, 0) > 0 and ws(57, 120000, 1030) >= 4 * (3 * 120000 + 2 * 57 * 1030)
    for args in [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (65536, 0, 0), (1, 2**31, 1), (1, 1, 2**31)]:
        assert ws(*args) == -1
    buf = (C.c_int64 * 64)()   # host memory, 16-byte aligned or not: a refused call never touches it
    base = C.addressof(buf)
    base += (-base) % 16
    dummy = C.c_void_p(base)
    good = _native.MatchPairsOptions(64, 1, 1, 0, 0.8)
    call = lib.sfm_match_pairs

    def refused(images=2, features=8, pairs=1, rows=4, max_n=4, image_offset=dummy, desc=dummy, ok=dummy, pair_images=dummy,
                row_offset=dummy, options=good, partner=dummy, distance=dummy, pair_status=dummy, workspace=dummy,
                workspace_bytes=1 << 20):
        return call(images, features, pairs, rows, max_n, image_offset, desc, ok, pair_images, row_offset,
                    None if options is None else C.byref(options), partner, distance, pair_status, workspace, workspace_bytes,
                    None) == EINVAL

    # sizes
    for name in ("images", "features", "pairs", "rows", "max_n"):
        assert refused(**{name: -1}), name
    assert refused(pairs=65536)
    assert refused(features=2**31) and refused(rows=2**31) and refused(max_n=2**31) and refused(images=2**31 - 1)
    assert refused(pairs=0, rows=4) and b"rows without pairs" in lib.sfm_last_error()
    # null pointers
    for name in ("image_offset", "desc", "ok", "pair_images", "row_offset", "options", "partner", "distance", "pair_status",
                 "workspace"):
        assert refused(**{name: None}), name
    # alignment
    assert refused(desc=C.c_void_p(base + 8)) and refused(workspace=C.c_void_p(base + 8))
    assert refused(row_offset=C.c_void_p(base + 4)) and refused(partner=C.c_void_p(base + 2))
    assert refused(image_offset=C.c_void_p(base + 1)) and refused(pair_status=C.c_void_p(base + 2))
    # options
    M = _native.MatchPairsOptions
    for bad in (M(-1, 1, 1, 0, 0.8), M(257, 1, 1, 0, 0.8), M(64, 2, 1, 0, 0.8), M(64, 1, 2, 0, 0.8), M(64, 1, 1, 1, 0.8),
                M(64, 1, 1, 0, 0.0), M(64, 1, 1, 0, -0.5), M(64, 1, 1, 0, float("nan")), M(64, 1, 1, 0, float("inf"))):
        assert refused(options=bad)
    assert refused(options=M(64, 1, 1, 7, 0.8)) and b"reserved" in lib.sfm_last_error()
    # workspace
    assert refused(workspace_bytes=ws(1, 4, 4) - 1) and b"workspace" in lib.sfm_last_error()
    # no pairs: nothing to do, nothing touched
    assert call(2, 8, 0, 0, 4, dummy, dummy, dummy, None, None, C.byref(good), None, None, None, None, 0, None) == 0


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*_a, **_k):
        raise AssertionError("device work before the checks")

    monkeypatch.setattr(device, "require_gpu", no_device)


def test_public_api_rejects_bad_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd.feature_matching.graph_matching import match_image_pairs

    _no_device(monkeypatch)
    rng = np.random.default_rng(0)
    image = lambda n: (rng.integers(0, 256, (n, 32), dtype=np.uint8), np.ones(n, bool))   # noqa: E731
    good = [image(3), image(2), image(0)]
    value_errors = [
        (good, [(0, 0)], {}),                                                  # equal images
        (good, [(0, 3)], {}),                                                  # image out of range
        (good, [(-1, 1)], {}),
        (good, [(0, 1, 2)], {}),                                               # wrong shape
        (good, [(0.0, 1.0)], {}),                                              # not integers
        ([(np.zeros((3, 31), np.uint8), np.ones(3, bool))], [], {}),           # descriptors not (n, 32)
        ([(np.zeros((3, 32), np.uint8), np.ones(2, bool))], [], {}),           # flags not (n,)
        ([(np.zeros((2, 3, 32), np.uint8), np.ones(2, bool))], [], {}),
        (good, [(0, 1)], dict(max_distance=-1)),
        (good, [(0, 1)], dict(max_distance=257)),
        (good, [(0, 1)], dict(max_distance=6.0)),
        (good, [(0, 1)], dict(max_distance=True)),
        (good, [(0, 1)], dict(ratio=0.0)),
        (good, [(0, 1)], dict(ratio=-1.0)),
        (good, [(0, 1)], dict(ratio=float("nan"))),
        (good, [(0, 1)], dict(ratio=float("inf"))),
        (good, [(0, 1)], dict(max_pairs_per_call=0)),
        (good, [(0, 1)], dict(max_pairs_per_call=65536)),
        (good, [(0, 1)], dict(max_pairs_per_call=2.0)),
    ]
    for descriptors, pairs, options in value_errors:
        with pytest.raises(ValueError):
            match_image_pairs(descriptors, pairs, **options)
    type_errors = [
        ([(np.zeros((3, 32), np.int32), np.ones(3, bool))], [], {}),           # bits not uint8
        ([(np.zeros((3, 32), np.uint8), np.ones(3, np.float64))], [], {}),     # flags neither bool nor integer
        ([np.zeros((3, 32), np.uint8)], [], {}),                                # not a (bits, valid) pair
        (good, [(0, 1)], dict(ratio="0.8")),
        (good, [(0, 1)], dict(ratio=True)),
        (good, [(0, 1)], dict(cross_check=1)),
        (good, [(0, 1)], dict(cross_check=None)),
    ]
    for descriptors, pairs, options in type_errors:
        with pytest.raises(TypeError):
            match_image_pairs(descriptors, pairs, **options)
    with pytest.raises(TypeError):
        match_image_pairs(good, [(0, 1)], 64)                                   # the options are keyword-only


def test_no_pairs_and_empty_first_images_need_no_device(monkeypatch):
    from structure_from_motion_amd.feature_matching.brief import BriefDescriptors
    from structure_from_motion_amd.feature_matching.graph_matching import PairMatches, match_image_pairs

    _no_device(monkeypatch)
    full = BriefDescriptors(np.zeros((4, 32), np.uint8), np.ones(4, bool), np.zeros(4, np.uint8))
    none = (np.zeros((0, 32), np.uint8), np.zeros(0, bool))
    r = match_image_pairs([full, none], [])
    assert isinstance(r, PairMatches) and r.pairs.shape == (0, 2) and r.matches == [] and r.distances == []
    r = match_image_pairs([full, none, none], np.array([[1, 0], [2, 0], [1, 2]], dtype=np.int32))
    assert r.pairs.dtype == np.int64 and r.pairs.tolist() == [[1, 0], [2, 0], [1, 2]]
    assert [m.shape for m in r.matches] == [(0, 2)] * 3 and all(m.dtype == np.int64 for m in r.matches)
    assert [d.shape for d in r.distances] == [(0,)] * 3 and all(d.dtype == np.int32 for d in r.distances)


def test_call_bounds_and_all_pairs():
    from structure_from_motion_amd.feature_matching import graph_matching as gm

    assert gm.all_pairs(0).shape == (0, 2) and gm.all_pairs(1).shape == (0, 2)
    p = gm.all_pairs(4)
    assert p.dtype == np.int64 and p.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError):
            gm.all_pairs(bad)
    sizes = np.array([5, 0, 9, 2])
    assert gm.call_bounds(sizes, p, 65535) == [(0, 6)]
    assert gm.call_bounds(sizes, p, 4) == [(0, 4), (4, 6)]
    assert gm.call_bounds(sizes, p, 1) == [(q, q + 1) for q in range(6)]
    assert gm.call_bounds(sizes, p[:0], 3) == []
    # the column summaries of a call are bounded too: pairs x the largest image it names
    big = np.array([gm.MAX_COLUMN_SLOTS_PER_CALL // 2, 1, gm.MAX_COLUMN_SLOTS_PER_CALL])
    assert gm.call_bounds(big, np.array([[0, 1], [1, 0], [1, 0], [2, 1], [1, 0]]), 65535) == [(0, 2), (2, 3), (3, 4), (4, 5)]


def test_rotated_texture_views():
    degrees = (0.0, 17.0, 133.0)
    images, feats, ids = synthetic.rotated_texture_views(96, 128, degrees, 40, 7, seed=3)
    again = synthetic.rotated_texture_views(96, 128, degrees, 40, 7, seed=3)
    assert len(images) == len(feats) == len(ids) == 3
    cx, cy = (128 - 1) / 2.0, (96 - 1) / 2.0
    latent = None
    for v, (image, f, i, d) in enumerate(zip(images, feats, ids, degrees)):
        assert image.shape == (96, 128) and image.dtype == np.uint8 and np.array_equal(image, again[0][v])
        assert f.shape == (47, 2) and f.dtype == np.float64 and i.shape == (47,) and i.dtype == np.int64
        assert np.array_equal(f, again[1][v]) and np.array_equal(i, again[2][v])
        assert sorted(i[i >= 0]) == list(range(40)) and np.count_nonzero(i == -1) == 7
        assert np.all(f[:, 0] >= 20) and np.all(f[:, 0] <= 128 - 1 - 20) and np.all(f[:, 1] >= 20) and np.all(f[:, 1] <= 96 - 1 - 20)
        alone = f[i == -1]
        assert np.array_equal(alone, np.round(alone))
        # back to the unrotated frame: every view sees the same latent points
        seen = f[i >= 0][np.argsort(i[i >= 0])]
        c, s = np.cos(np.deg2rad(d)), np.sin(np.deg2rad(d))
        base = np.column_stack([cx + c * (seen[:, 0] - cx) - s * (seen[:, 1] - cy), cy + s * (seen[:, 0] - cx) + c * (seen[:, 1] - cy)])
        latent = base if latent is None else latent
        assert np.allclose(base, latent, atol=1e-9)
    assert np.array_equal(latent, np.round(latent))
    # the views show one texture: the descriptors of a latent point agree across views far better than chance (128 bits)
    bits = [bo.describe(image, f)[0][np.argsort(np.where(i >= 0, i, 10**6))][:40] for image, f, i in zip(images, feats, ids)]
    same = np.diagonal(gmo.distances(bits[0], bits[2]))
    assert np.median(same) < 64
    with pytest.raises(ValueError):
        synthetic.rotated_texture_views(40, 128, degrees, 4, 1, seed=3)


def test_lib_reexport():
    from lib.feature_matching import graph_matching as lib_gm
    from structure_from_motion_amd.feature_matching import graph_matching as gm

    assert lib_gm.match_image_pairs is gm.match_image_pairs
    assert lib_gm.all_pairs is gm.all_pairs and lib_gm.PairMatches is gm.PairMatches


# (kept, precision, recall) of the best partner per row and of max_distance=64, ratio=0.8, cross_check=True on
# rotated_texture_pair(240, 320, degrees, 300, seed=7) plus 150 partnerless features per image: DESIGN.md section 6w
QUALITY = {
    0: ((450, 0.662, 0.993), (291, 0.993, 0.963)),
    7: ((450, 0.629, 0.943), (278, 0.975, 0.903)),
    17: ((450, 0.624, 0.937), (264, 0.989, 0.870)),
    45: ((450, 0.607, 0.910), (250, 0.988, 0.823)),
    90: ((450, 0.662, 0.993), (293, 1.000, 0.977)),
    133: ((450, 0.620, 0.930), (256, 0.996, 0.850)),
    180: ((450, 0.662, 0.993), (290, 0.993, 0.960)),
    251: ((450, 0.618, 0.927), (248, 0.988, 0.817)),
}


@pytest.mark.parametrize("degrees", sorted(QUALITY))
def test_validation_quality(degrees):
    image_a, image_b, pairs = synthetic.rotated_texture_pair(240, 320, degrees, 300, seed=7)
    rng = np.random.default_rng(1)
    extra_a = np.column_stack([rng.integers(20, 300, 150), rng.integers(20, 220, 150)]).astype(np.float64)
    extra_b = np.column_stack([rng.integers(20, 300, 150), rng.integers(20, 220, 150)]).astype(np.float64)
    bits_a, valid_a, _ = bo.describe(image_a, np.concatenate([pairs[:, :2], extra_a]))
    bits_b, valid_b, _ = bo.describe(image_b, np.concatenate([pairs[:, 2:], extra_b]))
    summaries = gmo.Summaries(bits_a, valid_a, bits_b, valid_b)

    def figures(**options):
        partner, _ = gmo.decide(summaries, **options)
        kept, right = int(np.count_nonzero(partner >= 0)), int(np.count_nonzero(partner[:300] == np.arange(300)))
        return kept, right / kept, right / 300

    raw = figures(max_distance=256, ratio=None, cross_check=False)
    validated = figures(max_distance=64, ratio=0.8, cross_check=True)
    print(degrees, "raw", raw, "validated", validated)
    table_raw, table_validated = QUALITY[degrees]
    assert raw[0] == table_raw[0] and validated[0] == table_validated[0]
    assert (round(raw[1], 3), round(raw[2], 3)) == table_raw[1:]
    assert (round(validated[1], 3), round(validated[2], 3)) == table_validated[1:]
    assert validated[1] >= table_validated[1] - 0.03
    assert validated[1] > raw[1]
