"""The multi-scale keypoint detector without a GPU: the NumPy definition (tests/keypoint_oracle.py) against a per-pixel
double-loop restatement and exact rational arithmetic, its quota, tie and order rules, the exports and bindings, the C ABI's
refusals, the argument checks of the public API, the host's sort and trim, the call that needs no device, the generator, the lib
re-export and the quality table of DESIGN.md section 6x."""
import ctypes as C
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import graph_matching_oracle as gmo
import keypoint_oracle as ko
from structure_from_motion_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h


def _fast_loop(image, t):
    """FAST-9 corner test and score of every pixel, one pixel at a time."""
    H, W = image.shape
    out = np.zeros((H, W), dtype=np.uint16)
    for y in range(15, H - 15):
        for x in range(15, W - 15):
            p = int(image[y, x])
            ring = [int(image[y + dy, x + dx]) for dx, dy in ko.CIRCLE]
            brighter, darker = [v > p + t for v in ring], [v < p - t for v in ring]
            corner = any(all(mask[(start + k) % 16] for k in range(9)) for mask in (brighter, darker) for start in range(16))
            if corner:
                out[y, x] = max(sum(v - p - t for v, b in zip(ring, brighter) if b), sum(p - v - t for v, d in zip(ring, darker) if d))
    return out


def _suppress_loop(score):
    H, W = score.shape
    out = np.zeros((H, W), dtype=np.uint16)
    for y in range(H):
        for x in range(W):
            s = int(score[y, x])
            keep = s > 0
            for ny in (y - 1, y, y + 1):
                for nx in (x - 1, x, x + 1):
                    if (ny, nx) == (y, x):
                        continue
                    n = int(score[ny, nx]) if 0 <= ny < H and 0 <= nx < W else 0
                    keep = keep and (s > n if (ny, nx) < (y, x) else s >= n)
            out[y, x] = s if keep else 0
    return out


def _small_image(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(31, 41)), int(rng.integers(31, 45))                 # at most 40 x 44
    kind = seed % 4
    if kind == 0:
        image = rng.integers(0, 256, (H, W), dtype=np.uint8)
    elif kind == 1:
        image = rng.choice(np.array([0, 255], dtype=np.uint8), (H, W), p=[0.35, 0.65])   # saturated: what t = 254 needs
    elif kind == 2:
        image = rng.choice(np.array([0, 1, 2, 254, 255], dtype=np.uint8), (H, W))        # differences of 1 and 2: what t = 1 needs
    else:
        image = np.tile(rng.integers(0, 256, (4, 4), dtype=np.uint8), (11, 12))[:H, :W]   # ties
    image = np.ascontiguousarray(image)
    y, x = int(rng.integers(15, H - 15)), int(rng.integers(15, W - 15))
    image[y - 3:y + 4, x - 3:x + 4] = 255 if seed % 2 else 0                     # one certain corner of the extreme kind
    image[y, x] = 0 if seed % 2 else 255
    return image


@pytest.mark.parametrize("seed", range(8))
def test_oracle_equals_the_double_loop(seed):
    image = _small_image(seed)
    found = 0
    for t in (1, 20, 254):
        score = ko.fast_scores(image, t)
        assert score.dtype == np.uint16 and np.array_equal(score, _fast_loop(image, t))
        kept = ko.suppress(score)
        assert kept.dtype == np.uint16 and np.array_equal(kept, _suppress_loop(score))
        assert score.max() <= 4064 and (t != 254 or set(np.unique(score)) <= {0, 9, 10, 11, 12, 13, 14, 15, 16})
        found += np.count_nonzero(kept)
        # no two survivors touch: what bounds the candidate list of a plane
        ys, xs = np.nonzero(kept)
        for y, x in zip(ys, xs):
            assert np.count_nonzero(kept[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]) == 1
    assert found > 0
    assert ko.fast_scores(image, 254).max() == 16                                # the planted corner: 16 x (255 - 0 - 254)


def test_fast_named_cases():
    image = np.full((31, 31), 100, dtype=np.uint8)                               # one testable pixel
    for k in range(9):
        dx, dy = ko.CIRCLE[(12 + k) % 16]                                        # an arc of 9 across the end of the circle's list
        image[15 + dy, 15 + dx] = 130
    assert ko.fast_scores(image, 20)[15, 15] == 9 * 10 and np.count_nonzero(ko.fast_scores(image, 20)) == 1
    assert ko.fast_scores(image, 29)[15, 15] == 9 and ko.fast_scores(image, 30)[15, 15] == 0    # strictly brighter
    dx, dy = ko.CIRCLE[0]
    image[15 + dy, 15 + dx] = 100                                                # 8 contiguous: no corner
    assert not ko.fast_scores(image, 20).any()
    image[15 + dy, 15 + dx] = 130
    image[15 + ko.CIRCLE[6][1], 15 + ko.CIRCLE[6][0]] = 0                        # a darker pixel elsewhere: the larger sum wins
    assert ko.fast_scores(image, 20)[15, 15] == max(90, 80)
    image[15 + ko.CIRCLE[7][1], 15 + ko.CIRCLE[7][0]] = 0
    assert ko.fast_scores(image, 20)[15, 15] == 160
    assert not ko.fast_scores(np.full((30, 200), 7, np.uint8), 1).any() and ko.fast_scores(np.zeros((30, 200), np.uint8), 1).shape == (30, 200)


def test_level_formula_is_exact_bilinear_sampling():
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 256, (61, 75), dtype=np.uint8)
    plane[:8, :8] = 255
    plane[8:16, :8] = 0
    level = ko.downsample(plane)
    assert level.shape == (48, 60) and level.dtype == np.uint8
    for y in range(level.shape[0]):
        for x in range(level.shape[1]):
            # pixel centres aligned: (x + 1/2) 5/4 - 1/2
            sx, sy = Fraction(5, 4) * (x + Fraction(1, 2)) - Fraction(1, 2), Fraction(5, 4) * (y + Fraction(1, 2)) - Fraction(1, 2)
            x0, y0 = sx.numerator // sx.denominator, sy.numerator // sy.denominator
            fx, fy = sx - x0, sy - y0
            exact = ((1 - fy) * ((1 - fx) * int(plane[y0, x0]) + fx * int(plane[y0, x0 + 1]))
                     + fy * ((1 - fx) * int(plane[y0 + 1, x0]) + fx * int(plane[y0 + 1, x0 + 1])))
            rounded = exact + Fraction(1, 2)
            assert int(level[y, x]) == rounded.numerator // rounded.denominator
    planes = ko.pyramid(plane, 8)
    assert [p.shape for p in planes] == [(61, 75), (48, 60)]                     # 38 x 48 would be too small
    assert [p.shape for p in ko.pyramid(plane, 1)] == [(61, 75)]
    assert ko.level_shapes(59, 61, 8) == [(59, 61)] and ko.level_shapes(60, 60, 8) == [(60, 60), (48, 48)]
    assert len(ko.level_shapes(10**6, 10**6, 12)) == 12


def test_no_sample_leaves_the_plane():
    for W in range(48, 4097):
        w = 4 * W // 5
        assert ((10 * (w - 1) + 1) >> 3) + 1 <= W - 1


def test_base_coordinates_are_exact():
    for level in range(12):
        for x in (0, 1, 15, 47, 1234, 4095, 2**20):
            exact = Fraction(x)
            for _ in range(level):
                exact = (10 * exact + 1) / 8                                       # one level down: ux / 8
            got = ko.base_xy([x], [x], [level])
            assert got.dtype == np.float64 and Fraction(float(got[0, 0])) == exact == Fraction(float(got[0, 1]))
            assert exact == Fraction(5, 4) ** level * (x + Fraction(1, 2)) - Fraction(1, 2)


def test_quotas():
    from structure_from_motion_amd.feature_matching import keypoints as kp

    for L in range(1, 13):
        for N in (1, 2, 7, 200, 1000, 12345, 2**31 - 1):
            q = ko.quotas(L, N)
            assert len(q) == L and sum(q) == N and all(a >= b for a, b in zip(q, q[1:])) and min(q) >= 0
            assert q == kp.level_quotas(L, N)
            weights = [Fraction(4, 5) ** l for l in range(L)]                     # the levels' side lengths
            for l in range(1, L):
                assert q[l] == int(N * weights[l] / sum(weights))
    assert ko.quotas(1, 9) == [9] and ko.quotas(8, 1) == [1, 0, 0, 0, 0, 0, 0, 0]


def test_tie_rule_and_order():
    score = np.zeros((5, 7), dtype=np.uint16)
    score[2, 2] = score[2, 3] = 50                                               # equal neighbours in a row: the earlier survives
    score[0, 5] = score[1, 6] = 40                                               # ... and on a diagonal
    score[4, 0] = 7
    score[4, 6] = 50
    kept = ko.suppress(score)
    assert sorted(zip(*np.nonzero(kept))) == [(0, 5), (2, 2), (4, 0), (4, 6)]
    score[3, 2] = 50                                                             # below (2, 2): later in raster order, loses
    assert sorted(zip(*np.nonzero(ko.suppress(score)))) == [(0, 5), (2, 2), (4, 0), (4, 6)]
    score[1, 1] = 50                                                             # before (2, 2): wins
    assert sorted(zip(*np.nonzero(ko.suppress(score)))) == [(0, 5), (1, 1), (4, 0), (4, 6)]
    x, y, s = ko.ordered_survivors(kept)
    assert list(zip(s, y, x)) == [(50, 2, 2), (50, 4, 6), (40, 0, 5), (7, 4, 0)]     # score down, then y, then x
    kept[2, 5] = 50
    assert list(zip(*ko.ordered_survivors(kept)))[:3] == [(2, 2, 50), (5, 2, 50), (6, 4, 50)]


@functools.lru_cache(maxsize=None)
def _scene():
    images = [synthetic.similarity_texture_views(h, w, [25.0], [1.0], seed)[0][0] for seed, (h, w) in enumerate([(90, 120), (64, 150)])]
    images.append(np.tile(np.random.default_rng(5).integers(0, 256, (8, 8), dtype=np.uint8), (12, 12)))   # 96 x 96, ties
    images.append(np.zeros((30, 40), np.uint8))
    return images


@pytest.mark.parametrize("num_features,levels", [(1, 8), (7, 3), (40, 8), (40, 1), (10**5, 8)])
def test_the_host_sorts_and_trims_like_the_definition(num_features, levels):
    """What the device leaves — every survivor at or above its plane's cutoff, in any order — through the host's half."""
    from structure_from_motion_amd.feature_matching import keypoints as kp

    images = _scene()
    maps = [ko.Maps(image, levels, 20) for image in images]
    layout = kp.plan([im.shape for im in images], num_features, levels)
    assert [r[1] for r in layout.rows] == sorted(r[1] for r in layout.rows)       # levels ascending
    assert [r[4] for r in layout.rows] == list(np.cumsum([0] + [r[2] * r[3] for r in layout.rows])[:-1])
    rows = []
    for p, (image, level, h, w, _, quota) in enumerate(layout.rows):
        assert maps[image].planes[level].shape == (h, w) and quota == ko.quotas(len(maps[image].planes), num_features)[level]
        x, y, s = maps[image].survivors[level]
        cutoff = 4096 if quota == 0 else 1 if len(s) < quota else int(s[quota - 1])   # the largest T with count(score >= T) >= quota
        keep = s >= cutoff
        assert len(x) <= kp._survivor_bound(h, w)
        rows += [(p, int(a), int(b), int(c)) for a, b, c in zip(x[keep], y[keep], s[keep])]
    rng = np.random.default_rng(num_features)
    candidates = np.array(rows, dtype=np.int32).reshape(-1, 4)[rng.permutation(len(rows))]
    want = [ko.describe(m, num_features) for m in maps]
    lookup = {}
    for i, w in enumerate(want):
        for j in range(len(w.xy)):
            lookup[(i, int(w.level[j]), int(w.level_xy[j, 0]), int(w.level_xy[j, 1]))] = (w.bits[j], w.angle_bin[j])
    bits = np.zeros((len(candidates), 32), np.uint8)
    bins = np.zeros(len(candidates), np.uint8)
    for k, (p, x, y, _) in enumerate(candidates.tolist()):
        entry = lookup.get((layout.rows[p][0], layout.rows[p][1], x, y))
        if entry is not None:                                                      # a tie beyond the quota: trimmed, never read
            bits[k], bins[k] = entry
    run = kp._Run(layout, None, None, None, len(candidates), len(candidates), 1, candidates, bits, np.ones(len(candidates), bool), bins)
    got = kp._assemble(run, len(images))
    assert len(got) == len(images)
    for g, w in zip(got, want):
        assert g.xy.dtype == np.float64 and g.xy.tobytes() == w.xy.tobytes() and g.xy.shape == (len(w.level), 2)
        assert g.level.dtype == np.uint8 and np.array_equal(g.level, w.level)
        assert g.score.dtype == np.int32 and np.array_equal(g.score, w.score)
        assert np.array_equal(g.descriptors.bits, w.bits) and np.array_equal(g.descriptors.angle_bin, w.angle_bin)
        assert np.all(g.descriptors.valid) and np.all(w.valid)
    assert len(got[3].xy) == 0 and (num_features > 1 or [len(g.xy) for g in got[:3]] == [1, 1, 1])


def test_symbols_are_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native, build, device
    from structure_from_motion_amd.feature_matching import keypoints

    lib = _native.load()
    assert "sfm_detect_keypoints" in _native.SIGNATURES and len(_native.SIGNATURES["sfm_detect_keypoints"]) == 20
    assert "sfm_detect_keypoints_workspace_bytes" in _native.OTHER_SYMBOLS
    assert hasattr(lib, "sfm_detect_keypoints") and hasattr(lib, "sfm_detect_keypoints_workspace_bytes")
    assert "sfm_keypoints.hip" in build.SOURCES and "sfm_brief_device.h" in build.HEADERS
    assert C.sizeof(_native.KeypointPlane) == 32 and C.sizeof(_native.KeypointCandidate) == 16
    assert callable(device.detect_keypoints) and callable(keypoints.detect_and_describe)
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header and _native.ABI_VERSION == 15 and lib.sfm_abi_version() == 15
    for name in ("sfm_keypoint_plane", "sfm_keypoint_candidate", "sfm_detect_keypoints_workspace_bytes", "int sfm_detect_keypoints("):
        assert name in header
    table = device.keypoint_plane_table([(0, 0, 60, 64, 0, 5), (0, 1, 48, 51, 3840, 3)])
    assert (table[1].image, table[1].level, table[1].height, table[1].width, table[1].offset, table[1].quota, table[1].reserved) == (
        0, 1, 48, 51, 3840, 3, 0)


def test_c_abi_refuses_bad_arguments_without_a_gpu(native_lib):
    from structure_from_motion_amd import _native, device

    lib = _native.load()
    ws = lib.sfm_detect_keypoints_workspace_bytes
    assert ws(0) > 0 and ws(3) >= 3 * 4096 * 4 and ws(65535) > 0
    assert ws(-1) == -1 and ws(65536) == -1
    buf = (C.c_int64 * 64)()   # host memory: a refused call never touches it
    base = C.addressof(buf)
    base += (-base) % 16
    dummy = C.c_void_p(base)
    good = [(0, 0, 60, 64, 0, 5), (1, 0, 48, 48, 3840, 2), (0, 1, 48, 51, 6144, 3)]
    pool_bytes = 6144 + 48 * 51
    call = lib.sfm_detect_keypoints

    def refused(rows=good, planes=None, images=2, pool=dummy, pool_bytes=pool_bytes, threshold=20, offsets=dummy, boundaries=dummy,
                bins=30, score=dummy, kept=dummy, capacity=64, counter=dummy, candidates=dummy, desc=dummy, ok=dummy,
                angle_bin=dummy, workspace=dummy, workspace_bytes=1 << 20, table="rows"):
        plane_table = device.keypoint_plane_table(rows) if isinstance(table, str) else table
        return call(plane_table, len(rows) if planes is None else planes, images, pool, pool_bytes, threshold, offsets, boundaries,
                    bins, score, kept, capacity, counter, candidates, desc, ok, angle_bin, workspace, workspace_bytes, None) == EINVAL

    # sizes and options
    for name in ("planes", "images", "pool_bytes", "capacity", "workspace_bytes"):
        assert refused(**{name: -1}), name
    assert refused(planes=65536) and refused(pool_bytes=2**31) and refused(capacity=2**31) and refused(images=2**31)
    assert refused(capacity=0)
    for t in (0, 255, -20):
        assert refused(threshold=t) and b"threshold" in lib.sfm_last_error()
    assert refused(bins=0) and refused(bins=65)
    # null pointers
    for name in ("pool", "offsets", "boundaries", "score", "kept", "counter", "candidates", "desc", "ok", "angle_bin", "workspace"):
        assert refused(**{name: None}), name
    assert refused(table=None)
    # alignment
    assert refused(candidates=C.c_void_p(base + 8)) and refused(workspace=C.c_void_p(base + 8))
    assert refused(desc=C.c_void_p(base + 4)) and refused(boundaries=C.c_void_p(base + 4)) and refused(offsets=C.c_void_p(base + 2))
    assert refused(score=C.c_void_p(base + 1)) and refused(kept=C.c_void_p(base + 1)) and refused(counter=C.c_void_p(base + 2))
    # workspace
    assert refused(workspace_bytes=ws(3) - 1) and b"workspace" in lib.sfm_last_error()
    # the plane table
    edit = lambda p, **fields: [tuple(fields.get(k, v) for k, v in zip(("image", "level", "height", "width", "offset", "quota"), r))  # noqa: E731
                                if i == p else r for i, r in enumerate(good)]
    assert refused(rows=edit(0, image=2)) and refused(rows=edit(0, image=-1))                # no such image
    assert refused(rows=edit(0, level=1)) and refused(rows=edit(2, level=2)) and refused(rows=edit(2, level=-1))
    assert refused(rows=[good[0], good[2], good[1]])                                         # levels must ascend
    assert refused(rows=edit(1, image=0))                                                    # two planes of one image and level
    assert refused(rows=edit(2, image=1))                                                    # 48 x 51 is not 4/5 of 48 x 48
    assert refused(rows=edit(2, height=47)) and refused(rows=edit(2, width=52))
    assert refused(rows=edit(0, height=0)) and refused(rows=edit(1, width=-3))
    assert refused(rows=[(0, 0, 59, 64, 0, 5), (0, 1, 47, 51, 3776, 3)], pool_bytes=10**4)   # a level below 48
    assert refused(rows=edit(1, offset=3839)) and b"overlap" in lib.sfm_last_error()         # into the plane before
    assert refused(rows=edit(2, offset=6143)) and refused(pool_bytes=pool_bytes - 1)
    assert refused(rows=edit(0, offset=-1))
    assert refused(rows=edit(1, quota=-1))
    table = device.keypoint_plane_table(good)
    table[1].reserved = 7
    assert refused(table=table) and b"reserved" in lib.sfm_last_error()
    levels = [(0, l, 48, 48, 48 * 48 * l, 1) for l in range(13)]                              # level 12
    assert refused(rows=levels, pool_bytes=10**6)


def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*_a, **_k):
        raise AssertionError("device work before the checks")

    monkeypatch.setattr(device, "require_gpu", no_device)


def test_public_api_rejects_bad_arguments_before_device_work(monkeypatch):
    from structure_from_motion_amd.feature_matching.keypoints import detect_and_describe

    _no_device(monkeypatch)
    good = [np.zeros((50, 60), np.uint8)]
    value_errors = [
        ([np.zeros((50, 60, 3), np.uint8)], {}),                                # colour
        ([np.zeros(50, np.uint8)], {}),
        ([np.zeros((0, 60), np.uint8)], {}),                                    # empty
        (good, dict(num_features=0)), (good, dict(num_features=-5)), (good, dict(num_features=10.0)), (good, dict(num_features=True)),
        (good, dict(num_features=2**31)),
        (good, dict(levels=0)), (good, dict(levels=13)), (good, dict(levels=2.0)), (good, dict(levels=None)),
        (good, dict(threshold=0)), (good, dict(threshold=255)), (good, dict(threshold=20.0)), (good, dict(threshold="20")),
        ([np.zeros((1, 2**30), np.uint8)] * 2, {}),                             # a pool of 2^31 pixels
    ]
    for images, options in value_errors:
        with pytest.raises(ValueError):
            detect_and_describe(images, **options)
    type_errors = [
        ([np.zeros((50, 60), np.float64)], {}),                                 # nothing is converted
        ([np.zeros((50, 60), np.int8)], {}), ([np.zeros((50, 60), bool)], {}), ([np.zeros((50, 60), np.uint16)], {}),
        ([[[0] * 60] * 50], {}),                                                # not an array
        (np.zeros((50, 60), np.uint8), {}),                                     # one image instead of a sequence
        (good + [None], {}),
    ]
    for images, options in type_errors:
        with pytest.raises(TypeError):
            detect_and_describe(images, **options)
    with pytest.raises(TypeError):
        detect_and_describe(good, 1000)                                         # the options are keyword-only


def test_an_empty_collection_needs_no_device(monkeypatch):
    from structure_from_motion_amd.feature_matching.keypoints import detect_and_describe

    _no_device(monkeypatch)
    assert detect_and_describe([]) == [] and detect_and_describe((), num_features=5, levels=1, threshold=254) == []


def test_plan_and_capacity():
    from structure_from_motion_amd.feature_matching import keypoints as kp

    assert kp.level_shapes(59, 61, 8) == ko.level_shapes(59, 61, 8) and kp.level_shapes(1080, 1920, 8) == ko.level_shapes(1080, 1920, 8)
    layout = kp.plan([(60, 60), (30, 200), (200, 263)], 1000, 8)
    assert [(r[0], r[1]) for r in layout.rows[:5]] == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1)]
    assert layout.pool_bytes == sum(r[2] * r[3] for r in layout.rows)
    bounds = [kp._survivor_bound(r[2], r[3]) for r in layout.rows]
    assert bounds[0] == 15 * 15 and bounds[1] == 0
    assert 1 <= layout.capacity <= sum(bounds)
    assert kp.plan([(30, 200)], 1000, 8).capacity == 1                          # never an empty buffer
    assert kp.plan([(2000, 2000)], 10, 1).capacity == 10 + kp.SLACK_PER_PLANE
    assert np.array_equal(kp.base_coordinates([[3, 4], [0, 0]], [2, 0]), ko.base_xy([3, 0], [4, 0], [2, 0]))


def test_similarity_texture_views():
    degrees, scales = (0.0, 90.0, 33.0), (1.0, 1.0, 1.6)
    images, to_canvas = synthetic.similarity_texture_views(96, 128, degrees, scales, seed=3, noise=0.0)
    again = synthetic.similarity_texture_views(96, 128, degrees, scales, seed=3, noise=0.0)
    other = synthetic.similarity_texture_views(96, 128, degrees, scales, seed=4, noise=0.0)
    assert len(images) == len(to_canvas) == 3
    cx, cy = (128 - 1) / 2.0, (96 - 1) / 2.0
    for v, (image, A, d, s) in enumerate(zip(images, to_canvas, degrees, scales)):
        assert image.shape == (96, 128) and image.dtype == np.uint8 and np.array_equal(image, again[0][v])
        assert not np.array_equal(image, other[0][v])
        assert A.shape == (2, 3) and A.dtype == np.float64 and np.array_equal(A, again[1][v])
        assert np.allclose(A[:, :2], s * np.array([[np.cos(np.deg2rad(d)), -np.sin(np.deg2rad(d))],
                                                   [np.sin(np.deg2rad(d)), np.cos(np.deg2rad(d))]]))
        assert np.allclose(A @ [cx, cy, 1.0], to_canvas[0] @ [cx, cy, 1.0])     # every view looks at the canvas centre
        assert image.min() < 80 and image.max() > 175                            # the stretch reaches the view
    # the map is what joins the views: a pixel of view 0 and the pixel of view v at the same canvas point show the same texture
    qx, qy = np.meshgrid(np.arange(30, 98, dtype=np.float64), np.arange(30, 66, dtype=np.float64))
    canvas = np.stack([qx.ravel(), qy.ravel(), np.ones(qx.size)]) * 1.0
    spot = to_canvas[0] @ canvas
    for v in (1, 2):
        A = to_canvas[v]
        back = np.linalg.solve(A[:, :2], spot - A[:, 2:3])
        bx, by = np.floor(back[0] + 0.5).astype(int), np.floor(back[1] + 0.5).astype(int)
        assert bx.min() >= 0 and bx.max() < 128 and by.min() >= 0 and by.max() < 96
        a = images[0][qy.ravel().astype(int), qx.ravel().astype(int)].astype(np.float64)
        b = images[v][by, bx].astype(np.float64)
        assert np.corrcoef(a, b)[0, 1] > 0.8 and abs(np.corrcoef(a, images[v][qy.ravel().astype(int), qx.ravel().astype(int)])[0, 1]) < 0.5
    noisy = synthetic.similarity_texture_views(96, 128, degrees, scales, seed=3)[0]
    assert 0.5 < np.std(noisy[0].astype(np.float64) - images[0]) < 4.0          # noise = 0.01: 2.55 grey levels
    for bad in (dict(height=40), dict(scales=(1.0, 1.0)), dict(scales=(1.0, 0.0, 2.0)), dict(scales=(1.0, -1.0, 2.0))):
        arguments = dict(height=96, width=128, degrees=degrees, scales=scales, seed=3)
        arguments.update(bad)
        with pytest.raises(ValueError):
            synthetic.similarity_texture_views(**arguments)


def test_lib_reexport():
    from lib.feature_matching import keypoints as lib_kp
    from structure_from_motion_amd.feature_matching import keypoints as kp

    assert lib_kp.detect_and_describe is kp.detect_and_describe and lib_kp.ImageKeypoints is kp.ImageKeypoints


# (kept, right) with one level and with eight levels against the view at scale 1.0, 0 degrees, of
# similarity_texture_views(480, 640, DEGREES, SCALES, seed=7) at num_features = 1000, threshold = 20 and match_pair's defaults:
# DESIGN.md section 6x
SCALES, DEGREES = (1.0, 1.0, 1.0, 1.25, 1.5, 2.0, 2.0), (0.0, 0.0, 45.0, 17.0, 45.0, 0.0, 133.0)
TABLE = {
    1: ((545, 542), (745, 745)),
    2: ((390, 388), (430, 427)),
    3: ((56, 45), (338, 335)),
    4: ((11, 1), (196, 192)),
    5: ((13, 0), (132, 127)),
    6: ((17, 0), (114, 110)),
}


def test_what_the_pyramid_buys():
    """Rows 4 (scale 1.5, 45 degrees) and 6 (scale 2.0, 133 degrees) of the table, recomputed from the definition."""
    from apps.match_scaled_views import count_right

    images, to_canvas = synthetic.similarity_texture_views(480, 640, DEGREES, SCALES, seed=7)
    views = (0, 4, 6)
    counted = {}
    for levels in (1, 8):
        k = {v: ko.describe(ko.Maps(images[v], levels, 20), 1000) for v in views}
        for v in views[1:]:
            partner, distance = gmo.match_pair(k[0].bits, k[0].valid, k[v].bits, k[v].valid)
            matches, _ = gmo.compact(partner, distance)
            right = count_right(matches, k[0].xy, k[0].level, SCALES[0], to_canvas[0], k[v].xy, k[v].level, SCALES[v], to_canvas[v])
            counted[levels, v] = (len(matches), right)
    for v in views[1:]:
        assert SCALES[v] / SCALES[0] >= 1.5
        (kept_1, right_1), (kept_8, right_8) = counted[1, v], counted[8, v]
        print(f"scale {SCALES[v]}, {DEGREES[v]} degrees: one level {kept_1} / {right_1}, eight levels {kept_8} / {right_8}")
        table_kept, table_right = TABLE[v][1]
        assert right_8 / kept_8 >= table_right / table_kept - 0.03
        assert right_1 <= right_8 / 4
        assert right_8 >= 20
