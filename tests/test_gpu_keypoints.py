"""GPU tests of the multi-scale keypoint detector (csrc/sfm_keypoints.hip): keypoints, descriptors, pyramid planes and both
score maps byte for byte against the NumPy definition (tests/keypoint_oracle.py) on one collection of images whose sizes cross
every boundary of the definition and of the kernels' 64 x 16 tiles, against ``compute_brief``, call against call, collection
against single images, through the capacity re-call and through the app."""
import functools

import numpy as np
import pytest

import graph_matching_oracle as gmo
import keypoint_oracle as ko

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native_lib):
    from structure_from_motion_amd import device

    device.require_gpu()


from structure_from_motion_amd import synthetic  # noqa: E402
from structure_from_motion_amd.feature_matching import keypoints as kp  # noqa: E402
from structure_from_motion_amd.feature_matching.brief import compute_brief  # noqa: E402

# (height, width, content).  30 x 200: no testable pixel; 31 x 31: one; 59 x 61: level 1 would be 47 wide and does not exist;
# 60 x 60: level 1 exists and is the smallest there is; heights 15 / 16 / 17 and 47 / 48 / 49 and widths 63 / 64 / 65 and
# 127 / 128 / 129: one below, at and one above the extents of one, two and three tiles of 64 x 16 pixels
COLLECTION = (
    (30, 200, "noise"), (31, 31, "noise"), (48, 48, "noise"), (59, 61, "texture"), (60, 60, "noise"), (97, 131, "tiled"),
    (129, 64, "texture"), (200, 263, "texture"), (15, 63, "noise"), (16, 64, "noise"), (17, 65, "tiled"), (47, 63, "tiled"),
    (48, 64, "noise"), (49, 65, "texture"), (63, 127, "noise"), (64, 128, "constant"), (65, 129, "tiled"), (100, 110, "constant"),
)
THRESHOLDS, LEVELS, MAX_LEVELS = (1, 20, 254), (1, 3, 8), 8
NUM_FEATURES = (1, 7, 200, 100000)                  # the last: more than there are survivors in any image
SETTINGS = [(t, l, n) for t in THRESHOLDS for l in LEVELS for n in NUM_FEATURES]


def _image(height, width, content, seed):
    rng = np.random.default_rng(seed)
    if content == "texture":
        return synthetic.similarity_texture_views(height, width, [10.0 * seed], [1.0], seed)[0][0]
    if content == "constant":
        return np.full((height, width), 137, dtype=np.uint8)
    if content == "tiled":                           # one 8 x 8 tile repeated: scores tie massively
        tile = rng.integers(0, 256, (8, 8), dtype=np.uint8)
        return np.ascontiguousarray(np.tile(tile, (height // 8 + 1, width // 8 + 1))[:height, :width])
    noise = rng.integers(0, 256, (height, width), dtype=np.uint8)   # corners everywhere
    noise[rng.random((height, width)) < 0.2] = 255                   # ... and saturated pixels
    noise[rng.random((height, width)) < 0.1] = 0
    if height >= 48 and width >= 48:                 # a corner that passes threshold 254: a 0 inside a ring of 255 ...
        y, x = height // 2, width // 2
        noise[y - 3:y + 4, x - 3:x + 4] = 255
        noise[y, x] = 0
    if height >= 60 and width >= 60:                 # ... and a 255 inside a ring of 0
        noise[15:22, 15:22] = 0
        noise[18, 18] = 255
    return noise


@functools.lru_cache(maxsize=None)
def images():
    out = [_image(h, w, content, seed) for seed, (h, w, content) in enumerate(COLLECTION)]
    for image in out:
        image.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def maps(threshold):
    """The oracle's planes, score maps and survivors of every image at eight levels: computed once per threshold, shared by
    every test, never changed (fewer levels read a prefix of them)."""
    return tuple(ko.Maps(image, MAX_LEVELS, threshold) for image in images())


_memo = [dict() for _ in COLLECTION]                # descriptors per (level, x, y) of an image's planes: no setting changes them


def expected(threshold, levels, num_features, only=None):
    return [ko.describe(m, num_features, _memo[i], levels) for i, m in enumerate(maps(threshold)) if only is None or i == only]


def assert_equal_keypoints(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.xy.dtype == np.float64 and g.level.dtype == np.uint8 and g.score.dtype == np.int32
        assert g.descriptors.bits.dtype == np.uint8 and g.descriptors.valid.dtype == np.bool_
        assert g.xy.shape == (len(w.xy), 2), i
        assert g.xy.tobytes() == w.xy.tobytes(), i
        assert np.array_equal(g.level, w.level) and np.array_equal(g.score, w.score), i
        assert np.array_equal(g.descriptors.bits, w.bits), i
        assert np.array_equal(g.descriptors.valid, w.valid) and np.all(g.descriptors.valid), i
        assert np.array_equal(g.descriptors.angle_bin, w.angle_bin), i


def assert_equal_maps(run, threshold):
    """The pyramid planes and both score maps the C call left on the device."""
    pool = run.pool.cpu().numpy()
    score = run.score.cpu().numpy().view(np.uint16)
    kept = run.kept.cpu().numpy().view(np.uint16)
    want = maps(threshold)
    for image, level, h, w, at, _ in run.plan.rows:
        m = want[image]
        assert m.planes[level].shape == (h, w)
        assert np.array_equal(pool[at:at + h * w].reshape(h, w), m.planes[level]), (image, level)
        assert np.array_equal(score[at:at + h * w].reshape(h, w), m.scores[level]), (image, level)
        assert np.array_equal(kept[at:at + h * w].reshape(h, w), m.kept[level]), (image, level)


def test_the_collection_covers_the_cases():
    shapes = [ko.level_shapes(h, w, MAX_LEVELS) for h, w, _ in COLLECTION]
    assert len(shapes[0]) == 1 and len(shapes[3]) == 1 and shapes[4] == [(60, 60), (48, 48)]
    assert max(len(s) for s in shapes) == 7          # 200 x 263 stops at 51 x 68
    m = maps(20)
    assert not m[0].scores[0].any() and np.count_nonzero(m[1].scores[0]) <= 1
    assert not m[15].scores[0].any() and not m[17].scores[0].any()          # constant: no corner anywhere
    ties = m[5].survivors[0][2]
    assert len(ties) > 3 * len(np.unique(ties))      # the tiled image: every score many times
    assert all(len(m[7].survivors[l][0]) > 0 for l in range(7))
    assert max(sum(len(s[0]) for s in x.survivors) for x in maps(1)) < NUM_FEATURES[-1]
    assert [int(s) for x in maps(254) for s in x.survivors[0][2]] == [16] * 6   # only the planted corners pass 254


@pytest.mark.parametrize("threshold,levels,num_features", SETTINGS)
def test_equals_the_definition(threshold, levels, num_features):
    got, run = kp._detect(list(images()), num_features, levels, threshold)
    assert_equal_keypoints(got, expected(threshold, levels, num_features))
    assert_equal_maps(run, threshold)
    public = kp.detect_and_describe(list(images()), num_features=num_features, levels=levels, threshold=threshold)
    assert_equal_keypoints(public, expected(threshold, levels, num_features))


def test_each_descriptor_is_compute_briefs_on_the_oracle_plane():
    got = kp.detect_and_describe(list(images()), num_features=200, levels=8, threshold=20)
    want = expected(20, 8, 200)
    described = 0
    for i, (g, w) in enumerate(zip(got, want)):
        for level in np.unique(w.level):
            rows = np.nonzero(w.level == level)[0]
            d = compute_brief(np.array(maps(20)[i].planes[level]), w.level_xy[rows].astype(np.float64))
            assert np.array_equal(g.descriptors.bits[rows], d.bits) and np.all(d.valid)
            assert np.array_equal(g.descriptors.angle_bin[rows], d.angle_bin)
            described += len(rows)
    assert described > 500


def test_two_calls_give_the_same_bytes():
    a = kp.detect_and_describe(list(images()), num_features=200, levels=8, threshold=1)
    b = kp.detect_and_describe(list(images()), num_features=200, levels=8, threshold=1)
    for x, y in zip(a, b):
        assert x.xy.tobytes() == y.xy.tobytes() and x.level.tobytes() == y.level.tobytes()
        assert x.score.tobytes() == y.score.tobytes() and x.descriptors.bits.tobytes() == y.descriptors.bits.tobytes()
        assert x.descriptors.angle_bin.tobytes() == y.descriptors.angle_bin.tobytes()


def test_the_collection_equals_the_single_images():
    together = kp.detect_and_describe(list(images()), num_features=7, levels=3, threshold=20)
    for i, image in enumerate(images()):
        alone = kp.detect_and_describe([image], num_features=7, levels=3, threshold=20)
        assert_equal_keypoints(alone, expected(20, 3, 7, only=i))
        assert alone[0].xy.tobytes() == together[i].xy.tobytes()
        assert np.array_equal(alone[0].descriptors.bits, together[i].descriptors.bits)


@pytest.mark.parametrize("num_features", (7, 100000))
def test_a_capacity_below_the_candidates_gives_the_same_result(num_features):
    want = expected(1, 8, num_features)
    got, run = kp._detect(list(images()), num_features, 8, 1, capacity=5)
    assert run.calls == 2 and run.found > 5 and run.capacity == run.found
    assert_equal_keypoints(got, want)
    free, free_run = kp._detect(list(images()), num_features, 8, 1)
    assert free_run.found == run.found               # the cutoffs do not depend on the capacity
    assert_equal_keypoints(free, want)


def test_the_app_counts_what_the_definition_counts():
    from apps import match_scaled_views as app

    degrees, scales = (0.0, 30.0), (1.0, 1.5)
    views, to_canvas = synthetic.similarity_texture_views(120, 160, degrees, scales, 5)
    record = app.run(degrees, scales, 120, 160, features=150, threshold=20, seed=5, images=views, to_canvas=to_canvas)
    assert [r["levels"] for r in record["runs"]] == [1, 8]
    for r in record["runs"]:
        k = [ko.describe(ko.Maps(v, r["levels"], 20), 150) for v in views]
        partner, distance = gmo.match_pair(k[0].bits, k[0].valid, k[1].bits, k[1].valid)
        matches, _ = gmo.compact(partner, distance)
        right = app.count_right(matches, k[0].xy, k[0].level, scales[0], to_canvas[0], k[1].xy, k[1].level, scales[1],
                                to_canvas[1])
        assert r["keypoints"] == [len(x.xy) for x in k]
        assert [(p["images"], p["kept"], p["right"]) for p in r["pairs"]] == [([0, 1], len(matches), right)]
