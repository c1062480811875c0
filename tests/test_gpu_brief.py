"""GPU tests of the oriented BRIEF descriptor and its Hamming matcher (csrc/sfm_brief.hip): bit-exact against the NumPy
definition (tests/brief_oracle.py) and against the reference-shaped heapq route of match_brute_force."""
import numpy as np
import pytest

import brief_oracle as bo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native_lib):
    from structure_from_motion_amd import device

    device.require_gpu()


from lib.common.feature import Feature  # noqa: E402
from lib.feature_matching import brief, matching  # noqa: E402
from structure_from_motion_amd import synthetic  # noqa: E402
from structure_from_motion_amd.feature_matching import _device_match  # noqa: E402
from structure_from_motion_amd.feature_matching import matching as matching_impl  # noqa: E402

SCENE_SEED = 7


def texture(height, width, seed):
    """Smooth random uint8 texture (neighbouring box sums differ, few ties)."""
    return synthetic.rotated_texture_pair(max(height, 48), max(width, 48), 0, 1, seed)[0][:height, :width].copy()


def edge_features(height, width, n, seed):
    """n features on a height x width image: first every combination of centre pixels in {14, 15, W-16, W-15} x
    {14, 15, H-16, H-15} (valid only at 15 and size - 16), non-finite coordinates, x + 0.5 exactly integral (rounds up, and across
    the validity edge), duplicates — then random positions over and beyond the image."""
    rng = np.random.default_rng(seed)
    xs, ys = [14, 15, width - 16, width - 15], [14, 15, height - 16, height - 15]
    special = [(float(x), float(y)) for x in xs for y in ys]
    special += [(np.nan, 30.0), (30.0, np.nan), (np.inf, 30.0), (30.0, -np.inf), (1e300, 30.0),
                (20.5, 30.5), (21.0, 31.0), (14.5, 30.0), (width - 16 + 0.5, 30.0), (30.0, 14.5), (30.0, height - 16 + 0.5),
                (30.25, 20.75), (30.25, 20.75), (30.0, 21.0), (-3.0, 20.0), (20.0, -0.5), (15.4999, 15.4999)]
    rand = np.column_stack([rng.uniform(-4, width + 4, n), rng.uniform(-4, height + 4, n)])
    rand[::3] = np.floor(rand[::3])
    return np.concatenate([np.array(special, dtype=np.float64), rand])[:n]


def assert_descriptors_equal(got, image, feats):
    bits, valid, bins = bo.describe(image, feats)
    assert got.bits.dtype == np.uint8 and got.valid.dtype == bool and got.angle_bin.dtype == np.uint8
    assert got.bits.shape == (len(feats), 32)
    np.testing.assert_array_equal(got.valid, valid)
    np.testing.assert_array_equal(got.angle_bin, bins)
    np.testing.assert_array_equal(got.bits, bits)
    return valid


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_compute_brief_bit_exact_small_image(n):
    image = texture(64, 80, 11)
    feats = edge_features(64, 80, n, n)
    valid = assert_descriptors_equal(brief.compute_brief(image, feats), image, feats)
    if n >= 63:
        assert valid.any() and not valid.all()
    # the Feature-list form of the same features
    got = brief.compute_brief(image, [Feature(x=float(x), y=float(y)) for x, y in feats])
    assert_descriptors_equal(got, image, feats)


def test_compute_brief_bit_exact_300_features():
    image_a, image_b, pairs = synthetic.rotated_texture_pair(240, 320, 45, 300, SCENE_SEED)
    for image, feats in ((image_a, pairs[:, :2]), (image_b, pairs[:, 2:])):
        got = brief.compute_brief(image, feats)
        assert assert_descriptors_equal(got, image, feats).all()
        assert len(np.unique(got.angle_bin)) > 20          # the scene exercises the angle bins


def test_compute_brief_flat_and_extreme_images():
    """m = 0 (bin 0, all box sums equal) and the largest moments and box sums a uint8 image can give."""
    feats = np.array([[20.0, 20.0], [24.0, 22.0]])
    flat = np.full((48, 48), 255, dtype=np.uint8)
    assert_descriptors_equal(brief.compute_brief(flat, feats), flat, feats)
    step = np.zeros((48, 48), dtype=np.uint8)
    step[:, 21:] = 255
    assert_descriptors_equal(brief.compute_brief(step, feats), step, feats)
    assert_descriptors_equal(brief.compute_brief(np.ascontiguousarray(step.T), feats), np.ascontiguousarray(step.T), feats)


def random_descriptors(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":        # three distinct descriptors: almost every comparison in the heap is a tie
        pool = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        pool[1] = pool[0]
        pool[1, 0] ^= 1       # distance 1 from pool[0]
        bits = pool[rng.integers(0, 3, n)]
    else:
        bits = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if kind == "invalid":
        valid = rng.random(n) >= 0.2
    else:
        valid = np.ones(n, dtype=bool)
    return bits, valid


def host_summary(bits_a, valid_a, bits_b, valid_b):
    """matching._host_rows — the reference's heapq loop — over a Python popcount closure."""
    ints_a = [int.from_bytes(b.tobytes(), "little") if ok else None for b, ok in zip(bits_a, valid_a)]
    ints_b = [int.from_bytes(b.tobytes(), "little") if ok else None for b, ok in zip(bits_b, valid_b)]

    def score(a, b):
        return float("inf") if a is None or b is None else float(bin(a ^ b).count("1"))

    best, arg, second, _ = matching_impl._host_rows(ints_a, ints_b, score)
    return np.array(best, dtype=np.float64), np.array(arg, dtype=np.int64), np.array(second, dtype=np.float64)


# the last three: more than one 512-column tile, a one-column last tile, more than one 256-row block
SIZES = [(1, 1), (1, 2), (3, 3), (127, 129), (128, 128), (129, 127), (130, 700), (5, 1), (3, 1025), (2, 513), (257, 40)]


@pytest.mark.parametrize("kind", ["random", "ties", "invalid", "all_b_invalid"])
@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_hamming_summary_equals_heapq(n_a, n_b, kind):
    bits_a, valid_a = random_descriptors(n_a, kind, 1000 + n_a)
    bits_b, valid_b = random_descriptors(n_b, kind, 2000 + n_b)
    if kind == "all_b_invalid":
        valid_b[:] = False
    best, arg, second = _device_match.hamming_summary(bits_a, valid_a, bits_b, valid_b)
    best_o, arg_o, second_o = host_summary(bits_a, valid_a, bits_b, valid_b)
    np.testing.assert_array_equal(best, best_o)              # assert_array_equal: NaN equals NaN
    np.testing.assert_array_equal(arg, arg_o)
    np.testing.assert_array_equal(second, second_o)
    if n_b == 1:
        assert np.isnan(second).all()
    if kind == "all_b_invalid":
        assert np.isinf(best).all() and not arg.any()
    # and the oracle's matrix agrees on the first minimum
    scores = bo.hamming_scores(bits_a, valid_a, bits_b, valid_b)
    np.testing.assert_array_equal(arg, np.argmin(scores, axis=1))
    np.testing.assert_array_equal(best, scores.min(axis=1))


def test_hamming_summary_no_rows():
    bits_b, valid_b = random_descriptors(4, "random", 0)
    best, arg, second = _device_match.hamming_summary(np.zeros((0, 32), np.uint8), np.zeros(0, bool), bits_b, valid_b)
    assert best.shape == arg.shape == second.shape == (0,)


class Unrecognised:
    """The same distances behind a callable match_brute_force does not know: the generic heapq route."""

    def __init__(self, score):
        self.score = score

    def __call__(self, a, b):
        return self.score(a, b)


@pytest.fixture(scope="module")
def pair45():
    image_a, image_b, pairs = synthetic.rotated_texture_pair(240, 320, 45, 300, SCENE_SEED)
    order = np.random.default_rng(5).permutation(len(pairs))     # the true partner of a[i] is b[where[i]], not b[i]
    where = np.argsort(order)
    fa = [Feature(x=float(x), y=float(y)) for x, y in pairs[:, :2]]
    fb = [Feature(x=float(x), y=float(y)) for x, y in pairs[order, 2:]]
    return image_a, image_b, pairs, order, where, fa, fb


STRATEGIES = {
    "none": None,
    "ratio": matching.ValidationStrategy.RATIO_TEST,
    "cross": {matching.ValidationStrategy.CROSSCHECK},
    "both": {matching.ValidationStrategy.RATIO_TEST, matching.ValidationStrategy.CROSSCHECK},
}


@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_match_brute_force_with_brief_score(pair45, strategy):
    image_a, image_b, pairs, order, where, fa, fb = pair45
    score = brief.BriefScore(image_a, image_b)
    kwargs = dict(validation_strategies=STRATEGIES[strategy], ratio_test_threshold=0.8)
    got = matching.match_brute_force(fa, fb, score, **kwargs)
    expect = matching.match_brute_force(fa, fb, Unrecognised(brief.BriefScore(image_a, image_b)), **kwargs)
    assert got == expect and len(got) > 100
    assert all(isinstance(m.match_score, float) and isinstance(m.b_index, int) for m in got)
    if strategy == "none":
        # the best matches are as often right as the oracle's
        a, b = bo.describe(image_a, pairs[:, :2]), bo.describe(image_b, pairs[order, 2:])
        rate_oracle = bo.correct_fraction(bo.hamming_scores(a[0], a[1], b[0], b[1]), where)
        assert len(got) == len(fa)
        rate = float(np.mean([m.b_index == where[m.a_index] for m in got]))
        assert rate == rate_oracle and rate >= 0.85


def test_brief_score_call_and_empty_lists(pair45):
    image_a, image_b, pairs, order, where, fa, fb = pair45
    score = brief.BriefScore(image_a, image_b)
    a, b = bo.describe(image_a, pairs[:3, :2]), bo.describe(image_b, pairs[order[:3], 2:])
    expect = bo.hamming_scores(a[0], a[1], b[0], b[1])
    for i in range(3):
        for j in range(3):
            value = score(fa[i], fb[j])
            assert type(value) is float and value == expect[i, j]
    assert score(Feature(x=3.0, y=50.0), fb[0]) == float("inf")            # patch leaves the image
    assert score(fa[0], Feature(x=float("nan"), y=50.0)) == float("inf")
    assert matching.match_brute_force([], fb, score) == []
    assert matching.match_brute_force(fa, [], score, validation_strategies=matching.ValidationStrategy.RATIO_TEST) == []
    with pytest.raises(IndexError):
        matching.match_brute_force(fa, [], score)


def test_repeatable():
    image = texture(64, 80, 11)
    feats = edge_features(64, 80, 130, 130)
    first, again = brief.compute_brief(image, feats), brief.compute_brief(image, feats)
    for u, v in zip(first, again):
        assert u.tobytes() == v.tobytes()
    bits_a, valid_a = random_descriptors(130, "ties", 1)
    bits_b, valid_b = random_descriptors(700, "ties", 2)
    one = _device_match.hamming_summary(bits_a, valid_a, bits_b, valid_b)
    two = _device_match.hamming_summary(bits_a, valid_a, bits_b, valid_b)
    for u, v in zip(one, two):
        assert u.tobytes() == v.tobytes()
