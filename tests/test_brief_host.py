"""Host tests of the oriented BRIEF descriptor: the committed pattern table, the NumPy definition (tests/brief_oracle.py),
its match rate under rotation next to NCC, argument checks and the C ABI.  No kernel is launched."""
import os
import re

import numpy as np
import pytest

import brief_oracle as bo
from structure_from_motion_amd import synthetic

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rotated_texture_pair(240, 320, angle, 300, SCENE_SEED): correct-match fraction of the oracle's descriptors, measured once on
# the committed scene generator and pattern table
SCENE_SEED = 7
MEASURED_BRIEF = {0: 0.993, 17: 0.950, 45: 0.917, 90: 0.993, 133: 0.937, 251: 0.933}


def test_pattern_file_matches_its_definition():
    offsets, boundaries = bo.pattern()
    assert offsets.shape == (30, 256, 4) and offsets.dtype == np.int8
    assert boundaries.shape == (30, 2) and boundaries.dtype == np.int64
    # |v| <= 13: a 5 x 5 box around a sample stays inside the 31 x 31 patch
    assert np.abs(offsets.astype(np.int64)).max() <= bo.PATCH_RADIUS - bo.BOX_HALF
    phi = (np.arange(30) + 0.5) * 2.0 * np.pi / 30
    expect = np.column_stack([np.round(2.0 ** 20 * np.cos(phi)), np.round(2.0 ** 20 * np.sin(phi))]).astype(np.int64)
    np.testing.assert_array_equal(boundaries, expect)
    np.testing.assert_array_equal(boundaries[15:], -boundaries[:15])
    # entry [b] is entry [0]'s (unrounded, norm <= 12) base points rotated by 2 pi b / 30: within rounding of rotating the
    # rounded entry [0], and never beyond the sample radius by more than the rounding
    base = offsets[0].astype(np.float64).reshape(-1, 2)
    for b in range(30):
        c, s = np.cos(2 * np.pi * b / 30), np.sin(2 * np.pi * b / 30)
        rotated = np.column_stack([base[:, 0] * c - base[:, 1] * s, base[:, 0] * s + base[:, 1] * c])
        got = offsets[b].astype(np.float64).reshape(-1, 2)
        assert np.abs(got - rotated).max() <= 0.5 + np.sqrt(0.5) + 1e-9
        assert np.hypot(got[:, 0], got[:, 1]).max() <= bo.SAMPLE_RADIUS + np.sqrt(0.5)
    # the product reads the same file
    from structure_from_motion_amd.feature_matching import brief

    assert os.path.samefile(brief.PATTERN_PATH, bo.PATTERN_PATH)
    got_offsets, got_boundaries = brief.load_pattern()
    np.testing.assert_array_equal(got_offsets, offsets)
    np.testing.assert_array_equal(got_boundaries, boundaries)


NORMALS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


@pytest.mark.parametrize("direction", range(8))
def test_half_plane_lands_in_expected_bin(direction):
    """A patch whose bright half faces `direction` * 45 degrees (x right, y down) has, by symmetry, its moment vector exactly
    along that direction.  Bin b is centred on 12 b degrees and starts at its lower boundary, so the expected bin is
    floor(45 direction / 12 + 1/2): 45 degrees is 3.75 bins in (bin 4), 90 degrees lies ON boundary 7 and belongs to bin 8."""
    nx, ny = NORMALS[direction]
    d = np.arange(64, dtype=np.int64) - 32
    dx, dy = np.meshgrid(d, d)
    image = np.where(dx * nx + dy * ny > 0, 200, 20).astype(np.uint8)
    m10, m01 = bo.moments(image, 32, 32)
    assert m10 * ny == m01 * nx and m10 * nx + m01 * ny > 0
    expect = int(np.floor(45.0 * direction / 12.0 + 0.5)) % 30
    assert bo.angle_bin(m10, m01) == expect
    bits, valid, bins = bo.describe(image, np.array([[32.0, 32.0]]))
    assert valid[0] and bins[0] == expect


def test_zero_moment_is_bin_zero_and_every_moment_has_one_bin():
    assert bo.angle_bin(0, 0) == 0
    flat = np.full((40, 40), 77, dtype=np.uint8)            # symmetric disc: m = 0
    assert bo.moments(flat, 20, 20) == (0, 0)
    bits, valid, bins = bo.describe(flat, np.array([[20.0, 20.0]]))
    assert valid[0] and bins[0] == 0 and not bits.any()    # equal box sums: no test is strictly smaller
    rng = np.random.default_rng(0)
    limit = 709 * 15 * 255                                   # the disc's pixel count times the largest |dx| I
    for m10, m01 in rng.integers(-limit, limit + 1, size=(10_000, 2)):
        bo.angle_bin(int(m10), int(m01))                     # asserts exactly one bin
    _, boundaries = bo.pattern()
    for b in range(30):                                      # a moment ON a boundary belongs to the bin that starts there
        assert bo.angle_bin(int(boundaries[b][0]), int(boundaries[b][1])) == (b + 1) % 30


def test_validity_and_centre_rounding():
    rng = np.random.default_rng(1)
    image = rng.integers(0, 256, (40, 50), dtype=np.uint8)
    H, W = image.shape
    feats = np.array([[14.49, 20], [14.5, 20], [W - 16 + 0.49, 20], [W - 16 + 0.5, 20], [20, 14.49], [20, 14.5],
                      [20, H - 16 + 0.49], [20, H - 16 + 0.5], [np.nan, 20], [20, np.inf], [20.5, 20.5], [21, 21]])
    bits, valid, bins = bo.describe(image, feats)
    assert valid.tolist() == [False, True, True, False, False, True, True, False, False, False, True, True]
    assert not bits[~valid].any() and not bins[~valid].any()
    np.testing.assert_array_equal(bits[10], bits[11])        # x + 0.5 exactly integral rounds up


@pytest.fixture(scope="module")
def scenes():
    return {angle: synthetic.rotated_texture_pair(240, 320, angle, 300, SCENE_SEED) for angle in MEASURED_BRIEF}


def test_rotated_texture_pair_contract(scenes):
    image_a, image_b, pairs = scenes[45]
    assert image_a.shape == image_b.shape == (240, 320) and image_a.dtype == image_b.dtype == np.uint8
    assert pairs.shape == (300, 4) and pairs.dtype == np.float64
    for x, y in ((pairs[:, 0], pairs[:, 1]), (pairs[:, 2], pairs[:, 3])):
        assert x.min() >= 20 and x.max() <= 319 - 20 and y.min() >= 20 and y.max() <= 239 - 20
    again = synthetic.rotated_texture_pair(240, 320, 45, 300, SCENE_SEED)
    assert all(np.array_equal(u, v) for u, v in zip(scenes[45], again))
    np.testing.assert_array_equal(scenes[0][0], image_a)     # the first image does not depend on the angle
    # no rotation, no noise: the second image IS the first
    a0, b0, p0 = synthetic.rotated_texture_pair(64, 80, 0, 5, 3, noise=0.0)
    np.testing.assert_array_equal(a0, b0)
    np.testing.assert_array_equal(p0[:, :2], p0[:, 2:])


@pytest.mark.parametrize("angle", sorted(MEASURED_BRIEF))
def test_oracle_match_rate_under_rotation(scenes, angle):
    image_a, image_b, pairs = scenes[angle]
    a, b = bo.describe(image_a, pairs[:, :2]), bo.describe(image_b, pairs[:, 2:])
    assert a[1].all() and b[1].all()
    rate = bo.correct_fraction(bo.hamming_scores(a[0], a[1], b[0], b[1]))
    print(f"angle {angle}: BRIEF correct-match fraction {rate:.4f}")
    assert rate >= MEASURED_BRIEF[angle] - 0.03
    assert rate >= 0.85
    if angle in (45, 90):
        ncc = bo.correct_fraction(bo.ncc_scores(image_a, image_b, pairs[:, :2], pairs[:, 2:], 9))
        print(f"angle {angle}: NCC window 9 correct-match fraction {ncc:.4f}")
        assert ncc <= 0.05


def test_argument_checks():
    from structure_from_motion_amd.feature_matching import brief

    image = np.zeros((40, 40), dtype=np.uint8)
    feats = np.array([[20.0, 20.0]])
    for bad in (image.astype(np.float64), image.astype(np.int16), image.astype(bool)):
        with pytest.raises(TypeError):
            brief.compute_brief(bad, feats)
    with pytest.raises(ValueError):
        brief.compute_brief(np.zeros((40, 40, 3), dtype=np.uint8), feats)
    for bad in (np.zeros((4, 3)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            brief.compute_brief(image, bad)
    with pytest.raises(TypeError):
        brief.BriefScore(image.astype(np.float32), image)
    # nothing to describe: no device is needed
    empty = brief.compute_brief(image, [])
    assert empty.bits.shape == (0, 32) and empty.valid.shape == (0,) and empty.angle_bin.shape == (0,)
    import lib.feature_matching.brief as drop_in

    assert drop_in.compute_brief is brief.compute_brief and drop_in.BriefScore is brief.BriefScore


def test_symbols_exported(native_lib):
    from structure_from_motion_amd import _native, build

    assert "sfm_brief.hip" in build.SOURCES
    assert "sfm_brief_describe" in _native.SIGNATURES and "sfm_hamming_summary" in _native.SIGNATURES
    assert "sfm_hamming_summary_workspace_bytes" in _native.OTHER_SYMBOLS
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    for name in ("sfm_brief_describe", "sfm_hamming_summary", "sfm_hamming_summary_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert getattr(native_lib, name) is not None
    assert native_lib.sfm_abi_version() == _native.ABI_VERSION == 15
    assert "#define SFM_ABI_VERSION 15" in header
    # 32 bytes per row and 512-column tile
    assert native_lib.sfm_hamming_summary_workspace_bytes(0, 10) == 0
    assert native_lib.sfm_hamming_summary_workspace_bytes(3, 512) == 3 * 32
    assert native_lib.sfm_hamming_summary_workspace_bytes(3, 513) == 2 * 3 * 32
    assert native_lib.sfm_hamming_summary_workspace_bytes(-1, 1) == -1
    # refusals that need no device: sizes and pointers are checked before any launch
    assert native_lib.sfm_brief_describe(None, 10, 10, None, 0, None, None, 30, None, None, None, None) == 0
    assert native_lib.sfm_brief_describe(None, 10, 10, None, 1, None, None, 30, None, None, None, None) != 0
    assert native_lib.sfm_brief_describe(None, 10, 10, None, 0, None, None, 65, None, None, None, None) != 0
    assert native_lib.sfm_hamming_summary(None, None, 0, None, None, 5, None, 0, None, None, None, None) == 0
    assert native_lib.sfm_hamming_summary(None, None, 2, None, None, 0, None, 0, None, None, None, None) != 0
