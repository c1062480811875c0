"""The logarithm of tests/rotation_averaging_oracle.py (operation by operation csrc/sfm_so3.h) against a definition it shares no
formula with: rotations built from an axis and an angle at 60 digits (tests/so3_log_cases.py), whose logarithm is angle * axis by
construction.  No GPU.

The bound is 1 000 x what rounding D to double alone costs: the largest change of a 60-digit logarithm when one entry of D moves
by half an ulp, measured below over the whole sweep (2 875 rotations: 115 axes x 25 angles from 0 to pi) as 1.9076e-16 rad and kept
as ``so3_log_cases.LOG_SENSITIVITY = 1.91e-16``, so the bound is 1.91e-13 rad, below the project's cap of 1e-8.  The logarithm's
largest error over the sweep is 9.9e-16 rad.  The formula before it (r = v theta / s down to s = 1e-10, then a column of
(D + I) / 2) missed the bound from pi - 1e-3 on: 1.9e-13 rad there, 1.8e-9 at pi - 1e-7, 1.4e-6 at pi - 1e-10.
"""
import numpy as np
import pytest

import rotation_averaging_oracle as ro
import so3_log_cases as sc


@pytest.fixture(scope="module")
def sweep():
    return sc.sweep()


def test_sweep_covers_every_branch(sweep):
    assert len(sweep) == 115 * 25
    columns, signs, below, above = set(), set(), 0, 0
    for _, D, r, _ in sweep:
        c = 0.5 * (D[0, 0] + D[1, 1] + D[2, 2] - 1.0)
        if c <= ro.HALF_TURN_COSINE:
            above += 1
            columns.add(int(np.argmax(np.diag(D))))
            signs.add(bool(r[int(np.argmax(np.abs(r)))] > 0))
        else:
            below += 1
    assert columns == {0, 1, 2} and signs == {True, False} and below and above


def test_half_ulp_sensitivity_is_what_the_bound_says(sweep):
    worst, where = 0.0, None
    for name, D, _, _ in sweep:
        s = sc.half_ulp_sensitivity(D)
        if s > worst:
            worst, where = s, name
    print(f"largest change of the 60-digit logarithm under half an ulp in one entry: {worst:.3g} rad ({where})")
    assert 0.99 * sc.LOG_SENSITIVITY <= worst <= sc.LOG_SENSITIVITY


def test_log_map_against_60_digits(sweep):
    worst = {}
    for name, D, r_true, sign_free in sweep:
        e = sc.error(ro.log_map(D), r_true, sign_free)
        angle = name.split(" at ")[1]
        if e > worst.get(angle, (-1.0, ""))[0]:
            worst[angle] = (e, name)
    for angle, (e, name) in worst.items():
        print(f"angle {angle:>10}: largest error {e:.3g} rad ({name})")
    bad = {a: v for a, v in worst.items() if not v[0] <= sc.BOUND}
    assert not bad, (sc.BOUND, bad)


def test_relative_error_at_small_angles(sweep):
    """Up to 2 rad the error is relative, however small the angle: two rounded entries of D per component of v, their
    difference and the product with theta / s, so at most 8 units of 2^-53 of the angle over the three components."""
    for name, D, r_true, _ in sweep:
        n = np.linalg.norm(r_true)
        if 0.0 < n <= 2.0:
            assert np.linalg.norm(ro.log_map(D) - r_true) <= 8 * 2.0 ** -53 * n, name


def test_exact_half_turns_and_first_of_equals():
    assert np.array_equal(ro.log_map(np.diag([1.0, -1.0, -1.0])), [np.pi, 0.0, 0.0])
    assert np.array_equal(ro.log_map(np.diag([-1.0, 1.0, -1.0])), [0.0, np.pi, 0.0])
    assert np.array_equal(ro.log_map(np.diag([-1.0, -1.0, 1.0])), [0.0, 0.0, np.pi])
    # a = (1, 1, 0) / sqrt(2): the diagonal entries 0 and 1 tie and column 0 is taken, so the first component is positive
    D = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    r = ro.log_map(D)
    assert r[0] > 0 and np.allclose(r, np.pi * np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), rtol=0, atol=1e-15)
    D = np.array([[-1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, -1.0, 0.0]])   # a = (0, 1, -1) / sqrt(2): column 1
    r = ro.log_map(D)
    assert r[1] > 0 and np.allclose(r, np.pi * np.array([0.0, 1.0, -1.0]) / np.sqrt(2.0), rtol=0, atol=1e-15)
