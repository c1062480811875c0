"""The sweep of rotations on which the logarithm of tests/rotation_averaging_oracle.py and csrc/sfm_so3.h is measured against a
definition of its own (tests/test_so3_log_host.py on the CPU, test_logarithm_on_a_star of tests/test_gpu_averaging_edges.py on
the device): D = cos(t) I + sin(t) [a]x + (1 - cos(t)) a a^T built with mpmath at 60 digits from a unit axis a and an angle t and
rounded once to double; its logarithm is t a by construction, with no formula shared with the code under test.

``mp_log`` is a 60-digit logarithm of a matrix near a rotation, used only to measure what half an ulp in one entry of D is
worth: the angle from atan2(|v|, c); the axis from v = vee(D - D^T) / 2 below 120 degrees and from the symmetric part
(D + D^T) / 2 = c I + (1 - c) a a^T above, signed by v (either definition alone is ill conditioned at one end).
"""
from __future__ import annotations

import mpmath
import numpy as np

DIGITS = 60
GAPS = (0.1, 1e-3, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 3e-10, 1.5e-10, 1e-10, 5e-11, 1e-11, 1e-13, 0.0)   # angle = pi - gap
ANGLES = (0.0, 1e-15, 1e-12, 5e-11, 1e-10, 2e-10, 1e-8, 1e-6, 1e-3, 1.0, 2.0)
SIGN_FREE_GAP = 1e-9   # below this gap r and -r both count: both are logarithms at pi, and v's sign fades into its rounding

# The largest change of the 60-digit logarithm when one entry of D moves by half an ulp, over the sweep (measured on the CPU by
# tests/test_so3_log_host.py as 1.9076e-16, which asserts that it is this value to 1 %): what rounding D to double alone costs.
LOG_SENSITIVITY = 1.91e-16
BOUND = min(1000 * LOG_SENSITIVITY, 1e-8)   # radians


def axes():
    """(name, axis): +-e0, +-e1, +-e2 (every column choice, both signs), axes whose two or three largest components are equal
    (the first-of-equals rule), and 100 seeded random ones."""
    out = []
    for k in range(3):
        for sign in (1.0, -1.0):
            a = np.zeros(3)
            a[k] = sign
            out.append((f"{'+' if sign > 0 else '-'}e{k}", a))
    for name, a in (("e0+e1", (1, 1, 0)), ("e0+e2", (1, 0, 1)), ("e1+e2", (0, 1, 1)), ("e0-e1", (1, -1, 0)), ("-e1-e2", (0, -1, -1)),
                    ("e0+e1+e2", (1, 1, 1)), ("-e0+e1-e2", (-1, 1, -1)), ("2e0+2e1+e2", (2, 2, 1)), ("e0+2e1+2e2", (1, 2, 2))):
        out.append((name, np.array(a, dtype=np.float64)))
    rng = np.random.default_rng(2024)
    for i in range(100):
        out.append((f"random {i}", rng.normal(size=3)))
    return out


def angles():
    """(name, angle as an mpf at 60 digits)."""
    with mpmath.workdps(DIGITS):
        return [(f"{t:g}", mpmath.mpf(t)) for t in ANGLES] + [(f"pi-{g:g}", mpmath.pi - mpmath.mpf(g)) for g in GAPS]


def rotation(axis, angle):
    """(D [3,3] rounded once to double, r = angle * axis / |axis| rounded to double) from 60-digit arithmetic."""
    with mpmath.workdps(DIGITS):
        a = [mpmath.mpf(float(x)) for x in axis]
        n = mpmath.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        a = [x / n for x in a]
        co, si = mpmath.cos(angle), mpmath.sin(angle)
        K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
        D = [[(co if i == j else 0) + si * K[i][j] + (1 - co) * a[i] * a[j] for j in range(3)] for i in range(3)]
        return np.array([[float(x) for x in row] for row in D]), np.array([float(angle * x) for x in a])


def sweep():
    """Every (name, D, r, sign_free) of the sweep, in a fixed order."""
    out = []
    for aname, axis in axes():
        for tname, t in angles():
            D, r = rotation(axis, t)
            out.append((f"{aname} at {tname}", D, r, tname.startswith("pi-") and float(tname[3:]) < SIGN_FREE_GAP))
    return out


def mp_log(D):
    """The logarithm of a matrix of mpf near a rotation, as a list of three mpf (at the caller's precision)."""
    v = [(D[2][1] - D[1][2]) / 2, (D[0][2] - D[2][0]) / 2, (D[1][0] - D[0][1]) / 2]
    s = mpmath.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = (D[0][0] + D[1][1] + D[2][2] - 1) / 2
    theta = mpmath.atan2(s, c)
    if c > -0.5:
        return [x * (theta / s) for x in v] if s > 0 else v
    S = [[(D[i][j] + D[j][i]) / 2 - (c if i == j else 0) for j in range(3)] for i in range(3)]
    k = max(range(3), key=lambda m: S[m][m])
    col = [S[m][k] for m in range(3)]
    n = mpmath.sqrt(col[0] * col[0] + col[1] * col[1] + col[2] * col[2])
    g = -1 if col[0] * v[0] + col[1] * v[1] + col[2] * v[2] < 0 else 1
    return [g * theta * x / n for x in col]


def error(r, r_true, sign_free):
    e = float(np.linalg.norm(r - r_true))
    return min(e, float(np.linalg.norm(r + r_true))) if sign_free else e


def half_ulp_sensitivity(D):
    """The largest |mp_log(D + half an ulp in one entry) - mp_log(D)| over the nine entries, in radians."""
    with mpmath.workdps(DIGITS):
        M = [[mpmath.mpf(float(D[i, j])) for j in range(3)] for i in range(3)]
        r0 = mp_log(M)
        worst = mpmath.mpf(0)
        for i in range(3):
            for j in range(3):
                P = [row[:] for row in M]
                P[i][j] = P[i][j] + mpmath.mpf(float(np.spacing(abs(D[i, j])))) / 2
                r = mp_log(P)
                for sign in (1, -1):   # at the half turn the perturbed matrix may land on the other logarithm
                    d = mpmath.sqrt(sum((r[m] - sign * r0[m]) ** 2 for m in range(3)))
                    if sign == 1:
                        best = d
                    elif float(D[0, 0] + D[1, 1] + D[2, 2]) < -0.9:
                        best = min(best, d)
                worst = max(worst, best)
        return float(worst)
