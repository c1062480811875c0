"""Generate structure_from_motion_amd/feature_matching/brief_pattern.json, the one table the oriented BRIEF descriptor
is defined by (the NumPy oracle, the host layer and the HIP kernel all read this file; nothing regenerates it at import).

  offsets     int8  [30, 256, 4]   (ax, ay, bx, by) of test t at angle bin b: 512 base points drawn from N(0, (31/5)^2)
                                   per axis (norms above 12 rejected), rotated by 2 pi b / 30 (x' = x c - y s,
                                   y' = x s + y c) and rounded with floor(v + 0.5)
  boundaries  int64 [30, 2]        B[b] = (round(2^20 cos phi_b), round(2^20 sin phi_b)), phi_b = (b + 1/2) 2 pi / 30

The file is JSON: nested lists of integers under those two names (the dtypes are the reader's).  Run once; the result
is committed.  `--check` compares a fresh table with the committed file instead of writing it.
"""
import json
import os
import sys

import numpy as np

BINS, TESTS, SAMPLE_RADIUS, SIGMA, SEED = 30, 256, 12.0, 31.0 / 5.0, 20260
PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "structure_from_motion_amd",
                    "feature_matching", "brief_pattern.json")


def make():
    rng = np.random.default_rng(SEED)
    points = np.empty((0, 2))
    while len(points) < 2 * TESTS:
        draw = rng.normal(0.0, SIGMA, size=(2 * TESTS, 2))
        points = np.concatenate([points, draw[np.hypot(draw[:, 0], draw[:, 1]) <= SAMPLE_RADIUS]])
    points = points[:2 * TESTS]
    offsets = np.empty((BINS, TESTS, 4), dtype=np.int8)
    for b in range(BINS):
        c, s = np.cos(2.0 * np.pi * b / BINS), np.sin(2.0 * np.pi * b / BINS)
        x = points[:, 0] * c - points[:, 1] * s
        y = points[:, 0] * s + points[:, 1] * c
        rounded = np.floor(np.column_stack([x, y]) + 0.5).astype(np.int64)
        assert np.abs(rounded).max() <= 13
        offsets[b] = rounded.reshape(TESTS, 4)       # test t compares points 2t (a) and 2t + 1 (b)
    phi = (np.arange(BINS) + 0.5) * 2.0 * np.pi / BINS
    boundaries = np.column_stack([np.round(2.0 ** 20 * np.cos(phi)), np.round(2.0 ** 20 * np.sin(phi))]).astype(np.int64)
    return offsets, boundaries


if __name__ == "__main__":
    offsets, boundaries = make()
    if "--check" in sys.argv:
        with open(PATH) as f:
            table = json.load(f)
        same = np.array_equal(table["offsets"], offsets) and np.array_equal(table["boundaries"], boundaries)
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    # plain text (a binary table would not diff): one line per angle bin
    rows = ",\n".join("  " + json.dumps(o.tolist(), separators=(",", ":")) for o in offsets)
    with open(PATH, "w") as f:
        f.write('{"boundaries": %s,\n "offsets": [\n%s\n ]}\n' % (json.dumps(boundaries.tolist()), rows))
    print(PATH, offsets.shape, boundaries.shape)
