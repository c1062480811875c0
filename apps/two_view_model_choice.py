"""Which model explains an image pair — an essential matrix or a homography — on synthetic pairs
(``lib.epipolar.homography.select_two_view_model``): every relative motion of tests/motion_cases.py on a scene
with depth, two rotations without translation (``pan10``, ``gen12``) and the bench motion in front of a plane
(``plane_bench``).  One JSON line per pair: the inlier counts of the two RANSAC passes, their ratio and the kind chosen.

    python apps/two_view_model_choice.py [--n 300] [--iterations 200] [--threshold 2e-5]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))   # the motions and scenes the tests use

import numpy as np  # noqa: E402

import motion_cases  # noqa: E402
from geometry_cases import rotation  # noqa: E402
from lib.common.feature import Feature  # noqa: E402
from lib.epipolar.homography import select_two_view_model  # noqa: E402
from lib.feature_matching.matching import Match  # noqa: E402
from structure_from_motion_amd import synthetic  # noqa: E402

# name -> (R, t, planar): the pairs without a usable baseline or without depth
EXTRA = {
    "pan10": (rotation(motion_cases.Y_AXIS, 10.0), np.zeros(3), False),
    "gen12": (rotation(motion_cases.GENERAL_AXIS, 12.0), np.zeros(3), False),
    "plane_bench": (*motion_cases.MOTIONS["bench"], True),
}


def pair_scene(R, t, planar, n, seed, noise_px, outlier_fraction, K=synthetic.BENCH_K):
    """Pixels (n, 2) of points in x, y in [-1, 1] and z in [4, 6] — or on the plane z = 5 + 0.2 x - 0.1 y — in [I | 0] and
    [R | t], with Gaussian noise and a fraction of the second view replaced by uniform pixels."""
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(4.0, 6.0, n)
    X = np.column_stack([x, y, 5.0 + 0.2 * x - 0.1 * y if planar else z])

    def project(Xc):
        uvw = Xc @ K.T
        return uvw[:, :2] / uvw[:, 2:3] + rng.normal(0.0, 1.0, (n, 2)) * noise_px

    pa, pb = project(X), project(X @ R.T + t)
    out = rng.random(n) < outlier_fraction
    rand_px = np.column_stack([rng.uniform(0, 2.0 * K[0, 2], n), rng.uniform(0, 2.0 * K[1, 2], n)])
    return pa, np.where(out[:, None], rand_px, pb)


def run(n=300, iterations=200, threshold=2e-5, min_extra=20, noise_px=0.5, outlier_fraction=0.3, scene_seed=7, shuffle_seed=5,
        essential_solver="five_point"):
    """-> list of dict(motion, homography_count, essential_count, ratio, kind), the motions of motion_cases first."""
    pairs = {name: (R, t, False) for name, (R, t) in motion_cases.MOTIONS.items()}
    pairs.update(EXTRA)
    rows = []
    for name, (R, t, planar) in pairs.items():
        pa, pb = pair_scene(R, t, planar, n, scene_seed, noise_px, outlier_fraction)
        fa = [Feature(float(p[0]), float(p[1])) for p in pa]
        fb = [Feature(float(p[0]), float(p[1])) for p in pb]
        random.seed(shuffle_seed)
        m = select_two_view_model(synthetic.BENCH_K, fa, fb, [Match(a_index=i, b_index=i) for i in range(n)], threshold, min_extra,
                                  iterations, essential_solver)
        rows.append(dict(motion=name, homography_count=m.homography_count, essential_count=m.essential_count,
                         ratio=None if m.essential_count == 0 else round(m.ratio, 4), kind=m.kind))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--threshold", type=float, default=2e-5)
    ap.add_argument("--min-extra", type=int, default=20)
    ap.add_argument("--essential-solver", default="five_point", choices=["five_point", "eight_point"])
    args = ap.parse_args()
    for row in run(args.n, args.iterations, args.threshold, args.min_extra, essential_solver=args.essential_solver):
        print(json.dumps(row))
