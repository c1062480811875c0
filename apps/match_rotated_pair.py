"""Match a textured image against rotated copies of itself with the two front ends of ``match_brute_force``: NCC over
axis-aligned 9 x 9 windows (``ImagePairScore``) and the Hamming distance of oriented BRIEF descriptors (``BriefScore``).

The scene is ``synthetic.rotated_texture_pair``: a band-limited random texture, its copy rotated about the image centre with
bilinear sampling and 1 % noise, and ground-truth feature pairs (the second list is shuffled, so an index says nothing).
For every angle the fraction of features whose best match — no validation strategy — is the true partner is printed, as
JSON.  Both matchers run on the GPU.

    python apps/match_rotated_pair.py --angles 0 17 45 90
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lib.common.feature import Feature
from lib.feature_matching.brief import BriefScore
from lib.feature_matching.matching import ImagePairScore, match_brute_force
from lib.feature_matching.ncc import calculate_ncc
from structure_from_motion_amd import synthetic


def correct_fraction(matches, where) -> float:
    return float(np.mean([m.b_index == where[m.a_index] for m in matches])) if matches else 0.0


def run(angles=(0.0, 17.0, 45.0, 90.0), height: int = 240, width: int = 320, features: int = 300, seed: int = 7,
        noise: float = 0.01, window: int = 9):
    out = dict(height=height, width=width, features=features, seed=seed, noise=noise, ncc_window=window, angles=[])
    for angle in angles:
        image_a, image_b, pairs = synthetic.rotated_texture_pair(height, width, angle, features, seed, noise)
        order = np.random.default_rng(seed).permutation(features)
        where = np.argsort(order)                     # the true partner of a[i] is b[where[i]]
        fa = [Feature(x=float(x), y=float(y)) for x, y in pairs[:, :2]]
        fb = [Feature(x=float(x), y=float(y)) for x, y in pairs[order, 2:]]
        ncc = match_brute_force(fa, fb, ImagePairScore(image_a, image_b, calculate_ncc, window))
        brief = match_brute_force(fa, fb, BriefScore(image_a, image_b))
        out["angles"].append(dict(degrees=float(angle), ncc=correct_fraction(ncc, where), brief=correct_fraction(brief, where)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--angles", type=float, nargs="+", default=[0.0, 7.0, 17.0, 45.0, 90.0, 133.0, 180.0, 251.0])
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--noise", type=float, default=0.01)
    args = ap.parse_args()
    print(json.dumps(run(args.angles, args.height, args.width, args.features, args.seed, args.noise), indent=1))
