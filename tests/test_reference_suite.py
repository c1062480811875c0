"""The cases of the reference's OWN host-side test modules, run against this package through the drop-in `lib` path.

The inputs of those modules and the reference's answers on them are stored as data (tests/golden/g15_host_modules.npz,
g10_line_ransac.npz, g12_harris.npz, g14_ssd_integer.npz — made by tests/golden/make_golden.py from the real reference);
no reference source is stored or read here.  The cases run in a fresh interpreter whose `lib` package is this repo's (`lib/`
re-exports `structure_from_motion_amd`).  Host-only modules must give the reference's answers — they are the drop-in contract
for `lib.ransac` (generic callables), `lib.feature_matching` (matching / util), `lib.blur`, `lib.data_utils`.  Modules whose
functions are HIP kernels here (`lib.common.correlate`, `ncc`, `ssd`) cannot compute without a GPU: there every case must fail
with this package's loud "no CPU fallback" error and nothing else; with a GPU their values are checked in
tests/test_gpu_matching.py and tests/test_gpu_harris.py.  The reference's `lib/epipolar` and `lib/harris` test modules need
cv2 / tkinter: their cases are restated in tests/test_gpu_api.py.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

HOST_ONLY = {   # module -> number of cases
    "lib.blur.gaussian": 2,
    "lib.data_utils.middlebury_utils": 1,
    "lib.feature_matching.matching": 2,
    "lib.feature_matching.util": 1,
    "lib.ransac.ransac": 1,
}
DEVICE_BACKED = {
    "lib.common.correlate": 2,
    "lib.feature_matching.ncc": 3,
    "lib.feature_matching.ssd": 1,
}

RUNNER = r'''
import json, os, random, sys, tempfile
from math import sqrt
from pathlib import Path
repo, golden, modules = sys.argv[1], sys.argv[2], sys.argv[3:]
sys.path.insert(0, repo)
import numpy as np
import lib
assert lib.__file__.startswith(repo), lib.__file__
from lib.common.feature import Feature
g = lambda name: np.load(os.path.join(golden, name + ".npz"))
CASES = {}

def case(module):
    def register(fn):
        CASES.setdefault(module, []).append(fn)
        return fn
    return register

@case("lib.blur.gaussian")
def gaussian_kernels():
    from lib.blur import gaussian
    d = g("g15_host_modules")
    for size, sigma in zip(d["gauss_sizes"], d["gauss_sigmas"]):
        np.testing.assert_allclose(gaussian.create_gaussian_kernel(int(size), float(sigma)), d[f"gauss_{size}"],
                                   rtol=1e-15, atol=0)

@case("lib.blur.gaussian")
def gaussian_invalid_sizes():
    from lib.blur import gaussian
    for size in g("g15_host_modules")["gauss_invalid_sizes"]:
        try:
            gaussian.create_gaussian_kernel(int(size), 1.0)
        except ValueError:
            continue
        raise AssertionError(f"kernel size {size} accepted")

@case("lib.data_utils.middlebury_utils")
def load_camera():
    from lib.data_utils.middlebury_utils import load_camera_k_r_t
    d = g("g15_host_modules")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "par.txt"
        path.write_bytes(d["par_text"].tobytes())
        for i in (1, 2):
            K, T = load_camera_k_r_t(path, i)
            np.testing.assert_array_equal(np.asarray(K, dtype=np.float64), d[f"par_K_{i}"])
            np.testing.assert_array_equal(T.Tmat, d[f"par_T_{i}"])

def match_case(name, strategy):
    from lib.feature_matching import matching
    d = g("g15_host_modules")
    table = d[f"match_{name}_table"]
    fa = [Feature(i + 1, i + 1) for i in range(table.shape[0])]
    fb = [Feature(j + 10, j + 10) for j in range(table.shape[1])]
    ms = matching.match_brute_force(fa, fb, lambda a, b: table[fa.index(a), fb.index(b)],
                                    validation_strategies=strategy and getattr(matching.ValidationStrategy, strategy),
                                    ratio_test_threshold=float(d[f"match_{name}_thr"]))
    got = np.array([[m.a_index, m.b_index, m.match_score] for m in ms], dtype=np.float64).reshape(-1, 3)
    np.testing.assert_array_equal(got, d[f"match_{name}_out"])

case("lib.feature_matching.matching")(lambda: match_case("plain", None))
case("lib.feature_matching.matching")(lambda: match_case("ratio", "RATIO_TEST"))

@case("lib.feature_matching.util")
def within_bounds():
    from lib.feature_matching import util
    d = g("g15_host_modules")
    shape, ws = tuple(int(v) for v in d["bounds_shape"]), int(d["bounds_window"])
    got = [bool(util.is_within_bounds(Feature(x=int(x), y=int(y)), shape, ws)) for x, y in d["bounds_xy"]]
    np.testing.assert_array_equal(got, d["bounds_inside"])

@case("lib.ransac.ransac")
def line_ransac():
    from lib.ransac import ransac
    d = g("g10_line_ransac")

    def fitter(points):   # two-point line a x + b y + c = 0, as the golden vector was made
        dx = points[1][0] - points[0][0]
        if abs(dx) <= 1e-6:
            return (1.0, 0.0, -points[0][0])
        s = (points[1][1] - points[0][1]) / dx
        return (s, -1.0, points[0][1] - s * points[0][0])

    def scorer(m, p):
        return abs(m[0] * p[0] + m[1] * p[1] + m[2]) / sqrt(m[0] ** 2 + m[1] ** 2)

    points = list(d["points"])
    random.seed(5)
    model, inliers = ransac.fit_with_ransac(data=points, model_fit_data_count=2, model_fitter=fitter, inlier_scorer=scorer,
                                            inlier_threshold=0.2, min_num_extra_inliers=len(points) / 2,
                                            error_aggregation_method=ransac.ErrorAggregationMethod.RMS)
    np.testing.assert_array_equal(np.array(model), d["model"])
    np.testing.assert_array_equal(np.array(inliers), d["inliers"])

@case("lib.common.correlate")
def correlate_known_answer():
    from lib.common import correlate
    d = g("g12_harris")
    np.testing.assert_array_equal(correlate.cross_correlate(d["cc_image"], d["cc_kernel"]), d["cc_out"])

@case("lib.common.correlate")
def correlate_ones():
    from lib.common import correlate
    np.testing.assert_array_equal(correlate.cross_correlate(np.ones((5, 10)), np.ones((5, 5))), g("g12_harris")["cc_ones5"])

def ncc_case(image_b):
    from lib.feature_matching import ncc
    image_a = g("g14_ssd_integer")["unit_int_image"]
    score = ncc.calculate_ncc(image_a, image_b(image_a), Feature(2, 2), Feature(2, 2), 5)
    assert -1e-8 <= score <= 2.0 + 1e-8, score

case("lib.feature_matching.ncc")(lambda: ncc_case(np.copy))
case("lib.feature_matching.ncc")(lambda: ncc_case(np.negative))
case("lib.feature_matching.ncc")(lambda: ncc_case(lambda a: np.random.default_rng(55).random(a.shape) + 17))

@case("lib.feature_matching.ssd")
def ssd_known_answer():
    from lib.feature_matching import ssd
    d = g("g14_ssd_integer")
    img = d["unit_int_image"]
    assert ssd.calculate_ssd(img, -img, Feature(2, 2), Feature(2, 2), 5) == d["unit_int_negated"]

report = {}
for module in modules:
    passed, problems = 0, []
    for fn in CASES[module]:
        try:
            fn()
            passed += 1
        except Exception as exc:  # noqa: BLE001 - reported to the parent
            problems.append(f"{type(exc).__name__}: {exc}")
    report[module] = {"passed": passed, "problems": problems}
assert sys.modules["lib"].__file__.startswith(repo)
print("REPORT " + json.dumps(report))
'''


def run_cases(modules):
    out = subprocess.run([sys.executable, "-c", RUNNER, REPO, GOLDEN, *modules], capture_output=True, text=True,
                         cwd=REPO, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("REPORT ")][-1]
    return json.loads(line[len("REPORT "):])


def test_reference_host_side_tests_pass_unmodified():
    report = run_cases(sorted(HOST_ONLY))
    for module, expected in HOST_ONLY.items():
        assert report[module]["problems"] == [], (module, report[module])
        assert report[module]["passed"] == expected, (module, report[module])


def test_reference_device_backed_tests_fail_loudly_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: these modules compute")
    report = run_cases(sorted(DEVICE_BACKED))
    for module, cases in DEVICE_BACKED.items():
        assert report[module]["passed"] == 0 and len(report[module]["problems"]) == cases, (module, report[module])
        assert all("no CPU fallback" in p for p in report[module]["problems"]), (module, report[module])
