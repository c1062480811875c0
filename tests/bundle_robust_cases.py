"""The inputs of the robust-loss tests beyond the regular graph ("Tests beyond the regular graph"), shared
by tests/test_bundle_robust_graphs_host.py, which calibrates each of them on the CPU (the oracle against itself under a
permutation of the observations), and tests/test_gpu_bundle_robust_graphs.py, which runs the device on them: the mixed
graphs of tests/bundle_graphs.py and the cameras and worlds of tests/geometry_cases.py with gross errors placed by
``bundle_graphs.corrupt_long_tracks``, the loss functions in 50 digits, and the grid of residuals for rho on the device."""
import functools

import mpmath
import numpy as np

import bundle_graphs as bg
import bundle_robust_oracle as bro
import geometry_cases as gc

# loss -> (loss_scale in bench pixels, the spread of a corrupted observation in bench pixels): Huber keeps a constant pull
# on an outlier and is tested on moderate ones
LOSS = {"cauchy": (2.0, 200.0), "huber": (2.0, 40.0)}
FRACTION = 0.05
STEPS = 10
CORRUPTION_SEED = 77


def corrupted(pr, loss, min_cameras=3, unit=1.0):
    """(the problem with 5 % of its observations' count in corrupted long tracks, the mask, the loss keywords)."""
    scale, spread = LOSS[loss]
    bad, mask = bg.corrupt_long_tracks(pr, FRACTION, spread * unit, CORRUPTION_SEED, min_cameras=min_cameras)
    return bad, mask, dict(loss=loss, loss_scale=scale * unit)


def args(pr):
    return (pr["K"], pr["poses"], pr["points"], pr["camera_indices"], pr["point_indices"], pr["pixels"])


def permuted(pr, seed=1):
    """The same observations in a fixed other order: only the summation order of the oracle changes."""
    perm = np.random.default_rng(seed).permutation(len(pr["pixels"]))
    return dict(pr, camera_indices=pr["camera_indices"][perm], point_indices=pr["point_indices"][perm],
                pixels=pr["pixels"][perm])


def oracle(pr, pcg, **kw):
    return (bro.adjust_pcg if pcg else bro.adjust)(*args(pr), **kw)


# ---- the mixed graphs of the parity tests: name -> (pcg, cameras, points, seed, keywords of bundle_graphs.mixed) ------------
MIXED = {
    "dense-8": (False, 8, 1500, 1, {}),
    "dense-31": (False, 31, 1500, 2, {}),     # F = 30: S in LDS, with full-length tracks
    "dense-32": (False, 32, 1500, 3, {}),     # F = 31: S in global memory, with full-length tracks
    "dense-64": (False, 64, 1500, 4, dict(full=False)),
    "pcg-65": (True, 65, 2000, 21, {}),
}
FOUR_ORDERS = ("dense-8", "pcg-65")   # run in every order of bundle_graphs.ORDERS; the others in "random"


@functools.lru_cache(maxsize=None)
def mixed_case(name, loss, order="random"):
    pcg, C, P, seed, kw = MIXED[name]
    return corrupted(bg.mixed(C, P, seed, order=order, **kw), loss)


RADIX_CAMERAS = 70000


@functools.lru_cache(maxsize=None)
def radix_case():
    """The input of test_gpu_bundle_graphs.py::test_pcg_radix_order_at_70000_cameras (three 8-bit radix passes of the
    camera order), corrupted for Cauchy -> (problem, mask, loss keywords, fixed cameras)."""
    C = RADIX_CAMERAS
    rng = np.random.default_rng(31)
    free = [1, 257, 513, 65537, 65793, 69999] + sorted(rng.choice(np.arange(2, 69999), 20, replace=False).tolist())
    pr = bg.irregular_problem(C, 70000, 31, singles=5000, pairs=15000, mid=(3, 4), duplicates=1000,
                              sparse={c: 40 for c in free}, order="camera-major")
    bad, mask, kw = corrupted(pr, "cauchy")
    return bad, mask, kw, np.setdiff1d(np.arange(C), free).tolist()


@functools.lru_cache(maxsize=None)
def all_held_case(loss):
    """Every point seen once: nothing is moving.  5 % of all observations are corrupted (each point has one)."""
    return corrupted(bg.irregular_problem(8, 1200, 12, singles=1100, unobserved=100), loss, min_cameras=1)


@functools.lru_cache(maxsize=None)
def one_camera_case(loss):
    """20 points seen twice by one camera: moving points whose V_p has rank 2."""
    return corrupted(bg.mixed(8, 1200, 14, one_camera=20), loss)


@functools.lru_cache(maxsize=None)
def blind_camera_case(loss):
    """A free camera without observations: S does not factor and every step is rejected."""
    return corrupted(bg.mixed(8, 1000, 11, sparse_count=0), loss)


# ---- cameras and worlds ----------------------------------------------------------------------------------------------------
CAMERA_STEPS = {"cauchy": 10, "huber": 5}   # Huber does not converge here and its orders part after 5 steps


@functools.lru_cache(maxsize=None)
def camera_case(camera, loss):
    """geometry_cases.bundle_case(camera, 8, 1000, 12) with the spread and the loss scale in the camera's pixel unit."""
    return corrupted(gc.bundle_case(camera, 8, 1000, 12), loss, unit=gc.PIXEL_UNIT[camera])


# ---- the losses in 50 digits -----------------------------------------------------------------------------------------------
mpmath.mp.dps = 50
RHO_BOUND = 4.0 * 2.0 ** -52
# Relative, for rho and for w, against the formulas of csrc/sfm_loss.h evaluated in 50 digits at the float64 e, a and
# a2 = fl(a * a).  Cauchy: the rounded division e / a2 moves log1p(x) by at most 1/2 ulp, since x / ((1 + x) log1p(x)) <= 1;
# log1p itself is within 2 ulp (the figure ROCm documents for its device maths library); the product with a2 adds 1/2: 3.
# Huber: sqrt, two products and a subtraction whose result is at least a2 (no cancellation): 3.  An ulp is at most 2^-52
# relative; 4 leaves one for the weights' division and sum.


def rho_mp(e, loss, a):
    """(rho, w) of one float64 e >= 0 as mpmath numbers, a2 being the float64 product the device forms."""
    e, a2, a = mpmath.mpf(float(e)), mpmath.mpf(float(a) * float(a)), mpmath.mpf(float(a))
    if loss == "huber":
        return (e, mpmath.mpf(1)) if e <= a2 else (2 * a * mpmath.sqrt(e) - a2, a / mpmath.sqrt(e))
    return a2 * mpmath.log1p(e / a2), 1 / (1 + e / a2)


def relative_error(value, exact):
    """|value - exact| / |exact| of a float64 against an mpmath number (0 where both are 0)."""
    if exact == 0:
        return 0.0 if value == 0.0 else np.inf
    return float(abs(mpmath.mpf(float(value)) - exact) / abs(exact))


RHO_SCALES = (2.0, 2.0 / 1520.0, 1000.0)


def _short(d):
    """d rounded to 26 significant bits, so that d * d is exact in float64."""
    m, x = np.frexp(d)
    return float(np.ldexp(np.round(np.ldexp(m, 26)), x - 26))


def rho_grid(a):
    """The residuals d of the grid for scale a: 0, a 2^k for k = -40, -36 .. 40 (26 significant bits: e = d d is exact), a
    itself (e == a2 bit for bit, the same product: Huber's tie takes the squared branch) and its two neighbours."""
    return [0.0] + [_short(a * 2.0 ** k) for k in range(-40, 41, 4)] + [a, float(np.nextafter(a, 0.0)),
                                                                         float(np.nextafter(a, np.inf))]


def one_observation(d):
    """One fixed camera [I | 0] with K = I, the point (0, 0, 1) and one observation at pixel (d, 0): the residual is
    (0 - d, 0) exactly and e = fl(d * d), so a call with max_steps = 0 returns initial_cost = rho(e)."""
    poses = np.zeros((1, 12))
    poses[0, :9] = np.eye(3).reshape(9)
    return dict(K=np.eye(3), poses=poses, points=np.array([[0.0, 0.0, 1.0]]), camera_indices=np.zeros(1, dtype=np.int32),
                point_indices=np.zeros(1, dtype=np.int32), pixels=np.array([[d, 0.0]]))
