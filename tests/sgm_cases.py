"""What the host and GPU tests of the semi-global smoothing share (tests/test_sgm_host.py, tests/test_gpu_sgm.py;
csrc/sfm_sgm.hip): the volumes, the accuracy counts of the definition and the stream case of
``sfm_sgm_aggregate``."""
import functools

import numpy as np

import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_oracle as so
import stream_cases

NAMES = ("depth", "index", "cost", "aggregated")
SETTINGS = dict(p1=0.1, p2=0.8, invalid_cost=1.0, paths=8)
DEPTH_GROUPS = (1, 2, 4, 8, 16)            # the values of a lane in csrc/sfm_sgm.hip: one kernel each, for D up to 16 times as many
MAX_DEPTHS = 16 * DEPTH_GROUPS[-1]

# The accuracy of the definition itself (tests/test_sgm_host.py computes it on the CPU; DESIGN.md §6ak quotes it): (right, wrong),
# the interior pixels within one hypothesis of the truth and the others (plane_sweep_cases.within_one), for the winners of the
# smoothed volume with SETTINGS on the scenes of tests/plane_sweep_cases.py (5 views of 48 x 64, D = 33, radius 3) and on the
# two-plane scene dimmed to a quarter of its contrast with noise of 8 grey levels; *_FILTERED: after TWO_PLANE_FILTER.  The
# winner-takes-all counts beside them are those of the sweep alone.
SLANTED_SGM = (11720, 336)
TWO_PLANE_SGM, TWO_PLANE_SGM_FILTERED = (11467, 601), (10330, 261)
DIMMED_WTA, DIMMED_WTA_FILTERED = (9950, 2118), (8183, 540)
DIMMED_SGM, DIMMED_SGM_FILTERED = (11101, 967), (10010, 427)


def dimmed(images):
    """The images at a quarter of their contrast around grey 96, with Gaussian noise of 8 grey levels."""
    return np.clip(images * 0.25 + 96 + np.random.default_rng(0).normal(0, 8, images.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def dimmed_accuracy():
    """The sweep's oracle on the dimmed two-plane scene, as plane_sweep_cases.two_plane_accuracy: -> (sweep, filter, truth index)."""
    sc = sweep_cases.scene(48, 64, views=5, seed=2, two_planes=True)
    z = sweep_cases.hypotheses(sc, 33)
    sources = sweep_cases.nearest_sources(5, 4)
    sweep = po.plane_sweep(dimmed(sc["images"]), sc["K"], sc["poses"], np.arange(5), sources, np.broadcast_to(z, (5, 33)), 3, top_k=2)
    kept = po.filter_depth_maps(sweep["depth"], sc["K"], sc["poses"], np.arange(5), sources, **sweep_cases.TWO_PLANE_FILTER)
    return sweep, kept, sweep_cases.truth_index(sc, z)


def counts(index, depth, truth, filtered):
    """(right, wrong) of the winners ``index``; with ``filtered`` of those whose ``depth`` TWO_PLANE_FILTER keeps."""
    keep = np.ones(index.shape, dtype=bool)
    if filtered:
        sc = sweep_cases.scene(48, 64, views=5, seed=2, two_planes=True)
        kept = po.filter_depth_maps(depth, sc["K"], sc["poses"], np.arange(5), sweep_cases.nearest_sources(5, 4), **sweep_cases.TWO_PLANE_FILTER)
        keep = np.isfinite(kept["filtered"])
    return sweep_cases.within_one(index, truth, keep, 3)


@functools.lru_cache(maxsize=None)
def accuracy(name, paths=8):
    """-> dict(wta, sgm, wta_filtered, sgm_filtered) of (right, wrong) on the scene "slanted", "two_planes" or "dimmed" (the
    slanted plane has no filtered counts)."""
    if name == "slanted":
        sweep, truth, z = sweep_cases.slanted_accuracy()
    else:
        sweep, _, truth = sweep_cases.two_plane_accuracy() if name == "two_planes" else dimmed_accuracy()
        z = sweep_cases.hypotheses(sweep_cases.scene(48, 64, views=5, seed=2, two_planes=True), 33)
    smooth = so.sgm_aggregate(sweep["volume"], z, **{**SETTINGS, "paths": paths})
    out = dict(wta=counts(sweep["index"], sweep["depth"], truth, False), sgm=counts(smooth["index"], smooth["depth"], truth, False))
    if name != "slanted":
        out.update(wta_filtered=counts(sweep["index"], sweep["depth"], truth, True),
                   sgm_filtered=counts(smooth["index"], smooth["depth"], truth, True))
    return out


def random_volume(shape, seed, nan_share=0.3):
    """A volume [R, D, H, W] of costs in [0, 2] with a share of NaNs, and depths [R, D] that grow from 2 to 6."""
    rng = np.random.default_rng(seed)
    volume = rng.uniform(0.0, 2.0, size=shape)
    volume[rng.uniform(size=shape) < nan_share] = np.nan
    return volume, np.ascontiguousarray(np.broadcast_to(np.linspace(2.0, 6.0, shape[1]), shape[:2]))


def dyadic_volume(shape, seed):
    """Costs that are multiples of 1/8 in [0, 4): with penalties that are multiples of 1/8 every sum of the definition is exact."""
    return np.random.default_rng(seed).integers(0, 32, size=shape).astype(np.float64) / 8.0


# Hand-made cost columns of D = 5 hypotheses for the winner rule (plane_sweep_oracle.winners; sfmdense::DepthWinner on the device):
# (what, costs, depths, index, depth, cost), a NaN cost being a hypothesis without one.  The costs are small integers, so the
# smoothing of a 1 x 1 image, where every path restarts, turns a column c into exactly paths * c: the step is the same, since
# o = 0.5 (before - after) / den does not change when all three costs are scaled by a power of two.
# den = (before - cost) + (after - cost) == 0 cannot be reached: a hypothesis before the winner costs strictly more than the
# winner, or it would have won; the flat columns below are what comes closest.
_N = np.nan
_Z = (1.0, 2.0, 4.0, 8.0, 16.0)
WINNER_COLUMNS = (
    ("no cost at all", (_N, _N, _N, _N, _N), _Z, -1, _N, _N),
    ("winner at index 0: no step", (1, 2, 3, 4, 5), _Z, 0, 1.0, 1.0),
    ("winner at index D - 1: no step", (5, 4, 3, 2, 1), _Z, 4, 16.0, 1.0),
    ("no cost before the winner: no step", (3, _N, 1, 2, 3), _Z, 2, 4.0, 1.0),
    ("no cost after the winner: no step", (3, 2, 1, _N, 3), _Z, 2, 4.0, 1.0),
    ("a flat column: the lowest index, no step", (1, 1, 1, 1, 1), _Z, 0, 1.0, 1.0),
    ("a flat triple: its lowest index, o = 0.5 (2 - 1) / 1", (2, 1, 1, 1, 2), _Z, 1, 1.0 / (1.0 / 2.0 + 0.5 * (1.0 / 4.0 - 1.0 / 2.0)), 1.0),
    ("a step towards d + 1: o = 0.5 (4 - 2) / 4", (5, 4, 1, 2, 5), _Z, 2, 1.0 / (1.0 / 4.0 + 0.25 * (1.0 / 8.0 - 1.0 / 4.0)), 1.0),
    ("a step towards d - 1: o = 0.5 (2 - 4) / 4", (5, 2, 1, 4, 5), _Z, 2, 1.0 / (1.0 / 4.0 + 0.25 * (1.0 / 2.0 - 1.0 / 4.0)), 1.0),
    ("a symmetric triple: o = 0, the depth through 1 / (1 / z)", (5, 3, 1, 3, 5), _Z, 2, 4.0, 1.0),
    ("two equal minima: the lower index, o = 0.5 (4 - 2) / 4", (4, 1, 2, 1, 4), _Z, 1, 1.0 / (1.0 / 2.0 + 0.25 * (1.0 / 4.0 - 1.0 / 2.0)), 1.0),
    ("duplicated depths: z_j == z_i", (5, 4, 1, 2, 5), (1.0, 2.0, 4.0, 4.0, 16.0), 2, 4.0, 1.0),
    ("a negative depth at the lowest cost", (5, 4, 1, 2, 5), (1.0, 2.0, -4.0, 8.0, 16.0), 3, 8.0, 2.0),
    ("a depth of zero at the lowest cost", (5, 2, 1, 4, 5), (1.0, 2.0, 0.0, 8.0, 16.0), 1, 2.0, 2.0),
    ("a NaN depth beside the winner: no step", (5, 4, 1, 2, 5), (1.0, 2.0, 4.0, _N, 16.0), 2, 4.0, 1.0),
    ("an infinite depth at the lowest cost", (1, 4, 5, 2, 3), (np.inf, 2.0, 4.0, 8.0, 16.0), 3, 1.0 / (1.0 / 8.0 + 0.25 * (1.0 / 16.0 - 1.0 / 8.0)), 2.0),
)


def winner_columns():
    """WINNER_COLUMNS as a volume [R, 5, 1, 1] with one case per reference, depths [R, 5] and the expected (index, depth, cost) [R]."""
    costs = np.array([c[1] for c in WINNER_COLUMNS], dtype=np.float64)
    depths = np.array([c[2] for c in WINNER_COLUMNS], dtype=np.float64)
    want = tuple(np.array([c[k] for c in WINNER_COLUMNS], dtype=t) for k, t in ((3, np.int32), (4, np.float64), (5, np.float64)))
    return costs[:, :, None, None], depths, want


@functools.lru_cache(maxsize=None)
def sweep_volume(seed=21):
    """The real cost volume of four views of 37 x 45 with D = 9 (the sweep's oracle, radius 2): -> (volume, depths [4, 9])."""
    sc = sweep_cases.scene(37, 45, 4, seed=seed)
    inp = sweep_cases.sweep_inputs(sc, 9, 2)
    out = po.plane_sweep(inp["images"], inp["K"], inp["poses"], inp["refs"], inp["sources"], inp["depths"], 2)
    return out["volume"], inp["depths"]


# The op list is empty on purpose, as for the plane sweep (the comment in tests/plane_sweep_cases.py): tests/test_stream_cases_host.py
# requires every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the ops
# of this call are listed in ops.SGM_OPS.  The calls below still go through them, and their outputs are compared.
@stream_cases.case(["sfm_sgm_aggregate"], [])
def sgm_aggregate(dev):
    """The smoothing of three volumes of 21 x 37 with D = 19 along 8 paths, two scenes of equal shapes and different volumes: the
    C entry point on the test's buffers with the running sum in its workspace, and the functional op on the same inputs, which
    returns the aggregated volume."""
    import torch

    from structure_from_motion_amd import ops

    i = stream_cases.Inst(dev)
    # three spare streams of torch's pool beside this case, as in tests/plane_sweep_cases.py
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    R, D, H, W = 3, 19, 21, 37
    (va, za), (vb, zb) = random_volume((R, D, H, W), 31), random_volume((R, D, H, W), 32)
    assert not np.array_equal(va, vb, equal_nan=True)
    volume, depths = i.inp(va, vb), i.inp(za, zb * 1.01)
    depth, index = i.out("depth", (R, H, W), torch.float64), i.out("index", (R, H, W), torch.int32)
    cost = i.out("cost", (R, H, W), torch.float64)
    lib = stream_cases._lib()
    ws = i.work(lib.sfm_sgm_workspace_bytes(R, D, H, W, 0))
    op = ops.load()

    def call():
        stream_cases._check(lib.sfm_sgm_aggregate(volume.data_ptr(), R, D, H, W, depths.data_ptr(), 0.1, 0.8, 1.0, 8, depth.data_ptr(),
                                                  index.data_ptr(), cost.data_ptr(), None, ws.data_ptr(), ws.numel(), stream_cases._st()),
                            "sfm_sgm_aggregate")
        return stream_cases.Returned(op.sgm_aggregate(volume, depths, 0.1, 0.8, 1.0, 4, True))
    i.call = call
    return i
