"""The semi-global smoothing without a GPU (csrc/sfm_sgm.hip): the header, the binding and the op tuple agree; the
workspace size; every ValueError of the Python layer; the definition (tests/sgm_oracle.py) on hand-computed volumes, under a
transposition, and its accuracy on rendered planes."""
import numpy as np
import pytest

import plane_sweep_cases as sweep_cases
import plane_sweep_oracle as po
import sgm_cases as cases   # registers the stream case of the entry point (see that module)
import sgm_oracle as so
import stream_cases
from structure_from_motion_amd import _native, ops
from structure_from_motion_amd.stereo import depth_maps as dm


# ---- the layers agree -------------------------------------------------------------------------------------------------------------
def test_header_binding_and_ops_agree():
    import test_stream_cases_host as header

    functions = header.declared()
    params, comment = functions["sfm_sgm_aggregate"]
    assert "sfm_sgm_aggregate" in _native.SIGNATURES and params.endswith("void* stream")
    assert len(_native.SIGNATURES["sfm_sgm_aggregate"]) == params.count(",") + 1 == 17
    assert comment and header.SYNC_PHRASE not in comment
    assert "sfm_sgm_aggregate" in stream_cases.covered_entries()
    size_params, _ = functions["sfm_sgm_workspace_bytes"]
    assert size_params.count(",") + 1 == 5 and "sfm_sgm_workspace_bytes" in _native.OTHER_SYMBOLS
    assert _native.ABI_VERSION == 15
    lib = _native.load()
    assert hasattr(lib, "sfm_sgm_aggregate") and hasattr(lib, "sfm_sgm_workspace_bytes")


def test_the_sgm_ops_are_listed_beside_the_pinned_tuples():
    assert ops.SGM_OPS == ("sgm_aggregate", "sgm_aggregate_")
    others = (ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS + ops.REGISTER_VIEWS_OPS + ops.SIMILARITY_OPS +
              ops.ALIGN_MODELS_OPS + ops.DEPTH_MAP_OPS + ops.FUSION_OPS)
    assert not set(ops.SGM_OPS) & set(others)
    with open(ops.OPS_LIB_PATH.replace("libsfm_torch_ops.so", "sfm_torch_ops.cpp")) as f:
        source = f.read()
    for name in ops.SGM_OPS:
        assert f'm.def("{name}(' in source and source.count(f'm.impl("{name}",') == 2   # the device kernel and the Meta kernel
    assert dm.MAX_SGM_DEPTHS == cases.MAX_DEPTHS == 256 and dm.SGM_PATHS == tuple(sorted(so.DIRECTIONS))


def test_the_stream_case_runs_the_entry_point():
    assert [name for name, case in stream_cases.CASES.items() if "sfm_sgm_aggregate" in case.entries] == ["sgm_aggregate"]
    case = stream_cases.CASES["sgm_aggregate"]
    assert case.entries == ("sfm_sgm_aggregate",) and case.ops == () and not case.synchronising
    (va, _), (vb, _) = cases.random_volume((3, 19, 21, 37), 31), cases.random_volume((3, 19, 21, 37), 32)   # the two scenes of the case
    assert va.shape == vb.shape and not np.array_equal(va, vb, equal_nan=True)


# ---- the winner rule on hand-made columns ---------------------------------------------------------------------------------------------
def test_the_winner_rule_on_hand_made_columns():
    volume, depths, (index, depth, cost) = cases.winner_columns()
    assert volume.shape[1:] == (5, 1, 1) and len(index) >= 12
    for r, column in enumerate(cases.WINNER_COLUMNS):
        with np.errstate(all="ignore"):
            eligible = np.isfinite(volume[r]) & (np.isfinite(depths[r]) & (depths[r] > 0.0))[:, None, None]
        got = po.winners(volume[r], eligible, depths[r])
        for name, g, w in zip(("depth", "index", "cost"), got, (depth[r], index[r], cost[r])):
            assert g.shape == (1, 1) and po.same_bytes(g[0, 0], w), f"{column[0]}: {name} {g[0, 0]} for {w}"
    for paths in (4, 8):   # through the smoothing: every path of a 1 x 1 image restarts, so S = paths * C' exactly
        smooth = so.sgm_aggregate(volume, depths, paths=paths, invalid_cost=1.0)
        assert po.same_bytes(smooth["index"][:, 0, 0], index) and po.same_bytes(smooth["depth"][:, 0, 0], depth)
        assert po.same_bytes(smooth["cost"][:, 0, 0], paths * cost)
        assert po.same_bytes(smooth["aggregated"], paths * so.unary(volume, 1.0))


# ---- the workspace ------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_are_monotone_and_refused_sizes_give_minus_one():
    size = _native.load().sfm_sgm_workspace_bytes
    base = (3, 33, 48, 64)
    assert size(*base, 0) >= 3 * 33 * 48 * 64 * 8 and size(*base, 0) % 256 == 0
    assert size(*base, 1) == 0                                  # the caller's `aggregated` holds the running sum
    assert size(0, 1, 1, 1, 0) >= 0 and size(1, 1, 1, 1, 0) >= 8   # no reference: a no-op with a workspace of any size
    for at in range(4):   # the running sum grows with every size
        bigger = list(base)
        bigger[at] *= 2
        assert size(*bigger, 0) > size(*base, 0) and size(*bigger, 1) == 0
    assert size(65535, 256, 1, 2**31 - 1, 0) == ((65535 * 256 * (2**31 - 1) * 8 + 255) // 256) * 256
    refused = [(-1, 33, 48, 64), (65536, 33, 48, 64), (3, 0, 48, 64), (3, 257, 48, 64), (3, -1, 48, 64), (3, 33, 0, 64), (3, 33, 48, 0),
               (3, 33, -48, -64), (3, 33, 2**16, 2**15), (3, 33, 2**31, 1), (3, 33, 1, 2**31), (3, 33, 2**33, 2**33)]
    for sizes in refused:
        assert size(*sizes, 0) == -1 and size(*sizes, 1) == -1, sizes


# ---- the Python layer refuses before any device work -------------------------------------------------------------------------------
def _maps(volume=True):
    return dm.DepthMaps(np.zeros((2, 5, 6)), np.zeros((2, 5, 6), np.int32), np.zeros((2, 5, 6)), np.arange(2),
                        np.zeros((2, 3, 5, 6)) if volume else None, np.zeros((2, 5, 6), np.uint8))


@pytest.mark.parametrize("change", [
    dict(depth_maps_or_volume=np.zeros((3, 5, 6))), dict(depth_maps_or_volume=np.zeros((2, 0, 5, 6))),
    dict(depth_maps_or_volume=np.zeros((2, 257, 1, 1)), depths=np.ones(257)), dict(depth_maps_or_volume=np.zeros((2, 3, 0, 6))),
    dict(depth_maps_or_volume=np.zeros((2, 3, 5, 0))), dict(depth_maps_or_volume=_maps(volume=False)),
    dict(depths=np.ones(4)), dict(depths=np.ones((3, 3))), dict(depths=np.ones((2, 3, 1))),
    dict(p1=-0.1), dict(p1=np.nan), dict(p1=0.9), dict(p2=np.inf), dict(p1="a"), dict(p2=None), dict(invalid_cost=np.nan),
    dict(invalid_cost=np.inf), dict(invalid_cost=[1.0, 2.0]), dict(paths=6), dict(paths=8.0), dict(paths=True), dict(paths=0),
    dict(max_refs_per_call=0), dict(max_refs_per_call=1.5),
])
def test_regularize_depth_maps_refuses(change):
    good = dict(depth_maps_or_volume=np.zeros((2, 3, 5, 6)), depths=np.array([2.0, 3.0, 4.0]))
    with pytest.raises(ValueError):
        dm.regularize_depth_maps(**{**good, **change})


@pytest.mark.parametrize("change", [
    dict(smoothness=0.1), dict(smoothness=(0.1,)), dict(smoothness=(0.1, 0.8, 1.0)), dict(smoothness=(0.8, 0.1)),
    dict(smoothness=(-0.1, 0.8)), dict(smoothness=(0.1, np.nan)), dict(smoothness=(0.1, np.inf)), dict(smoothness=("a", "b")),
    dict(smoothness=(0.1, 0.8), depths=np.linspace(4.0, 6.0, 257)), dict(smoothness=(0.1, 0.8), radius=0),
])
def test_compute_depth_maps_refuses_a_bad_smoothness(change):
    sc = sweep_cases.scene(16, 20, views=3, seed=3)
    good = dict(images=sc["images"], K=sc["K"], poses=sc["poses"], depths=np.array([4.0, 5.0, 6.0]))
    with pytest.raises(ValueError):
        dm.compute_depth_maps(**{**good, **change})


def test_no_reference_needs_no_device():
    out = dm.regularize_depth_maps(np.zeros((0, 3, 5, 6)), np.array([2.0, 3.0, 4.0]), return_aggregated=True)
    assert out.depth.shape == out.cost.shape == (0, 5, 6) and out.index.dtype == np.int32 and out.volume.shape == (0, 3, 5, 6)
    import lib.stereo.depth_maps as drop_in

    assert drop_in.regularize_depth_maps is dm.regularize_depth_maps


# ---- the definition on hand-made volumes: small dyadic numbers, so that every sum is exact ------------------------------------------
EIGHTH = dict(p1=0.125, p2=1.0, invalid_cost=1.0)


@pytest.mark.parametrize("paths", [4, 8])
def test_one_hypothesis_sums_its_cost_once_per_path(paths):
    volume = cases.dyadic_volume((2, 1, 5, 6), 1)
    volume[0, 0, 2, 3] = np.nan
    out = so.sgm_aggregate(volume, np.array([3.0]), paths=paths, **EIGHTH)
    assert np.array_equal(out["aggregated"], paths * so.unary(volume, 1.0))
    assert out["index"][0, 2, 3] == -1 and np.isnan(out["cost"][0, 2, 3]) and np.isnan(out["depth"][0, 2, 3])
    rest = np.isfinite(volume[:, 0])
    assert np.all(out["index"][rest] == 0) and np.all(out["depth"][rest] == 3.0) and np.array_equal(out["cost"][rest], paths * volume[:, 0][rest])


def test_a_strip_worked_by_hand():
    """D = 3 on a 1 x 4 strip with p1 = 1/4 and p2 = 1.  Left to right, pixel 1 is reached from the winner d = 0 of pixel 0: for
    nothing at d = 0, for p1 at d = 1 (a step) and for p2 at d = 2 (a jump, cheaper than the 2 + p1 of its neighbour)."""
    C = np.array([[0.0, 2.0, 2.0, 2.0], [2.0, 0.0, 2.0, 2.0], [2.0, 2.0, 2.0, 0.0]]).reshape(3, 1, 4)
    right = so.path_costs(C, 1, 0, 0.25, 1.0)[:, 0]
    assert np.array_equal(right, [[0.0, 2.0, 2.25, 2.25], [2.0, 0.25, 2.0, 2.0], [2.0, 3.0, 2.25, 0.25]])
    left = so.path_costs(C, -1, 0, 0.25, 1.0)[:, 0]
    assert np.array_equal(left, [[0.25, 2.5, 3.0, 2.0], [2.0, 0.25, 2.25, 2.0], [2.25, 2.0, 2.0, 0.0]])
    for dx, dy in ((0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)):   # one row: no pixel has a predecessor
        assert np.array_equal(so.path_costs(C, dx, dy, 0.25, 1.0), C)
    out = so.sgm_aggregate(C[None], np.array([2.0, 3.0, 4.0]), 0.25, 1.0, 1.0, 4)
    assert np.array_equal(out["aggregated"][0, :, 0], ((C[:, 0] + C[:, 0]) + right) + left)
    assert out["index"][0, 0].tolist() == [0, 1, 1, 2] and out["cost"][0, 0].tolist() == [0.25, 0.5, 8.25, 0.25]


def test_without_penalties_a_path_carries_nothing():
    volume = cases.dyadic_volume((1, 5, 4, 6), 2)
    for paths in (4, 8):
        out = so.sgm_aggregate(volume, np.linspace(2.0, 3.0, 5), 0.0, 0.0, 1.0, paths)   # L = (C' + m) - m
        assert np.array_equal(out["aggregated"], paths * volume)
        assert np.array_equal(out["index"][0], volume[0].argmin(axis=0))   # argmin: the first of equal minima


def test_a_constant_volume_and_ties_go_to_the_lower_index():
    out = so.sgm_aggregate(np.full((1, 4, 3, 5), 0.5), np.array([2.0, 3.0, 4.0, 5.0]), **EIGHTH)
    assert np.all(out["index"] == 0) and np.all(out["depth"] == 2.0)
    tie = so.sgm_aggregate(np.array([3.0, 1.0, 1.0, 2.0]).reshape(1, 4, 1, 1), np.array([2.0, 3.0, 4.0, 5.0]), **EIGHTH)
    assert tie["index"][0, 0, 0] == 1 and tie["cost"][0, 0, 0] == 8.0
    # S = (24, 8, 8, 16): den = (24 - 8) + (8 - 8), o = 0.5 * 16 / 16: half a step towards d = 2, in inverse depth
    assert tie["depth"][0, 0, 0] == 1.0 / (1.0 / 3.0 + 0.5 * (1.0 / 4.0 - 1.0 / 3.0))


def test_a_pixel_without_costs_has_no_winner_and_passes_messages_on():
    volume = np.full((1, 3, 1, 3), 2.0)
    volume[0, 1, 0, 0] = volume[0, 1, 0, 2] = 0.0   # both ends agree on d = 1
    volume[0, :, 0, 1] = np.nan
    z = np.array([2.0, 3.0, 4.0])
    out = so.sgm_aggregate(volume, z, **EIGHTH)
    assert out["index"][0, 0].tolist() == [1, -1, 1] and np.isnan(out["depth"][0, 0, 1]) and np.isnan(out["cost"][0, 0, 1])
    filled = so.sgm_aggregate(np.where(np.isnan(volume), 1.0, volume), z, **EIGHTH)
    assert np.all(np.isfinite(out["aggregated"])) and np.array_equal(out["aggregated"], filled["aggregated"])
    assert filled["index"][0, 0, 1] == 1   # through the pixel in between the ends still support d = 1
    assert np.all(so.sgm_aggregate(np.full((2, 3, 4, 5), np.nan), z, **EIGHTH)["index"] == -1)   # a bad reference of the sweep


def test_an_invalid_depth_is_never_chosen():
    volume = np.full((1, 3, 2, 2), 2.0)
    volume[0, 1] = 0.0
    for bad in (-3.0, 0.0, np.nan, np.inf):
        out = so.sgm_aggregate(volume, np.array([2.0, bad, 4.0]), **EIGHTH)
        assert np.all(out["aggregated"][0, 1] < out["aggregated"][0, 0]) and np.all(out["index"] == 0) and np.all(out["depth"] == 2.0)
    infinite = volume.copy()
    infinite[0, 1, 0, 0], infinite[0, 1, 1, 1] = np.inf, -np.inf   # not finite: invalid, like a NaN
    out = so.sgm_aggregate(infinite, np.array([2.0, 3.0, 4.0]), **EIGHTH)
    assert out["index"][0].tolist() == [[0, 1], [1, 0]] and np.all(np.isfinite(out["aggregated"]))


def test_eight_paths_commute_with_a_transposition():
    volume = cases.dyadic_volume((1, 5, 6, 9), 3)
    volume[0, :, 2, 4] = np.nan
    z = np.linspace(2.0, 3.0, 5)
    straight = so.sgm_aggregate(volume, z, **EIGHTH)
    turned = so.sgm_aggregate(np.ascontiguousarray(volume.transpose(0, 1, 3, 2)), z, **EIGHTH)
    assert np.array_equal(turned["aggregated"], straight["aggregated"].transpose(0, 1, 3, 2))   # exact: only the fold order differs
    for name in ("depth", "index", "cost"):
        assert po.same_bytes(turned[name], np.ascontiguousarray(straight[name].transpose(0, 2, 1))), name


# ---- the accuracy of the definition ------------------------------------------------------------------------------------------------
def test_oracle_accuracy_on_the_three_scenes():
    slanted, two, dim = cases.accuracy("slanted"), cases.accuracy("two_planes"), cases.accuracy("dimmed")
    print("slanted", slanted, "two planes", two, "dimmed", dim)
    assert slanted["wta"][0] == sweep_cases.SLANTED_WITHIN_ONE   # (the pixels without a winner are neither right nor wrong)
    assert two["wta"] == (sweep_cases.TWO_PLANE_RIGHT_BEFORE, sweep_cases.TWO_PLANE_WRONG_BEFORE)
    assert two["wta_filtered"] == (sweep_cases.TWO_PLANE_RIGHT_AFTER, sweep_cases.TWO_PLANE_WRONG_AFTER)
    assert dim["wta"] == cases.DIMMED_WTA and dim["wta_filtered"] == cases.DIMMED_WTA_FILTERED
    # the pinned counts of the smoothed winners: at least as many right, at most as many wrong
    pinned = ((slanted["sgm"], cases.SLANTED_SGM), (two["sgm"], cases.TWO_PLANE_SGM), (two["sgm_filtered"], cases.TWO_PLANE_SGM_FILTERED),
              (dim["sgm"], cases.DIMMED_SGM), (dim["sgm_filtered"], cases.DIMMED_SGM_FILTERED))
    for (right, wrong), (want_right, want_wrong) in pinned:
        assert right >= want_right and wrong <= want_wrong
    # whatever the pinned values: smoothing loses no right depth, removes four wrong depths in ten where there is an occlusion
    # edge, and the filter then keeps more right depths and fewer wrong ones
    for scene in (slanted, two, dim):
        assert scene["sgm"][0] >= scene["wta"][0]
    for scene in (two, dim):
        assert scene["sgm"][1] <= 0.6 * scene["wta"][1]
        assert scene["sgm_filtered"][0] >= scene["wta_filtered"][0] and scene["sgm_filtered"][1] <= scene["wta_filtered"][1]
