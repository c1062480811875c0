"""Host side of the homography feature: the NumPy definition (tests/homography_oracle.py) on exact data, the
package's host fitter and scorer against it bit for bit, the C ABI, the ops and the argument checks of the public functions.
Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import homography_oracle as ho
from structure_from_motion_amd.common.feature import Feature
from structure_from_motion_amd.epipolar import homography as hg
from structure_from_motion_amd.feature_matching.matching import Match

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sfm_homography_fit", "sfm_homography_score", "sfm_homography_inlier_mask", "sfm_homography_ransac_pass")


@pytest.mark.parametrize("motion", ["plane_bench", "pan10"])
def test_oracle_reproduces_exact_data(motion):
    sc = ho.motion_scene(motion, 200, 3)
    S = np.array([np.random.default_rng(k).choice(200, 4, replace=False) for k in range(50)])
    H, flags, ratio = ho.fit(sc["corr"], S)
    assert not flags.any() and (ratio >= 1e-6).all()
    for k in range(50):
        assert ho.transfer_error(H[k], sc["corr"]).max() <= 1e-12
    assert np.all(ho.det(H) >= 0.0)
    assert np.abs(np.sqrt(np.sum(H * H, axis=1)) - 1.0).max() <= 1e-15
    if motion == "pan10":   # x_b ~ R x_a in K-normalised coordinates, det R = 1 > 0
        # H itself (not its action on the points) is known to rounding / (sigma_8 / sigma_1): 1e-12 needs a well-spread
        # sample, so this one takes the items nearest to the four corners of image a
        xy = sc["corr"][:, :2]
        corners = np.array([[xy[:, 0].min(), xy[:, 1].min()], [xy[:, 0].max(), xy[:, 1].min()],
                            [xy[:, 0].max(), xy[:, 1].max()], [xy[:, 0].min(), xy[:, 1].max()]])
        spread = np.array([[int(np.argmin(np.sum((xy - c) ** 2, axis=1))) for c in corners]])
        assert len(set(spread[0])) == 4
        H4, flag4, _ = ho.fit(sc["corr"], spread)
        R = sc["R"].reshape(9)
        assert flag4[0] == 0 and np.abs(H4[0] - R / np.linalg.norm(R)).max() <= 1e-12


def test_hand_made_samples():
    rows = np.arange(4)[None]
    H, flags, ratio = ho.fit(ho.REPEATED, rows)
    assert flags[0] == 1 and ratio[0] < 1e-12
    H, flags, ratio = ho.fit(ho.COLLINEAR_A, rows)
    assert flags[0] == 0 and ratio[0] > 1e-4
    assert abs(ho.det(H)[0]) < 1e-12
    # four coincident points: a non-finite scale ends in the flag; an index out of range too
    H, flags, ratio = ho.fit(np.tile(ho.COLLINEAR_A[0], (4, 1)), rows)
    assert flags[0] == 1 and np.isnan(H).all()
    assert ho.fit(ho.COLLINEAR_A, np.array([[0, 1, 2, 4]]))[1][0] == 1
    assert ho.fit(ho.COLLINEAR_A, np.array([[0, -1, 2, 3]]))[1][0] == 1


def test_host_fitter_and_scorer_equal_the_oracle_bit_for_bit():
    sc = ho.motion_scene("plane_bench", 120, 11, 0.5, 0.3)
    K, pairs = sc["K"], ho.feature_pairs(sc)
    S = np.array([np.random.default_rng(100 + k).choice(120, 4, replace=False) for k in range(40)])
    H_ref, flags, _ = ho.fit(sc["corr"], S)
    assert not flags.any()
    for k in range(40):
        H = hg.homography_model_fitter([pairs[i] for i in S[k]], K)
        assert H.shape == (3, 3) and np.array_equal(H.reshape(9), H_ref[k])
        e_ref = ho.transfer_error(H_ref[k], sc["corr"])
        got = np.array([hg.calculate_transfer_error_score(H, pair, K) for pair in pairs[:30]])
        assert np.array_equal(got, e_ref[:30])
    # a model that maps items through the line at infinity scores +inf on them, on both sides alike
    H_inf = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -10.0, 0.0, 1.0])
    e_ref = ho.transfer_error(H_inf, sc["corr"])
    got = np.array([hg.calculate_transfer_error_score(H_inf.reshape(3, 3), pair, K) for pair in pairs])
    assert np.isinf(e_ref).any() and np.isfinite(e_ref).any() and np.array_equal(got, e_ref)
    # the two hand-made samples through the host fitter
    unit_K = np.eye(3)
    as_pairs = lambda rows: [(Feature(r[0], r[1]), Feature(r[2], r[3])) for r in rows]   # noqa: E731
    with pytest.raises(hg.HomographyCalculationError):
        hg.homography_model_fitter(as_pairs(ho.REPEATED), unit_K)
    assert abs(np.linalg.det(hg.homography_model_fitter(as_pairs(ho.COLLINEAR_A), unit_K))) < 1e-12
    with pytest.raises(ValueError):
        hg.homography_model_fitter(as_pairs(ho.COLLINEAR_A[:3]), unit_K)


def test_symbols_exported_and_bound(native_lib):
    from structure_from_motion_amd import _native, build

    assert "sfm_homography.hip" in build.SOURCES
    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    with open(os.path.join(REPO, "include", "sfm_hip.h")) as f:
        header = f.read()
    assert "#define SFM_ABI_VERSION 15" in header
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert name in _native.SIGNATURES and getattr(native_lib, name) is not None
    assert "sfm_homography_sample_fit_philox" not in header   # no stand-alone Philox fit entry


def test_entries_refuse_bad_sizes_before_any_launch(native_lib):
    lib = native_lib
    bad = [(3, 10, 1), (-1, 10, 1), (10, -1, 1), (10, 10, -1), (10, 10, 65536), (2**31, 10, 1)]
    for n, h, b in bad:
        assert lib.sfm_homography_fit(None, n, None, h, b, None, None, None) != 0, (n, h, b)
        assert lib.sfm_homography_score(None, n, None, None, h, b, 1.0, None, None, None, None) != 0
        assert lib.sfm_homography_inlier_mask(None, n, None, None, h, b, None, 1.0, None, None) != 0
        assert lib.sfm_homography_ransac_pass(0, 1, 0, 0, None, n, h, b, 1.0, 0.0, 3, None, None, None, None, None, None, None,
                                              None, None) != 0
    # null pointers, an unknown aggregation and a negative h_begin are refused as well
    assert lib.sfm_homography_fit(None, 10, None, 10, 1, None, None, None) != 0
    assert lib.sfm_homography_ransac_pass(0, 1, 0, 0, None, 10, 10, 1, 1.0, 0.0, 3, None, None, None, None, None, None, None, None,
                                          None) != 0
    assert b"null pointer" in lib.sfm_last_error()
    assert lib.sfm_homography_ransac_pass(0, 1, 0, 0, None, 10, 10, 1, 1.0, 0.0, 7, None, None, None, None, None, None, None, None,
                                          None) != 0
    assert b"aggregation" in lib.sfm_last_error()
    assert lib.sfm_homography_ransac_pass(0, 1, 0, -1, None, 10, 10, 1, 1.0, 0.0, 3, None, None, None, None, None, None, None, None,
                                          None) != 0
    # empty calls are no-ops
    assert lib.sfm_homography_fit(None, 10, None, 0, 1, None, None, None) == 0
    assert lib.sfm_homography_score(None, 10, None, None, 10, 0, 1.0, None, None, None, None) == 0


def test_ops_registered_with_meta_kernels(native_lib):
    from structure_from_motion_amd import ops

    op = ops.load()
    for name in ("homography_fit", "homography_score", "homography_inlier_mask"):
        assert name in ops.FUNCTIONAL_OPS and getattr(op, name).default._schema.name == f"sfm_hip::{name}"
    assert "homography_ransac_pass_" in ops.INPLACE_OPS
    schema = str(op.homography_ransac_pass_.default._schema)
    assert "Tensor(b!) H" in schema and "Tensor(h!)? mask" in schema
    B, n, h = 2, 50, 7
    corr = torch.empty((B, n, 4), dtype=torch.float64, device="meta")
    S = torch.empty((B, h, 8), dtype=torch.int32, device="meta")
    H, flags = op.homography_fit(corr, S)
    assert H.shape == (B, h, 9) and H.dtype == torch.float64 and flags.shape == (B, h) and flags.dtype == torch.int32
    cnt, s1, s2 = op.homography_score(corr, H, S, 1e-5)
    assert cnt.shape == s1.shape == s2.shape == (B, h) and cnt.dtype == torch.int32 and s1.dtype == torch.float64
    mask = op.homography_inlier_mask(corr, H, S, torch.empty((B, 5), dtype=torch.int64, device="meta"), 1e-5)
    assert mask.shape == (B, n) and mask.dtype == torch.uint8


def test_solver_table_and_routing():
    from functools import partial

    from structure_from_motion_amd.ransac import ransac

    assert ransac.SOLVERS["homography"] == ransac.Solver("homography", 4, "homography_fitter")
    assert ransac._SCORER_ROLE["homography"] == "transfer_scorer"
    assert ransac.solver_sample_size("homography", "homography") == 4
    with pytest.raises(ValueError, match="unknown homography solver 'dlt'"):
        ransac.solver_sample_size("homography", "dlt")
    with pytest.raises(ValueError, match="unknown essential-matrix solver 'homography'"):
        ransac.solver_sample_size("essential", "homography")
    K = np.array(ho.synthetic.BENCH_K)
    fit, score = partial(hg.homography_model_fitter, camera_matrix=K), partial(hg.calculate_transfer_error_score, camera_matrix=K)
    spec = ransac._device_spec(fit, score, 4)
    assert isinstance(spec, ransac.DeviceSpec) and spec.solver == "homography" and np.array_equal(spec.camera_matrix, K)
    assert ransac._device_spec(fit, score, 6) is None
    from structure_from_motion_amd.epipolar import epipolar_ransac as er

    assert ransac._device_spec(fit, partial(er.calculate_sed_inlier_score, camera_matrix=K), 4) is None
    import lib.epipolar.homography as drop_in

    assert drop_in.estimate_homography_with_ransac is hg.estimate_homography_with_ransac
    assert drop_in.select_two_view_model is hg.select_two_view_model


def test_public_functions_refuse_bad_arguments_before_device_work():
    K = ho.synthetic.BENCH_K
    fa = [Feature(float(i), float(2 * i)) for i in range(10)]
    fb = [Feature(float(i) + 1.0, float(2 * i)) for i in range(10)]
    few = [Match(a_index=i, b_index=i) for i in range(3)]
    enough = [Match(a_index=i, b_index=i) for i in range(10)]
    bad_K = [np.eye(2), np.diag([0.0, 1.0, 1.0]), np.full((3, 3), np.nan)]
    for call in (hg.estimate_homography_with_ransac, hg.select_two_view_model):
        with pytest.raises(ValueError, match="Four feature pairs"):
            call(K, fa, fb, few, 2e-5)
        for k in bad_K:
            with pytest.raises(ValueError, match="camera matrix"):
                call(k, fa, fb, enough, 2e-5)
    with pytest.raises(ValueError, match="unknown essential-matrix solver"):
        hg.select_two_view_model(K, fa, fb, enough, 2e-5, essential_solver="seven_point")
