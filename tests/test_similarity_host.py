"""The similarity alignment without a GPU: the NumPy oracle against itself (two routes) and against known
motions, the degeneracy rule, the C ABI and its refusals, the ops and their Meta kernels, the argument checks of the public
functions and the host helpers."""
import ctypes as C

import numpy as np
import pytest

import similarity_cases as cases   # registers the stream cases of the three entry points (see that module)
import similarity_oracle as so
from structure_from_motion_amd import _native

SFM_EINVAL = -1   # include/sfm_hip.h
ENTRIES = ("sfm_similarity_ransac_pass", "sfm_similarity_fit_masked", "sfm_similarity_refine")
SIZES = ("sfm_similarity_fit_workspace_bytes", "sfm_similarity_refine_workspace_bytes")


def _truth_row(sim):
    return np.concatenate([sim[1].reshape(9), sim[2], [sim[0]]])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _route_gap(pairs, S):
    """(largest gap between the two routes over the compared samples, share of samples left out as near-degenerate)."""
    m1, f1, r1 = so.fit(pairs, S)
    m2, f2, _ = so.fit(pairs, S, so.model_horn)
    assert np.array_equal(f1, f2)
    near = cases.near_degenerate(r1)
    compared = np.nonzero((f1 == 0) & ~near)[0]
    return max([so.model_gap(m1[k], m2[k], pairs) for k in compared], default=0.0), float(np.mean(near))


@pytest.mark.parametrize("shape", cases.PARITY_SHAPES, ids=str)
def test_the_two_routes_agree_on_the_parity_fixtures_within_the_recorded_gap(shape):
    """The device's tolerance is ten times cases.ROUTE_GAP: every fixture stays inside the recorded gap, and under the cap on
    near-degenerate samples (a condition of the GPU test, confirmed here first)."""
    B, n, h = shape
    pairs = cases.parity_fixture(shape)
    for b in range(B):
        gap, near = _route_gap(pairs[b], so.sample_table(cases.SEED + b * cases.STRIDE, cases.H_BEGIN, h, n))
        print(shape, b, "gap", gap, "near-degenerate share", near)
        assert gap <= cases.ROUTE_GAP and near <= cases.NEAR_CAP


@pytest.mark.parametrize("name", list(cases.special_motions()))
def test_the_two_routes_agree_on_the_special_motions_and_fit_them(name):
    pairs, sim = cases.special_motions()[name]
    S = so.sample_table(cases.SEED, 0, 64, 64)
    gap, near = _route_gap(pairs, S)
    print(name, "gap", gap, "near-degenerate share", near)
    assert gap <= cases.ROUTE_GAP and near <= cases.NEAR_CAP
    model, flag, _ = so.model_svd(pairs[:, :3], pairs[:, 3:])
    assert flag == 0
    # the clouds 1e6 units out are stored to eps 1e6 = 1e-10 of their unit extent: that, not the solve, bounds the distance to
    # the truth there
    assert so.model_gap(model, _truth_row(sim), pairs) <= (1e-8 if name == "far_from_origin" else 1e-12)
    R = model[:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.max(np.abs(R @ R.T - np.eye(3))) < 1e-12


def test_the_oracle_recovers_a_known_similarity_and_scores_it_to_zero():
    pairs, sim, _ = cases.scene(100, 3)
    for route in (so.model_svd, so.model_horn):
        model, flag, ratio = route(pairs[:, :3], pairs[:, 3:])
        assert flag == 0 and ratio > 0.1
        assert so.model_gap(model, _truth_row(sim), pairs) < 1e-13
        assert np.max(so.error(model, pairs)) < 1e-26


def test_the_degeneracy_rule():
    pairs, _, _ = cases.scene(20, 4)
    n = len(pairs)
    # a repeated index, an index out of range
    _, flags, _ = so.fit(pairs, np.array([[0, 0, 1], [2, 5, 2], [0, 1, n], [-1, 1, 2], [0, 1, 2]]))
    assert flags.tolist() == [1, 1, 1, 1, 0]
    line = np.outer(np.array([0.0, 1.0, 2.5]), np.array([1.0, -2.0, 0.5])) + 0.3
    good = pairs[:3]
    for route in (so.model_svd, so.model_horn):
        assert route(line, good[:, 3:])[1] == 1            # three collinear points on side A
        assert route(good[:, :3], line)[1] == 1            # on side B
        assert route(np.ones((3, 3)), good[:, 3:])[1] == 1   # coincident points on side A (sa2 = 0)
        assert route(good[:, :3], np.ones((3, 3)))[1] == 1   # on side B (M = 0)
        assert route(np.full((3, 3), np.nan), good[:, 3:])[1] == 1
        flat, _ = cases.special_motions()["coplanar"]
        assert route(flat[:, :3], flat[:, 3:])[1] == 0     # a coplanar set determines the similarity
        assert route(good[:, :3], good[:, 3:])[1] == 0


def test_a_mirror_image_fits_no_more_than_its_samples():
    pairs = cases.mirror_pairs()
    S, models, flags, cnt, s1, s2, best, err, mask = so.pass_outcome(pairs, 5, 0, 64, cases.THR, len(pairs) // 2, cases.RMS)
    assert best == -1 and not mask.any() and not flags.any()
    for m in models:
        assert abs(np.linalg.det(m[:9].reshape(3, 3)) - 1.0) < 1e-12   # proper rotations only


def test_the_sampler_is_the_shared_one_and_valid_below_eight_items():
    from oracle import sfm_oracle as orc

    assert np.array_equal(so.sample_table(7, 3, 50, 64), orc.philox_sample_table(7, 3, 50, 64))
    for n in (3, 4, 7):
        S = so.sample_table(9, 0, 40, n)
        assert np.all(S[:, n:] == -1)
        assert all(sorted(row[:n]) == list(range(n)) for row in S.tolist())
    # the draws of position k do not depend on how many positions follow
    assert np.array_equal(so.sample_table(9, 0, 40, 8)[:, 0] < 8, np.ones(40, dtype=bool))


def test_the_outlier_fixture_holds_an_all_clean_sample_and_the_oracle_finds_the_clean_set():
    pairs, sim, clean, h, gate, seed = cases.outlier_fixture()
    S, models, flags, cnt, s1, s2, best, err, mask = so.pass_outcome(pairs, seed, 0, h, cases.THR, gate, cases.RMS)
    assert sum(bool(clean[row[:3]].all()) for row in S) >= 10
    assert best >= 0 and np.array_equal(mask != 0, clean)
    assert so.model_gap(models[best], _truth_row(sim), pairs) <= cases.PARITY_TOL
    # the displaced points are at least 100 x the threshold away (in the error's own, squared, unit: 1e4 x)
    assert np.min(so.error(_truth_row(sim), pairs)[~clean]) >= 1e4 * cases.THR


def test_the_refit_rounds_of_the_oracle():
    pairs, sim, clean = cases.scene(300, 8, outliers=0.3, noise=1e-4)
    S, models, flags, cnt, s1, s2, best, err, mask = so.pass_outcome(pairs, 2, 0, 64, cases.THR, 10, cases.RMS)
    model, keep, info = so.refine(pairs, models[best], mask, err, cases.THR, cases.RMS, 3)
    assert info["accepted"] >= 1 and info["count"] >= int(np.count_nonzero(mask)) and info["rounds_run"] >= info["accepted"]
    again, keep0, info0 = so.refine(pairs, models[best], mask, err, cases.THR, cases.RMS, 0)
    assert np.array_equal(again, models[best]) and info0 == dict(error=err, count=int(np.count_nonzero(mask)), accepted=0, rounds_run=0)
    none = so.refine(pairs, models[best], np.zeros(len(pairs)), err, cases.THR, cases.RMS, 2)
    assert np.array_equal(none[0], models[best]) and none[2]["count"] == 0 and none[2]["rounds_run"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI, the ops
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_signatures(native_lib):
    import test_stream_cases_host as header

    assert _native.ABI_VERSION == 15 and native_lib.sfm_abi_version() == 15
    declared = header.declared()
    for name in ENTRIES:
        assert name in _native.SIGNATURES and hasattr(native_lib, name)
        params = declared[name][0]
        assert params.endswith("void* stream") and len(params.split(",")) == len(_native.SIGNATURES[name])
    for name in SIZES:
        assert hasattr(native_lib, name) and name in declared and name in _native.OTHER_SYMBOLS
    assert native_lib.sfm_similarity_fit_workspace_bytes(1000, 2) > 0
    assert native_lib.sfm_similarity_refine_workspace_bytes(1000, 2) > native_lib.sfm_similarity_fit_workspace_bytes(1000, 2)
    for n, batch in ((2, 1), (-1, 1), (2**31, 1), (10, -1), (10, 65536)):
        assert native_lib.sfm_similarity_fit_workspace_bytes(n, batch) == -1
        assert native_lib.sfm_similarity_refine_workspace_bytes(n, batch) == -1
    assert C.sizeof(_native.SimilarityRefineInfo) == 24


def test_entry_points_refuse_bad_arguments_before_any_launch(native_lib):
    """Every refusal is an SFM_EINVAL with its reason, checked on the host: no GPU is needed to be refused."""
    lib = native_lib
    p, q = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: the calls are refused first

    def run_pass(h_begin=0, pairs=p, n=10, h=8, batch=1, agg=3, S=p, result=p):
        return lib.sfm_similarity_ransac_pass(1, 1, 1, h_begin, pairs, n, h, batch, 1e-6, 0.0, agg, S, p, p, p, p, p, result, p, None)

    def run_fit(pairs=p, n=10, batch=1, model=p, ws=p, ws_bytes=1 << 20):
        return lib.sfm_similarity_fit_masked(pairs, n, batch, None, model, p, ws, ws_bytes, None)

    def run_refine(pairs=p, n=10, batch=1, agg=3, rounds=2, mask_out=q, info=p, ws=p, ws_bytes=1 << 20):
        return lib.sfm_similarity_refine(pairs, n, batch, p, p, p, 1e-6, agg, rounds, p, mask_out, info, ws, ws_bytes, None)

    def refused(call, reason, **kw):
        assert call(**kw) == SFM_EINVAL
        assert reason in lib.sfm_last_error(), (reason, lib.sfm_last_error())
    for call in (run_pass, run_fit, run_refine):
        refused(call, b"negative size", n=-1)
        refused(call, b"negative size", batch=-1)
        refused(call, b"3 <= n", n=2)
        refused(call, b"2^31", n=2**31)
        refused(call, b"null pointer", pairs=None)
        refused(call, b"aligned", pairs=C.c_void_p(0x1008))
        assert call(batch=0) == _native.SFM_OK   # a no-op
    refused(run_pass, b"negative size", h=-1)
    refused(run_pass, b"unknown aggregation", agg=4)
    refused(run_pass, b"h_begin", h_begin=-1)
    refused(run_pass, b"null pointer", S=None)
    refused(run_pass, b"null pointer", result=None)
    refused(run_pass, b"one launch covers", batch=65536)
    refused(run_fit, b"65535", batch=65536)
    refused(run_fit, b"null pointer", model=None)
    refused(run_fit, b"null pointer", ws=None)
    refused(run_fit, b"workspace too small", ws_bytes=lib.sfm_similarity_fit_workspace_bytes(10, 1) - 1)
    refused(run_refine, b"negative size", rounds=-1)
    refused(run_refine, b"unknown aggregation", agg=-1)
    refused(run_refine, b"null pointer", info=None)
    refused(run_refine, b"alias", mask_out=p)
    refused(run_refine, b"workspace too small", ws_bytes=lib.sfm_similarity_refine_workspace_bytes(10, 1) - 1)


def test_ops_are_registered_and_listed_beside_the_pinned_tuples(native_lib):
    import torch

    from structure_from_motion_amd import ops

    op = ops.load()
    assert ops.SIMILARITY_OPS == ("similarity_ransac_pass", "similarity_ransac_pass_", "similarity_fit", "similarity_fit_",
                                  "similarity_refine", "similarity_refine_")
    assert not set(ops.SIMILARITY_OPS) & set(ops.FUNCTIONAL_OPS + ops.INPLACE_OPS + ops.LATER_FUNCTIONAL_OPS + ops.REGISTER_VIEWS_OPS)
    for name in ops.SIMILARITY_OPS:
        assert hasattr(op, name)
    assert str(op.similarity_refine.default._schema) == (
        "sfm_hip::similarity_refine(Tensor pairs, Tensor model, Tensor mask, Tensor err, float thr, int aggregation, int rounds) -> "
        "(Tensor, Tensor, Tensor)")
    assert "Tensor(a!) model_out, Tensor(b!) flags_out) -> ()" in str(op.similarity_fit_.default._schema)
    assert "Tensor(h!)? mask) -> ()" in str(op.similarity_ransac_pass_.default._schema)
    meta = dict(device="meta")
    B, n, h = 3, 700, 33
    pairs = torch.empty((B, n, 6), dtype=torch.float64, **meta)
    model, flags, cnt, s1, s2, S, result, mask = op.similarity_ransac_pass(pairs, 1, 1, 0, h, 1e-6, 0.0, 3)
    assert model.shape == (B, h, 13) and model.dtype == torch.float64 and model.device.type == "meta"
    assert flags.shape == cnt.shape == s1.shape == s2.shape == (B, h) and cnt.dtype == torch.int32 and s2.dtype == torch.float64
    assert S.shape == (B, h, 8) and result.shape == (B, 5) and mask.shape == (B, n) and mask.dtype == torch.uint8
    model, flags = op.similarity_fit(pairs, None)
    assert model.shape == (B, 13) and flags.shape == (B,) and flags.dtype == torch.int32
    model_out, mask_out, info = op.similarity_refine(pairs, model, mask, torch.empty((B,), dtype=torch.float64, **meta), 1e-6, 3, 2)
    assert model_out.shape == (B, 13) and mask_out.shape == (B, n) and info.shape == (B, 3) and info.dtype == torch.int64


def test_device_layer_names():
    from structure_from_motion_amd import device

    for name in ("run", "refine", "outcome", "buffers"):
        assert hasattr(device.SimilarityWorkspace, name)
    assert callable(device.fit_similarity) and callable(device.read_similarity_refine_info) and callable(device.similarity_refine)


# ---------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from structure_from_motion_amd import device

    def no_device(*args, **kwargs):
        raise AssertionError("device touched")

    monkeypatch.setattr(device, "require_gpu", no_device)
    monkeypatch.setattr(device, "to_device", no_device)


def test_every_value_error_is_raised_with_the_device_untouched(monkeypatch):
    from lib.multiview import alignment
    from structure_from_motion_amd.multiview import alignment as inner

    assert alignment.estimate_similarity_with_ransac is inner.estimate_similarity_with_ransac
    _no_device(monkeypatch)
    a, b = np.random.default_rng(0).normal(size=(2, 10, 3))
    bad_inputs = [(a[:, :2], b, "shape"), (a, b[:9], "equal lengths"), (a[:2], b[:2], "three pairs"), (a.reshape(-1), b, "shape")]
    nan = a.copy()
    nan[3, 1] = np.nan
    inf = b.copy()
    inf[0, 0] = np.inf
    bad_inputs += [(nan, b, "finite"), (a, inf, "finite")]
    for pa, pb, why in bad_inputs:
        with pytest.raises(ValueError, match=why):
            alignment.estimate_similarity_with_ransac(pa, pb, 1e-6)
        with pytest.raises(ValueError, match=why):
            alignment.fit_similarity(pa, pb)
    for kw, why in ((dict(inlier_threshold=float("nan")), "NaN"), (dict(min_num_extra_inliers=-1), "min_num_extra_inliers"),
                    (dict(refine_rounds=-1), "refine_rounds"), (dict(refine_rounds=1.5), "refine_rounds"),
                    (dict(iterations=2.5), "iterations"), (dict(seed="x"), "seed"), (dict(error_aggregation="median"), "error_aggregation")):
        args = dict(inlier_threshold=1e-6)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            alignment.estimate_similarity_with_ransac(a, b, **args)
    with pytest.raises(ValueError, match="mask"):
        alignment.fit_similarity(a, b, mask=np.ones(9))
    # no hypotheses: no model, and still no device
    assert alignment.estimate_similarity_with_ransac(a, b, 1e-6, iterations=0) is None
    assert alignment.estimate_similarity_with_ransac(a, b, 1e-6, iterations=-5) is None
    # valid arguments get as far as the device
    with pytest.raises(AssertionError, match="device touched"):
        alignment.estimate_similarity_with_ransac(a, b, 1e-6)
    with pytest.raises(AssertionError, match="device touched"):
        alignment.fit_similarity(a, b, mask=np.ones(10))


def test_transform_poses_keeps_every_reprojection():
    from lib.multiview import alignment
    from structure_from_motion_amd import synthetic

    sc = synthetic.multi_view_scene(views=5, points=60, seed=2, outlier_fraction=0.0)
    K = np.asarray(synthetic.BENCH_K, dtype=np.float64)
    poses, points = np.asarray(sc["poses_true"]), np.asarray(sc["points_true"])
    cam, pt, pixels = sc["camera_indices"], sc["point_indices"], sc["pixels"]
    before = cases.reprojection_errors(poses, points, cam, pt, pixels, K)
    for sim in (cases.similarity(5), cases.similarity(6, scale=1e-3), (1.0, np.eye(3), np.zeros(3))):
        after = cases.reprojection_errors(alignment.transform_poses(sim, poses), alignment.apply_similarity(sim, points), cam, pt, pixels, K)
        # pixels are ~1e3 and camera coordinates pass through two more 3 x 3 products: a few hundred eps of 1e3, squared against
        # errors of ~1 px^2 at most
        assert np.max(np.abs(after - before)) <= 1e-9 * max(1.0, float(np.max(before)))
        as_matrices = alignment.transform_poses(sim, np.concatenate([poses[:, :9].reshape(-1, 3, 3), poses[:, 9:, None]], axis=2))
        assert as_matrices.shape == (5, 3, 4)
        assert np.array_equal(as_matrices[:, :, :3].reshape(-1, 9), alignment.transform_poses(sim, poses)[:, :9])
    with pytest.raises(ValueError, match="shape"):
        alignment.transform_poses(sim, np.zeros((4, 7)))


def test_compose_and_invert_round_trip():
    from lib.multiview import alignment

    x = cases.cloud(30, 1)
    f, g = cases.similarity(1), cases.similarity(2, scale=250.0)
    both = alignment.compose(g, f)
    assert np.max(np.abs(alignment.apply_similarity(both, x) - alignment.apply_similarity(g, alignment.apply_similarity(f, x)))) < 1e-10
    back = alignment.compose(alignment.invert(f), f)
    assert abs(back[0] - 1.0) < 1e-15 and np.max(np.abs(back[1] - np.eye(3))) < 1e-15 and np.max(np.abs(back[2])) < 1e-14
    assert np.max(np.abs(alignment.apply_similarity(alignment.invert(g), alignment.apply_similarity(g, x)) - x)) < 1e-12
    est = alignment.SimilarityEstimate(f[0], f[1], f[2], np.arange(3), 0.0, False)
    inv = alignment.invert(est)
    assert isinstance(inv, alignment.SimilarityEstimate) and np.allclose(alignment.apply_similarity(inv, alignment.apply_similarity(est, x)), x)
