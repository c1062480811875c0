"""The device route of fit_with_ransac on the MI355X against the same steps made by hand with the workspaces,
the samplers and ``inlier_order``: for every solver the same model to the bit, the same inliers in the same order as new objects,
and the same effect on the ``random`` module.  48 items x 64 hypotheses: a sample, survivors, outliers and several hypotheses
per wave."""
import os
import random

import numpy as np
import pytest
import torch

import device_route_cases as drc
from device_route_cases import CASES, SOLVERS, K
from structure_from_motion_amd.feature_matching.matching import Match
from structure_from_motion_amd.ransac.ransac import ErrorAggregationMethod, aggregation_code, fit_with_ransac

pytestmark = pytest.mark.gpu

N, ITERATIONS, MIN_EXTRA, SHUFFLE_SEED, PHILOX_SEED = 48, 64, 10, 11, 7
RMS = aggregation_code(ErrorAggregationMethod.RMS)
SAMPLERS = ("pyshuffle", "philox_seeded", "philox_unseeded")


@pytest.fixture(scope="module")
def dev(native_lib):
    from structure_from_motion_amd import device

    return device.require_gpu()


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for name in ("SFM_LOCAL_OPTIMIZATION", "SFM_SAMPLER", "SFM_SEED", "SFM_DEGENERATE"):
        monkeypatch.delenv(name, raising=False)


def _set_sampler(monkeypatch, sampler):
    if sampler != "pyshuffle":
        monkeypatch.setenv("SFM_SAMPLER", "philox")
    if sampler == "philox_seeded":
        monkeypatch.setenv("SFM_SEED", str(PHILOX_SEED))


def _upload(solver, array):
    from structure_from_motion_amd import device

    n = len(array)
    if CASES[solver].model == "pose":
        return device.to_device(array).reshape(1, n, 5)
    return device.normalize_correspondences(device.to_device(array[:, :2]), device.to_device(array[:, 2:]), K).reshape(1, n, 4)


def _workspace(solver, n, iterations, dev):
    from structure_from_motion_amd import device

    cls = {"essential": device.RansacWorkspace, "homography": device.HomographyWorkspace, "pose": device.PnPWorkspace}
    return cls[CASES[solver].model](1, n, iterations, dev)


def _draw(solver, ws, n, iterations):
    """The samples of a pass from the present ``random`` state and environment, made by hand -> (table, philox): the shuffle
    table uploaded into ws.S; or a Philox seed, the table of the eight-point pass then filled by a sampling launch."""
    from structure_from_motion_amd import device

    if os.environ.get("SFM_SAMPLER") != "philox":
        table = device.PyShuffleTable(n, iterations, random, advance=True)
        ws.S.copy_(device.to_device(table.S, dtype=torch.int32).reshape(1, iterations, 8))
        return table, None
    seed = int(os.environ["SFM_SEED"]) if "SFM_SEED" in os.environ else random.getrandbits(64)
    if solver == "eight_point":
        device.sample_philox(seed, 0, iterations, n, out=ws.S)
        return None, None
    return None, (seed, 0, 1)


def _run(solver, ws, x, philox, min_extra, threshold):
    thr = CASES[solver].threshold if threshold is None else threshold
    if CASES[solver].model == "pose":
        ws.run(x, K, thr, min_extra, RMS, philox=philox, solver=solver)
    elif solver == "homography":
        ws.run(x, thr, min_extra, RMS, philox=philox)
    else:
        ws.run(x, thr, min_extra, RMS, philox=philox, solver=solver)


def _by_hand(solver, array, dev, iterations=ITERATIONS, min_extra=MIN_EXTRA, threshold=None):
    """One pass made by hand -> (ws, x, outcome, the winner's row or None, its inliers' indices in the reference's order)."""
    from structure_from_motion_amd.epipolar._engine import inlier_order

    n = len(array)
    x = _upload(solver, array)
    ws = _workspace(solver, n, iterations, dev)
    table, philox = _draw(solver, ws, n, iterations)
    _run(solver, ws, x, philox, min_extra, threshold)
    outcome = ws.outcome(0)
    if outcome.best_h < 0:
        return ws, x, outcome, None, np.zeros(0, dtype=np.int64)
    row = ws.model[0, outcome.best_h].cpu().numpy().copy()
    return ws, x, outcome, row, inlier_order(table, outcome, CASES[solver].size)


def _flat(model):
    """A returned model as its row: a (3, 3) matrix, or (R, t)."""
    return np.concatenate([np.asarray(part).reshape(-1) for part in model]) if isinstance(model, tuple) else model.reshape(-1)


def _objects(items):
    """Every object of a list of items: the tuples and what they hold."""
    return [obj for item in items for obj in (item, *item)]


def _check_copies(solver, inliers, data, array, order):
    assert np.array_equal(drc.rows_of(solver, inliers), array[order])
    given = {id(obj) for obj in _objects(data)}
    assert not any(id(obj) in given for obj in _objects(inliers))


def _fit(solver, data, iterations=ITERATIONS, min_extra=MIN_EXTRA):
    case = CASES[solver]
    fit, score = drc.callables(solver)
    return fit_with_ransac(data, case.size, fit, score, case.threshold, min_extra, ErrorAggregationMethod.RMS, iterations)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("solver", SOLVERS)
def test_route_equals_the_steps_by_hand(dev, monkeypatch, solver, sampler):
    _set_sampler(monkeypatch, sampler)
    array = drc.scene(solver, N)
    data = drc.items_of(solver, array)
    random.seed(SHUFFLE_SEED)
    model, inliers = _fit(solver, data)
    state = random.getstate()

    random.seed(SHUFFLE_SEED)
    ws, x, outcome, row, order = _by_hand(solver, array, dev)
    assert random.getstate() == state
    # the scene does its job: a winner, survivors next to its sample, and outliers
    assert outcome.best_h >= 0 and MIN_EXTRA <= outcome.extra_inliers < N - CASES[solver].size
    assert np.array_equal(_flat(model), row)
    assert len(order) == CASES[solver].size + outcome.extra_inliers and np.array_equal(order[:CASES[solver].size], outcome.sample)
    if sampler != "pyshuffle":   # survivors in index order
        assert np.array_equal(order[CASES[solver].size:], np.nonzero(outcome.mask == 1)[0])
    _check_copies(solver, inliers, data, array, order)

    # the effect on the random module, spelled out: one shuffle per iteration; 64 bits; nothing with SFM_SEED
    random.seed(SHUFFLE_SEED)
    if sampler == "pyshuffle":
        pool = list(range(N))
        for iteration in range(ITERATIONS):
            random.shuffle(pool)
            if iteration == outcome.best_h:   # the winner's shuffled list: its sample, then the rest
                size = CASES[solver].size
                assert order.tolist() == pool[:size] + [i for i in pool[size:] if outcome.mask[i] == 1]
    elif sampler == "philox_unseeded":
        random.getrandbits(64)
    assert random.getstate() == state


@pytest.mark.parametrize("sampler", ["pyshuffle", "philox_seeded"])
@pytest.mark.parametrize("n", [N, 5])
def test_two_view_passes_equal_two_separate_passes(dev, monkeypatch, n, sampler):
    """One upload and one table against a workspace, a table and an upload per pass; at n = 5 E has no winner."""
    from structure_from_motion_amd.ransac._device_route import two_view_passes

    _set_sampler(monkeypatch, sampler)
    min_extra = MIN_EXTRA if n == N else 0
    array = drc.scene("homography", n)
    data = drc.items_of("homography", array)
    random.seed(SHUFFLE_SEED)
    got = two_view_passes(data, K, 2e-5, min_extra, RMS, ITERATIONS, "five_point")
    state = random.getstate()
    expected = []
    for solver in ("homography", "five_point"):
        if n < CASES[solver].size:
            expected.append((None, np.zeros(0, dtype=np.int64), 0))
            continue
        random.seed(SHUFFLE_SEED)
        ws, x, outcome, row, order = _by_hand(solver, array, dev, min_extra=min_extra, threshold=2e-5)   # one for both passes
        assert random.getstate() == state
        expected.append((row, order, CASES[solver].size + outcome.extra_inliers if row is not None else 0))
    assert expected[0][0] is not None and (expected[1][0] is not None) == (n == N)
    for (model, inliers, count), (row, order, want) in zip((got[:3], got[3:]), expected):
        assert (model is None and row is None) or np.array_equal(model.reshape(-1), row)
        assert count == want and len(inliers) == len(order)
        _check_copies("homography", inliers, data, array, order)


def test_two_view_passes_never_raise_on_degenerate_samples(dev, monkeypatch):
    from structure_from_motion_amd.ransac._device_route import two_view_passes

    array = drc.degenerate_scene("homography", N)
    random.seed(SHUFFLE_SEED)
    flagged = _by_hand("homography", array, dev)[2].n_flagged
    assert flagged > 0
    random.seed(SHUFFLE_SEED)
    monkeypatch.setenv("SFM_DEGENERATE", "raise")
    h, *_ = two_view_passes(drc.items_of("homography", array), K, 2e-5, MIN_EXTRA, RMS, ITERATIONS, "five_point")
    assert h is not None


def _record_calls(monkeypatch, calls, owner, name):
    real = getattr(owner, name)

    def spy(*args, **kwargs):
        calls.append(name)
        return real(*args, **kwargs)

    monkeypatch.setattr(owner, name, spy)


@pytest.mark.parametrize("solver", ["dlt", "p3p"])
def test_pnp_refinement_is_enqueued_before_the_readback(dev, monkeypatch, solver):
    """``refine_rounds=1`` against ``ws.run`` + ``ws.refine`` by hand; a kept round returns its inliers in index order."""
    from structure_from_motion_amd import device
    from structure_from_motion_amd.pnp import pnp

    array = drc.scene(solver, N)
    X, features = list(array[:, :3]), [drc.Feature(float(u), float(v)) for u, v in array[:, 3:]]
    matches = [Match(a_index=i, b_index=i) for i in range(N)]
    calls = []
    _record_calls(monkeypatch, calls, device.PnPWorkspace, "refine")
    _record_calls(monkeypatch, calls, device.PnPWorkspace, "outcome")
    random.seed(SHUFFLE_SEED)
    R, t, inliers = pnp.estimate_pose_pnp_with_ransac(K, X, features, matches, CASES[solver].threshold, MIN_EXTRA,
                                                      max_iterations=ITERATIONS, refine_rounds=1, solver=solver)
    assert calls == ["refine", "outcome"]
    state = random.getstate()

    random.seed(SHUFFLE_SEED)
    ws, x, outcome, row, order = _by_hand(solver, array, dev)
    model, mask, info = ws.refine(x, K, CASES[solver].threshold, RMS, 1, 20)
    assert random.getstate() == state and outcome.best_h >= 0
    assert device.read_pnp_refine_info(info)[0].accepted > 0   # Levenberg-Marquardt improves a minimal fit to noisy pixels
    assert np.array_equal(_flat((R, t)), model[0].cpu().numpy())
    keep = np.nonzero(mask[0].cpu().numpy())[0]
    assert np.array_equal(keep, np.sort(keep))
    data = [(X[i], features[i]) for i in range(N)]
    _check_copies(solver, inliers, data, array, keep)


def test_eight_point_local_optimisation_runs_after_the_readback(dev, monkeypatch):
    """``SFM_LOCAL_OPTIMIZATION=1`` against ``device.refine_inliers`` by hand; a kept refit returns its inliers in index order."""
    from structure_from_motion_amd import device

    monkeypatch.setenv("SFM_LOCAL_OPTIMIZATION", "1")
    array = drc.scene("eight_point", N)
    data = drc.items_of("eight_point", array)
    calls = []
    _record_calls(monkeypatch, calls, device.RansacWorkspace, "outcome")
    _record_calls(monkeypatch, calls, device, "refine_inliers")
    random.seed(SHUFFLE_SEED)
    E, inliers = _fit("eight_point", data)
    assert calls == ["outcome", "refine_inliers"]

    random.seed(SHUFFLE_SEED)
    ws, x, outcome, row, order = _by_hand("eight_point", array, dev)
    err = ws.result.view(torch.float64)[:, 2]
    E_ref, mask, info = device.refine_inliers(x, ws.E[:, outcome.best_h], ws.mask, err, CASES["eight_point"].threshold, RMS, 1)
    if device.read_refine_info(info)[0][2] > 0:
        row, order = E_ref[0].cpu().numpy(), np.nonzero(mask[0].cpu().numpy())[0]
    assert np.array_equal(E.reshape(-1), row)
    _check_copies("eight_point", inliers, data, array, order)


@pytest.mark.parametrize("solver", SOLVERS)
def test_degenerate_samples_raise_the_solvers_error_or_are_skipped(dev, monkeypatch, solver):
    """A repeated item for homography and five-point, coplanar points for eight-point and the DLT, collinear points for P3P:
    under the default policy the solver's error with its text and the flagged hypotheses of the pass made by hand; under
    ``SFM_DEGENERATE=skip`` what that pass selects (flagged hypotheses never win), or no model."""
    case = CASES[solver]
    array = drc.degenerate_scene(solver, N)
    data = drc.items_of(solver, array)
    random.seed(SHUFFLE_SEED)
    ws, x, outcome, row, order = _by_hand(solver, array, dev)
    assert outcome.n_flagged > 0 and 0 <= outcome.first_flagged < ITERATIONS
    text = f"{case.degenerate_text} (hypothesis {outcome.first_flagged}, {outcome.n_flagged} in total)"

    random.seed(SHUFFLE_SEED)
    with pytest.raises(case.error) as caught:
        _fit(solver, data)
    assert type(caught.value) is case.error and str(caught.value) == text

    monkeypatch.setenv("SFM_DEGENERATE", "skip")
    random.seed(SHUFFLE_SEED)
    if row is None:
        with pytest.raises(ValueError) as caught:
            _fit(solver, data)
        assert str(caught.value) == f"No model could be found with at least {MIN_EXTRA + case.size} inliers."
    else:
        model, inliers = _fit(solver, data)
        assert np.array_equal(_flat(model), row)
        _check_copies(solver, inliers, data, array, order)
