"""The device route of fit_with_ransac before it reaches the device: which pairs take it, and the checks
every solver makes, in its order, before any device work.  ``device.require_gpu`` raises here, so a test that got past the
checks would fail with ``NoDevice``."""
import numpy as np
import pytest

import device_route_cases as drc
from device_route_cases import CASES, SOLVERS, K
from structure_from_motion_amd import device
from structure_from_motion_amd.ransac import ransac


class NoDevice(Exception):
    pass


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def raiser():
        raise NoDevice

    monkeypatch.setattr(device, "require_gpu", raiser)
    for name in ("SFM_LOCAL_OPTIMIZATION", "SFM_SAMPLER", "SFM_SEED", "SFM_DEGENERATE"):
        monkeypatch.delenv(name, raising=False)


def _fit(solver, n, max_iterations, camera_matrix=K):
    case = CASES[solver]
    data = drc.items_of(solver, drc.scene(solver, max(n, 1))[:n])
    fit, score = drc.callables(solver, camera_matrix)
    return ransac.fit_with_ransac(data, case.size, fit, score, case.threshold, max_iterations=max_iterations)


def _raises_exactly(error, text, call):
    with pytest.raises(error) as caught:
        call()
    assert str(caught.value) == text


@pytest.mark.parametrize("solver", SOLVERS)
def test_tagged_pair_routes_to_its_solver(solver):
    fit, score = drc.callables(solver)
    spec = ransac._device_spec(fit, score, CASES[solver].size)
    assert isinstance(spec, ransac.DeviceSpec) and spec.solver == solver and np.array_equal(spec.camera_matrix, K)
    assert spec.camera_matrix.dtype == np.float64
    assert ransac._device_spec(fit, score, CASES[solver].size + 1) is None


@pytest.mark.parametrize("solver", SOLVERS)
def test_too_few_items_raise_the_solvers_text(solver):
    case = CASES[solver]
    for n in (0, case.size - 1):
        _raises_exactly(ValueError, case.too_few, lambda: _fit(solver, n, 5))


@pytest.mark.parametrize("solver", SOLVERS)
def test_too_few_items_and_no_iterations(solver):
    """Eight-point, DLT and P3P return no model before they look at the size; five-point and homography look at it first."""
    case = CASES[solver]
    text = case.too_few if case.size_check_first else f"No model could be found with at least {case.size} inliers."
    _raises_exactly(ValueError, text, lambda: _fit(solver, case.size - 1, 0))
    # enough items and no iterations: no model, and still no device
    _raises_exactly(ValueError, f"No model could be found with at least {case.size} inliers.", lambda: _fit(solver, case.size, 0))


@pytest.mark.parametrize("solver", SOLVERS)
def test_enough_items_reach_the_device(solver):
    with pytest.raises(NoDevice):
        _fit(solver, CASES[solver].size, 5)


def test_five_point_refuses_local_optimisation_between_its_checks(monkeypatch):
    """After the size check, before the iterations check and before any device work."""
    monkeypatch.setenv("SFM_LOCAL_OPTIMIZATION", "1")
    text = "SFM_LOCAL_OPTIMIZATION is not supported with solver='five_point'"
    _raises_exactly(ValueError, CASES["five_point"].too_few, lambda: _fit("five_point", 5, 5))
    _raises_exactly(ValueError, text, lambda: _fit("five_point", 6, 0))
    _raises_exactly(ValueError, text, lambda: _fit("five_point", 6, 5))
    for solver in ("eight_point", "homography", "dlt", "p3p"):   # the others do not refuse it
        with pytest.raises(NoDevice):
            _fit(solver, CASES[solver].size, 5)


@pytest.mark.parametrize("solver", SOLVERS)
def test_only_the_pose_route_checks_the_camera_and_after_the_size(solver):
    """A camera matrix whose row 2 is not (0, 0, 1): ``check_camera_matrix`` refuses it."""
    case = CASES[solver]
    bad = K.copy()
    bad[2, 0] = 1e-3
    _raises_exactly(ValueError, case.too_few, lambda: _fit(solver, case.size - 1, 5, bad))
    if case.model == "pose":
        _raises_exactly(ValueError, "row 2 of the camera matrix must be (0, 0, 1)", lambda: _fit(solver, case.size, 5, bad))
    else:
        with pytest.raises(NoDevice):
            _fit(solver, case.size, 5, bad)
