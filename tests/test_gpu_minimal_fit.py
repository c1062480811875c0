"""The sampling rule of the fit kernel the three minimal solvers share (csrc/sfm_minimal_fit.h): a pass that draws its
samples in the fit launch leaves, for every solver, the sample table S from which the table fit reproduces its models and
flags bit for bit, with -1 exactly at the positions past the sample that are >= n."""
import numpy as np
import pytest
import torch

from structure_from_motion_amd import device, synthetic
from structure_from_motion_amd._native import AGG_RMS
from structure_from_motion_amd.ransac.ransac import solver_sample_size

pytestmark = pytest.mark.gpu

K = synthetic.BENCH_K
BATCH, H = 2, 65                      # one lane past a full 64-lane block
PHILOX = (11, 3, 5)                   # seed, h_begin, seed_stride
SAMPLE = {"dlt": solver_sample_size("pose", "dlt"), "p3p": solver_sample_size("pose", "p3p"),
          "five_point": solver_sample_size("essential", "five_point")}


def _pose_routes(solver, n):
    pts = device.to_device(np.stack([synthetic.planar_pnp_scene(n, seed=40 + b, K=K)[0] for b in range(BATCH)]))
    ws = device.PnPWorkspace(BATCH, n, H)
    ws.run(pts, K, 4.0, 0, AGG_RMS, philox=PHILOX, solver=solver)
    fit = device.p3p_fit if solver == "p3p" else device.pnp_fit
    return ws.S, (ws.model, ws.flags), fit(pts, ws.S, K)


def _five_point_routes(n):
    corrs = []
    for b in range(BATCH):
        pa, pb, K2, *_ = synthetic.two_view_scene(n, seed=40 + b)
        corrs.append(device.normalize_correspondences(device.to_device(pa), device.to_device(pb), K2))
    corr = torch.stack(corrs)
    dev = corr.device
    S = torch.empty((BATCH, H, 8), dtype=torch.int32, device=dev)
    E = torch.empty((BATCH, H, 9), dtype=torch.float64, device=dev)
    flags, cnt = (torch.empty((BATCH, H), dtype=torch.int32, device=dev) for _ in range(2))
    s1, s2 = (torch.empty((BATCH, H), dtype=torch.float64, device=dev) for _ in range(2))
    result = torch.empty((BATCH, 5), dtype=torch.int64, device=dev)
    mask = torch.empty((BATCH, n), dtype=torch.uint8, device=dev)
    device.five_point_ransac_pass(corr, S, E, flags, cnt, s1, s2, result, mask, 2e-5, 0, AGG_RMS, philox=PHILOX)
    return S, (E, flags), device.five_point_fit(corr, S)


@pytest.mark.parametrize("extra", [0, 1, None], ids=["n=sample", "n=sample+1", "n=70"])
@pytest.mark.parametrize("solver", ["dlt", "p3p", "five_point"])
def test_philox_pass_and_table_fit_agree(solver, extra):
    sample = SAMPLE[solver]
    n = 70 if extra is None else sample + extra
    S, (model_a, flags_a), (model_b, flags_b) = _five_point_routes(n) if solver == "five_point" else _pose_routes(solver, n)
    # NaN models occur (no real solution, degenerate samples): compare the bits
    assert torch.equal(model_a.view(torch.int64), model_b.view(torch.int64))
    assert torch.equal(flags_a, flags_b)
    S = S.cpu().numpy()
    k = np.arange(8)
    assert np.array_equal(S == -1, np.broadcast_to((k >= sample) & (k >= n), S.shape))
    assert S[S != -1].min() >= 0 and S[S != -1].max() < n
