"""Rotation averaging timing: a ring of C cameras plus random chords, Q edges in all, 0.5 degrees of noise per
axis, squared and Huber (1 degree) from the spanning tree; ms per ``device.average_rotations`` call on resident tensors, the
steps and CG iterations it took, and the NumPy definition (tests/rotation_averaging_oracle.py, dense solver) beside it: the
whole call at the small size, one residual pass over a sample of edges at the large one (the definition is a Python loop per
edge; a full call there would take hours).  One JSON line per case.  ``python tests/perf/time_rotation_averaging.py C Q``
runs that one size without the oracle (for a profiler run)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rotation_averaging_oracle as ro
from structure_from_motion_amd import device as dev

WINDOW_S = 1.0   # calls are repeated until they fill this window (at least 5 of them)
ORACLE_SAMPLE = 20000
SIZES = ((1000, 20000), (100000, 2000000)) if len(sys.argv) < 3 else ((int(sys.argv[1]), int(sys.argv[2])),)
WITH_ORACLE = len(sys.argv) < 3


def rodrigues(v):
    """exp([v]x) of every row of v (n, 3)."""
    th = np.linalg.norm(v, axis=1)
    k = v / np.maximum(th, 1e-300)[:, None]
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * K + (1.0 - np.cos(th))[:, None, None] * (K @ K)


def graph(C, Q, seed):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(C, 3))
    R_true = rodrigues(axis / np.linalg.norm(axis, axis=1)[:, None] * rng.uniform(0.0, np.pi, size=(C, 1)))
    R_true[0] = np.eye(3)
    i = np.concatenate([np.arange(C), rng.integers(0, C, size=Q - C)])
    j = np.concatenate([(np.arange(C) + 1) % C, rng.integers(0, C, size=Q - C)])
    same = i == j
    j[same] = (j[same] + 1) % C
    flip = rng.random(Q) < 0.5
    i, j = np.where(flip, j, i), np.where(flip, i, j)
    rel = rodrigues(rng.normal(size=(Q, 3)) * np.radians(0.5)) @ R_true[j] @ np.transpose(R_true[i], (0, 2, 1))
    return R_true, np.stack([i, j], axis=1), rel


for C, Q in SIZES:
    R_true, pairs, rel = graph(C, Q, seed=7)
    args = (dev.to_device(pairs.astype(np.int32), torch.int32), dev.to_device(rel), dev.to_device(np.ones(Q)), C)
    for loss in ("squared", "huber"):
        kw = dict(loss=loss, loss_scale=np.radians(1.0))
        out = dev.average_rotations(*args, **kw)   # warm-up
        torch.cuda.synchronize()
        calls, start = [], time.perf_counter()
        while len(calls) < 5 or time.perf_counter() - start < WINDOW_S:
            t0 = time.perf_counter()
            out = dev.average_rotations(*args, **kw)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(calls))
        info = dev.read_rotavg_info(out[4])
        R = out[0].cpu().numpy()
        cos = np.clip((np.einsum("cij,cij->c", R, R_true) - 1.0) / 2.0, -1.0, 1.0)
        rec = dict(cameras=C, edges=Q, loss=loss, ms=ms, ms_min=min(calls), ms_max=max(calls), calls=len(calls), steps=info.steps, cg_iterations=info.cg_iterations, cg_max=info.cg_max,
                   status=dev.ROTAVG_STATUS[info.status], rounds=info.rounds, initial_cost=info.initial_cost,
                   final_cost=info.final_cost, max_error_deg=float(np.degrees(np.arccos(cos)).max()))
        if not WITH_ORACLE:
            print(json.dumps(rec), flush=True)
            continue
        t0 = time.perf_counter()
        if Q <= ORACLE_SAMPLE:
            want = ro.average_rotations(C, pairs, rel, loss=loss, loss_scale=np.radians(1.0), solver="dense")
            rec.update(oracle_s=time.perf_counter() - t0, oracle_steps=want["steps"], oracle="whole call, dense solver",
                       oracle_difference_rad=ro.max_rotation_difference(R, want["R"]) if want["steps"] == info.steps else None)
        else:
            ro.edge_residuals(pairs[:ORACLE_SAMPLE], rel[:ORACLE_SAMPLE], R, np.ones(ORACLE_SAMPLE, dtype=bool))
            per_edge = (time.perf_counter() - t0) / ORACLE_SAMPLE
            rec.update(oracle_s=None, oracle=f"one residual pass over {ORACLE_SAMPLE} edges",
                       oracle_residual_pass_us_per_edge=per_edge * 1e6, oracle_residual_passes_s=per_edge * Q * (info.steps + 1))
        print(json.dumps(rec), flush=True)
