"""Translation averaging timing: C cameras at random centres, a ring plus random chords, Q edges in all (about
four per camera), 0.5 degrees of noise on every direction, squared and Huber (sin 2 degrees) from the spanning tree with the
default warm-up and a fixed number of steps; ms per ``device.average_translations`` call on resident tensors, the steps and CG
iterations it took, ms per step, the largest position error after the scale-and-shift alignment, and at the small size the
NumPy definition (tests/translation_averaging_oracle.py, dense solver) beside it.  One JSON line per case.
``python tests/perf/time_translation_averaging.py C Q [STEPS]`` runs that one size without the oracle (for a profiler run)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import translation_averaging_oracle as to
from structure_from_motion_amd import device as dev

WINDOW_S = 1.0   # calls are repeated until they fill this window (at least 3 of them)
SIZES = ((100, 400), (10000, 40000), (100000, 400000)) if len(sys.argv) < 3 else ((int(sys.argv[1]), int(sys.argv[2])),)
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 50
WITH_ORACLE = len(sys.argv) < 3
ORACLE_MAX_EDGES = 1000


def graph(C, Q, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(C, 3)) * 3.0
    centres[0] = 0.0
    i = np.concatenate([np.arange(C), rng.integers(0, C, size=Q - C)])
    j = np.concatenate([(np.arange(C) + 1) % C, rng.integers(0, C, size=Q - C)])
    same = i == j
    j[same] = (j[same] + 1) % C
    flip = rng.random(Q) < 0.5
    i, j = np.where(flip, j, i), np.where(flip, i, j)
    v = to.unit(to.unit(centres[j] - centres[i]) + np.radians(0.5) * rng.normal(size=(Q, 3)))
    return centres, np.stack([i, j], axis=1), v


for C, Q in SIZES:
    centres, pairs, v = graph(C, Q, seed=7)
    args = (dev.to_device(pairs.astype(np.int32), torch.int32), dev.to_device(v), dev.to_device(np.ones(Q)), C)
    for loss in ("squared", "huber"):
        kw = dict(loss=loss, loss_scale=to.HUBER_SCALE, max_steps=STEPS, step_tolerance=1e-300)
        out = dev.average_translations(*args, **kw)   # warm-up
        torch.cuda.synchronize()
        calls, start = [], time.perf_counter()
        while len(calls) < 3 or time.perf_counter() - start < WINDOW_S:
            t0 = time.perf_counter()
            out = dev.average_translations(*args, **kw)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(calls))
        info = dev.read_transavg_info(out[5])
        c = out[0].cpu().numpy()
        rec = dict(cameras=C, edges=Q, loss=loss, ms=ms, ms_min=min(calls), ms_max=max(calls), calls=len(calls), steps=info.steps,
                   ms_per_step=ms / max(info.steps, 1), cg_iterations=info.cg_iterations, cg_max=info.cg_max,
                   status=dev.TRANSAVG_STATUS[info.status], rounds=info.rounds, initial_cost=info.initial_cost,
                   final_cost=info.final_cost, max_position_error=to.max_position_error(c, centres),
                   largest_residual_deg=float(np.degrees(np.nanmax(out[3].cpu().numpy()))))
        if WITH_ORACLE and Q <= ORACLE_MAX_EDGES:
            t0 = time.perf_counter()
            want = to.average_translations(C, pairs, v, loss=loss, loss_scale=to.HUBER_SCALE, max_steps=STEPS, step_tolerance=1e-300,
                                           solver="dense")
            rec.update(oracle_s=time.perf_counter() - t0, oracle="whole call, dense solver",
                       oracle_difference=float(np.max(np.abs(c - want["c"]))))
        print(json.dumps(rec), flush=True)
