"""Timings of the similarity alignment on the GPU (csrc/sfm_similarity.hip) for profiles/similarity/README.md: a whole pass and
its mask launch at a small and a large shape, the refinement per round, the masked fit at 10^6 items and the public call.

Device times are medians of `--repeats` runs between two events on the stream, after one warm run; the mask launch is the
difference between a pass with and without a mask, the refinement's round the difference between 3 rounds and none divided by
3.  The fit, scoring and selection launches are not separated: that needs a kernel trace.  Prints one JSON line, or with
--markdown the table of the README."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from structure_from_motion_amd import device   # noqa: E402
from structure_from_motion_amd.multiview import alignment   # noqa: E402

THR, RMS = 1e-6, 3
SHAPES = {"small": (4000, 2000), "large": (100000, 10000)}


def scene(n, seed=0, outliers=0.3, noise=3e-4):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(n, 3))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    W = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    R = np.eye(3) + np.sin(1.0) * W + (1.0 - np.cos(1.0)) * (W @ W)
    b = 1.7 * (a @ R.T) + np.array([0.5, -1.0, 2.0]) + rng.normal(scale=noise, size=(n, 3))
    bad = rng.permutation(n)[:int(outliers * n)]
    b[bad] += rng.uniform(-1.0, 1.0, size=(len(bad), 3))
    return a, b


def device_ms(call, repeats):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times)


def measure(repeats):
    dev = device.require_gpu()
    out = {"device": torch.cuda.get_device_name(dev), "repeats": repeats}
    for name, (n, h) in SHAPES.items():
        a, b = scene(n)
        pairs = device.to_device(np.hstack([a, b])).reshape(1, n, 6)
        ws = device.SimilarityWorkspace(1, n, h, dev)
        gate = n // 4
        whole = device_ms(lambda: ws.run(pairs, THR, gate, RMS, philox=(1, 0, 1)), repeats)
        no_mask = device_ms(lambda: ws.run(pairs, THR, gate, RMS, with_mask=False, philox=(1, 0, 1)), repeats)
        none = device_ms(lambda: ws.refine(pairs, THR, RMS, rounds=0), repeats)
        three = device_ms(lambda: ws.refine(pairs, THR, RMS, rounds=3), repeats)
        info = device.read_similarity_refine_info(ws.info)[0]
        t0 = time.perf_counter()
        est = alignment.estimate_similarity_with_ransac(a, b, THR, iterations=h, min_num_extra_inliers=gate, seed=1)
        host = 1e3 * (time.perf_counter() - t0)
        out[name] = {"n": n, "h": h, "pass_ms": whole, "pass_without_mask_ms": no_mask, "mask_launch_ms": whole - no_mask,
                     "refine_0_rounds_ms": none, "refine_3_rounds_ms": three, "refine_per_round_ms": (three - none) / 3.0,
                     "refine_rounds_run": info.rounds_run, "public_call_host_ms": host,
                     "inliers": None if est is None else int(len(est.inliers)), "scale": None if est is None else est.scale}
    n = 1_000_000
    a, b = scene(n, outliers=0.0)
    pairs = device.to_device(np.hstack([a, b])).reshape(1, n, 6)
    mask = torch.ones((1, n), dtype=torch.uint8, device=dev)
    buffers = (torch.empty((1, 13), dtype=torch.float64, device=dev), torch.empty((1,), dtype=torch.int32, device=dev))
    out["masked_fit"] = {"n": n, "ms": device_ms(lambda: device.fit_similarity(pairs, mask, out=buffers), repeats),
                         "null_mask_ms": device_ms(lambda: device.fit_similarity(pairs, None, out=buffers), repeats)}
    return out


def markdown(r):
    rows = ["| shape | pairs | hypotheses | whole pass | without mask | mask launch | refine, 0 rounds | refine, per round | public call (host) |",
            "|---|---|---|---|---|---|---|---|---|"]
    for name in SHAPES:
        s = r[name]
        rows.append(f"| {name} | {s['n']} | {s['h']} | {s['pass_ms']:.3f} ms | {s['pass_without_mask_ms']:.3f} ms | "
                    f"{s['mask_launch_ms']:.3f} ms | {s['refine_0_rounds_ms']:.3f} ms | {s['refine_per_round_ms']:.3f} ms | "
                    f"{s['public_call_host_ms']:.1f} ms |")
    m = r["masked_fit"]
    rows.append("")
    rows.append(f"Masked fit of {m['n']} items: {m['ms']:.3f} ms with an all-ones mask, {m['null_mask_ms']:.3f} ms with a null mask "
                f"({r['device']}, medians of {r['repeats']}).")
    return "\n".join(rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    result = measure(args.repeats)
    print(markdown(result) if args.markdown else json.dumps(result))
