"""Timing of the oriented BRIEF front end: `compute_brief` on 20 000 features of a 1080p image and the Hamming heap summary
of 20 000 x 20 000 descriptors — the size tests/perf/time_matcher.py times the NCC window-9 summary at.  Kernel times are
taken with device events around the C-ABI calls (inputs resident, after a warm-up), the API times are wall clock around
the public functions (uploads and the read-back included).  Prints one JSON line per measurement.

    python tools/bench_brief.py [--features 20000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from structure_from_motion_amd import _native, device  # noqa: E402
from structure_from_motion_amd.feature_matching import _device_match, brief  # noqa: E402


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n, reps = args.features, args.reps
    rng = np.random.default_rng(0)
    H, W = 1080, 1920
    image = rng.integers(0, 256, (H, W), dtype=np.uint8)
    feats = np.column_stack([rng.uniform(15, W - 16, n), rng.uniform(15, H - 16, n)])
    dev = device.require_gpu()
    lib = _native.load()
    st = device._stream()

    offsets, boundaries = brief._pattern_on(dev)
    img, ft = torch.as_tensor(image).to(dev), device.to_device(feats)
    desc = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    bins = torch.empty((n,), dtype=torch.uint8, device=dev)

    def describe():
        _native.check(lib.sfm_brief_describe(img.data_ptr(), H, W, ft.data_ptr(), n, offsets.data_ptr(), boundaries.data_ptr(),
                                             brief.BINS, desc.data_ptr(), ok.data_ptr(), bins.data_ptr(), st), "sfm_brief_describe")

    rec = dict(what="sfm_brief_describe", image=[H, W], features=n, kernel_ms=event_ms(describe, reps),
               api_ms=wall_ms(lambda: brief.compute_brief(image, feats), max(reps // 4, 1)))
    rec["features_per_s"] = n / (rec["kernel_ms"] * 1e-3)
    print(json.dumps(rec), flush=True)

    d = brief.compute_brief(image, feats)
    other = brief.compute_brief(np.ascontiguousarray(image[::-1]), feats)
    da, db = torch.as_tensor(d.bits).to(dev), torch.as_tensor(other.bits).to(dev)
    oka, okb = torch.as_tensor(d.valid.astype(np.uint8)).to(dev), torch.as_tensor(other.valid.astype(np.uint8)).to(dev)
    ws_bytes = int(lib.sfm_hamming_summary_workspace_bytes(n, n))
    ws = torch.empty((max(ws_bytes // 8, 1),), dtype=torch.float64, device=dev)
    best = torch.empty((n,), dtype=torch.float64, device=dev)
    second = torch.empty((n,), dtype=torch.float64, device=dev)
    arg = torch.empty((n,), dtype=torch.int32, device=dev)

    def summary():
        _native.check(lib.sfm_hamming_summary(da.data_ptr(), oka.data_ptr(), n, db.data_ptr(), okb.data_ptr(), n, ws.data_ptr(),
                                              ws_bytes, best.data_ptr(), arg.data_ptr(), second.data_ptr(), st), "sfm_hamming_summary")

    rec = dict(what="sfm_hamming_summary", n_a=n, n_b=n, workspace_mb=ws_bytes / 1e6, kernel_ms=event_ms(summary, reps),
               api_ms=wall_ms(lambda: _device_match.hamming_summary(d.bits, d.valid, other.bits, other.valid), max(reps // 4, 1)))
    rec["pairs_per_s"] = n * n / (rec["kernel_ms"] * 1e-3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
