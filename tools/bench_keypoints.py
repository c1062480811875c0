"""Timing of the multi-scale keypoint detector for 1 image and for 32 images of 1920 x 1080 at the
defaults (1 000 keypoints, 8 levels, threshold 20), in one session.  Per shape one JSON line each for

  kernel       ``sfm_detect_keypoints`` on a resident pool, device events around the C call (the table upload, the memsets and
               every launch are inside);
  api          ``detect_and_describe`` from host arrays, wall clock (packing, the upload, the call, the read-back, the sort);
  harris_loop  the only other route from an image to descriptors: ``detect_harris_corners(image, 1000)`` then ``compute_brief``
               per image, wall clock.  One scale, another detector, fp64: not like for like.

The images are views of ``synthetic.similarity_texture_views``'s texture (one canvas, one rotation per image).

    python tools/bench_keypoints.py [--reps 10] [--images 1 32]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from structure_from_motion_amd import device, synthetic  # noqa: E402
from structure_from_motion_amd.feature_matching import brief  # noqa: E402
from structure_from_motion_amd.feature_matching import keypoints as kp  # noqa: E402
from structure_from_motion_amd.harris.harris_detector import detect_harris_corners  # noqa: E402

HEIGHT, WIDTH = 1080, 1920


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


def run_shape(views, reps, harris_images):
    I = len(views)
    dev = device.require_gpu()
    layout = kp.plan([v.shape for v in views], 1000, 8)
    base = dict(images=I, height=HEIGHT, width=WIDTH, planes=len(layout.rows), pool_mb=layout.pool_bytes / 1e6,
                capacity=layout.capacity)
    run = kp._run(views, 1000, 8, 20)                    # fills the pool; its buffers serve the timed calls
    offsets, boundaries = brief._pattern_on(dev)
    table = device.keypoint_plane_table(layout.rows)
    cap = layout.capacity
    out = torch.empty((16 + 50 * cap,), dtype=torch.uint8, device=dev)
    at_desc, at_ok = 16 + 16 * cap, 16 + 48 * cap
    state = dict(ws=None)

    def call():
        state["ws"] = device.detect_keypoints(
            table, len(layout.rows), I, run.pool, 20, offsets, boundaries, brief.BINS, run.score, run.kept, cap,
            out[:4].view(torch.int32), out[16:at_desc].view(torch.int32), out[at_desc:at_ok], out[at_ok:at_ok + cap],
            out[at_ok + cap:], state["ws"])

    kernel_ms = event_ms(call, reps)
    found = int(out[:4].view(torch.int32).item())
    print(json.dumps(dict(base, what="kernel", ms=kernel_ms, ms_per_image=kernel_ms / I, candidates=found, calls=run.calls,
                          workspace_mb=state["ws"].numel() / 1e6)), flush=True)
    api_ms = wall_ms(lambda: kp.detect_and_describe(views), max(reps // 3, 1))
    kept = sum(len(k.xy) for k in kp.detect_and_describe(views))
    print(json.dumps(dict(base, what="api", ms=api_ms, ms_per_image=api_ms / I, keypoints=kept)), flush=True)

    sample = views[:harris_images] if harris_images > 0 else views
    as_float = [v.astype(np.float64) for v in sample]

    def harris():
        for image, f in zip(sample, as_float):
            brief.compute_brief(image, detect_harris_corners(f, 1000))

    harris_ms = wall_ms(harris, 1) * (I / len(sample))
    print(json.dumps(dict(base, what="harris_loop", ms=harris_ms, ms_per_image=harris_ms / I, images_run=len(sample),
                          extrapolated=len(sample) != I)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--harris-images", type=int, default=4, help="images the Harris loop runs (0: all); its total is scaled")
    args = ap.parse_args()
    most = max(args.images)
    views, _ = synthetic.similarity_texture_views(HEIGHT, WIDTH, [11.0 * v for v in range(most)], [1.0] * most, seed=1)
    for count in args.images:
        run_shape(views[:count], args.reps, args.harris_images)


if __name__ == "__main__":
    main()
