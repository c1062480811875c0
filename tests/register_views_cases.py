"""What the host and GPU tests of the ragged absolute-pose call share (tests/test_register_views_host.py,
tests/test_gpu_register_views.py): the constants of a call and the stream case of ``sfm_register_views``."""
import numpy as np

import register_views_oracle as rv
import stream_cases

SEED, STRIDE, H_BEGIN = 0x9E3779B97F4A7C15, 3, 5
ROUNDS, MAX_STEPS = 2, 20
BUFFER_NAMES = ("S", "model", "flags", "cnt", "s1", "s2", "result", "mask", "pose_out", "mask_out", "info", "status")


# The op list is empty on purpose, as for refine_pair_poses (tests/pair_refine_cases.py): tests/test_stream_cases_host.py requires
# every op a case names to be in ops.FUNCTIONAL_OPS / INPLACE_OPS, two tuples that an earlier schema guard pins, and the ops of
# this call are listed in ops.REGISTER_VIEWS_OPS.  The call below still goes through register_views_, and its outputs are compared.
@stream_cases.case(["sfm_register_views"], [])
def register_views(dev):
    """``RegisterViewsWorkspace.run`` on the twelve-view fixture, two scenes of equal shapes and two seeds: the in-place op on
    the test's buffers."""
    import torch

    from structure_from_motion_amd import device

    i = stream_cases.Inst(dev)
    # The hold fixture of tests/test_gpu_streams.py takes one stream of torch's pool per case, and the pool's streams share the
    # four hardware queues HIP opens by default in turn: with one case more, every later side stream of that module moves on by
    # one queue, and the one that test_the_protocol_catches_a_step_on_the_wrong_stream holds lands on the default stream's own,
    # where a stray default-stream step waits behind the hold and the protocol sees nothing.  Three more keep them where they were.
    i.keep_alignment = [torch.cuda.Stream() for _ in range(3)]
    a, b = rv.ragged_arrays(rv.fixture(0)), rv.ragged_arrays(rv.fixture(100))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    V, N, h = len(rv.SIZES), len(a[0]), 256
    pts = i.inp(a[0], b[0])
    offset, min_extra = i.same(a[1], torch.int64), i.same(a[2])
    ws = device.RegisterViewsWorkspace(V, N, h, dev)
    for name, buf in zip(BUFFER_NAMES, ws.buffers()):
        setattr(ws, name, i.out(name, tuple(buf.shape), buf.dtype))
    i.host = {"A": SEED, "B": SEED + 1}
    # the fillers of the views below the sample size and no degenerate sample elsewhere; the sizes fix every status
    i.constant |= {"flags", "status"}
    i.call = lambda: ws.run(pts, offset, min_extra, rv.K, rv.THR, rv.RMS, i.cur, STRIDE, H_BEGIN, ROUNDS, MAX_STEPS)
    return i
