"""The stream contract of the C ABI (include/sfm_hip.h: "Calls only enqueue work; nothing synchronises with the host"), as one
protocol applied to every entry point that takes a ``stream``.  tests/test_gpu_streams.py runs it on the GPU; the host test
tests/test_stream_cases_host.py keeps the tables below complete against the header and against ``ops``.

The protocol (``run_protocol``).  A case owns device-resident inputs ``In``, outputs ``Out``, every workspace ``Ws`` its entry
point takes from the caller, a callable that enqueues the call on torch's current stream, and two scenes A and B of identical
shapes and different content.

1. default stream, scene A: run, synchronise, snapshot ``OutA`` and ``WsA``;
2. default stream, scene B: run, synchronise, snapshot ``OutB`` — the expectation (the other GPU tests pin the default-stream
   result to the oracles, so no oracle is computed here);
3. non-vacuity: every compared output differs between A and B as bytes.  A case may name outputs that every valid scene
   leaves the same (``constant``: all-zero degeneracy flags, an all-zero status): they are compared in step 6 all the same;
4. restore the state a completed call on A leaves: A in ``In``, ``OutA`` in ``Out``, ``WsA`` in ``Ws``; synchronise;
5. on a side stream that a long chain of matrix products (the hold) keeps busy: copy B into ``In``, ``OutA`` into ``Out``,
   ``WsA`` into ``Ws``, check that the hold still runs, make the call and — for an entry point the header does not document as
   synchronising — check that the hold STILL runs when the call has returned: it only enqueued;
6. synchronise the side stream: ``Out`` must equal ``OutB`` byte for byte.

Why step 5 sees a launch, memset or copy that went to stream 0 instead of the caller's stream: stream 0 is not held, so the
stray step runs at once, on A's inputs and A's completed state; the restores queued on the side stream then overwrite what it
wrote, and the rest of the call runs later without it: the final ``Out`` mixes A into B.  A stray reset is overwritten by
``WsA`` and met as a stale non-zero word.  Whatever a stray step reads is a valid, completed state of another scene of the same
shapes — never a fill pattern — so a bug shows as a wrong answer, not as a wild access.

Known limit: a word whose completed state equals its reset state (the ``flag`` of ``sfm_build_tracks``, a counter that a
call leaves at zero) hides a stray reset of that word.

Outputs the header calls unordered (``sfm_compact_nonzero``, ``sfm_prune_top``, the candidates of ``sfm_detect_keypoints``)
are compared in a canonical order (``canon``); everything else as bytes.  Outputs of functional torch ops, which allocate
their results, are compared on outputs only (the tensors a call returns).

A case is driven through the lowest layer that lets the test own every buffer: the ``device.*`` wrapper where it takes all
buffers (through the torch op layer, so ``OpDevice`` / ``current_stream()`` of csrc/sfm_torch_ops.cpp are covered on the
way), else the C entry point with ``data_ptr()`` and ``torch.cuda.current_stream().cuda_stream``.
"""
import ctypes as C
import time

import numpy as np

# ------------------------------------------------------------------------------------------------------
# the tables the host test checks against include/sfm_hip.h and ops.py
# ------------------------------------------------------------------------------------------------------
# entry points whose header paragraph says the call "synchronises `stream`": they get the before-check only
SYNCHRONISING = frozenset({"sfm_bundle_adjust_pcg", "sfm_bundle_adjust_pcg_ex", "sfm_average_rotations",
                           "sfm_average_translations"})

_DEBUG = "debug / tracing entry point: writes intermediates for parity tests, not on the product path"
_HOST = "host-only: takes no stream and launches nothing"
EXEMPT = {
    "sfm_fit_stage": _DEBUG, "sfm_fit_eight_point_traced": _DEBUG, "sfm_debug_matrix_filter": _DEBUG,
}
# host-only functions are not in the guard's domain (no `stream` parameter); listed so that the reason is on record
HOST_ONLY = {
    "sfm_fit_trace_doubles": _HOST, "sfm_fold_select_records_host": _HOST, "sfm_pyshuffle_table": _HOST,
    "sfm_score_kernel_choice": _HOST, "sfm_score_kernel_choice_ex": _HOST, "sfm_score_set_default_options": _HOST,
    "sfm_score_get_default_options": _HOST,
}

CASES = {}   # name -> Case, in definition order


class Case:
    def __init__(self, name, entries, ops, build):
        self.name, self.entries, self.ops, self.build = name, tuple(entries), tuple(ops), build

    @property
    def synchronising(self):
        return any(e in SYNCHRONISING for e in self.entries)


def case(entries, ops=()):
    """Register ``build(dev) -> Inst`` as the case named after the function: ``entries`` the C entry points its call goes
    through, ``ops`` the torch ops (``ops.FUNCTIONAL_OPS`` / ``ops.INPLACE_OPS`` names) it reaches on the way."""
    def register(build):
        name = build.__name__
        assert name not in CASES
        CASES[name] = Case(name, entries, ops, build)
        return build
    return register


def covered_entries():
    return {e for c in CASES.values() for e in c.entries}


def covered_op_families():
    return {o.rstrip("_") for c in CASES.values() for o in c.ops}


# ------------------------------------------------------------------------------------------------------
# one case on the device
# ------------------------------------------------------------------------------------------------------
class Inst:
    """The buffers of one case.  ``inp(a, b)``: an input buffer with its contents in scene A and in scene B; ``out`` / ``work``:
    an output / a caller-owned workspace, zeroed.  ``host``: per-scene host arguments (a seed), read by ``call`` through
    ``self.cur``.  ``call()`` enqueues on the current stream and returns the tensors a functional op allocated (or nothing).
    ``canon(outs)``: dict of host arrays -> dict of host arrays in a canonical order.  ``constant``: see the module docstring."""

    def __init__(self, dev):
        import torch

        self.torch, self.dev = torch, dev
        self.In, self.A, self.B, self.Out, self.names, self.Ws = [], [], [], [], [], []
        self.host = {"A": None, "B": None}
        self.cur = None
        self.call = None
        self.canon = None
        self.constant = set()
        self.watch = []   # (name, input tensor the call also writes): compared, never restored from scene A

    def t(self, array, dtype=None):
        torch = self.torch
        if isinstance(array, torch.Tensor):
            return array.detach().clone().contiguous().to(self.dev)
        return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(self.dev)

    def inp(self, a, b, dtype=None):
        a, b = self.t(a, dtype), self.t(b, dtype)
        assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
        buf = self.torch.empty_like(a)
        self.In.append(buf), self.A.append(a), self.B.append(b)
        return buf

    def same(self, array, dtype=None):
        """An input both scenes share (a pattern table, an offset table of fixed shapes)."""
        return self.t(array, dtype)

    def out(self, name, shape, dtype):
        buf = self.torch.zeros(shape, dtype=dtype, device=self.dev)
        self.Out.append(buf), self.names.append(name)
        return buf

    def work(self, nbytes):
        buf = self.torch.zeros((max(int(nbytes), 16),), dtype=self.torch.uint8, device=self.dev)
        self.Ws.append(buf)
        return buf

    def load(self, scene):
        for buf, src in zip(self.In, self.A if scene == "A" else self.B):
            buf.copy_(src)
        self.cur = self.host[scene]


def _snapshot(inst, extra):
    """(device clones of Out, host arrays of Out + what the call returned)."""
    clones = [o.clone() for o in inst.Out]
    host = {n: o.cpu().numpy().copy() for n, o in zip(inst.names, inst.Out)}
    for name, t in inst.watch:
        host[name] = t.cpu().numpy().copy()
    for k, e in enumerate(extra if isinstance(extra, Returned) else ()):
        host[f"returned{k}"] = e.cpu().numpy().copy()
    return clones, (inst.canon(host) if inst.canon else host)


class Returned(tuple):
    """What ``call`` returns for tensors that a functional op allocated: compared on outputs only."""


class ProtocolFailure(AssertionError):
    pass


def run_protocol(inst, hold, synchronising=False, report=None):
    """Steps 1 to 6 of the module docstring.  ``hold()`` enqueues the hold on the current stream.  Raises ProtocolFailure with
    the step in its message."""
    torch = inst.torch
    torch.cuda.synchronize()
    inst.load("A")
    extra = inst.call()
    torch.cuda.synchronize()
    out_a, host_a = _snapshot(inst, extra)
    ws_a = [w.clone() for w in inst.Ws]
    inst.load("B")
    extra = inst.call()
    torch.cuda.synchronize()
    _, host_b = _snapshot(inst, extra)
    assert host_a.keys() == host_b.keys()
    for name in host_a:                                                   # 3: non-vacuity
        differs = host_a[name].tobytes() != host_b[name].tobytes()
        if not differs and name not in inst.constant:
            raise ProtocolFailure(f"step 3: output {name!r} is the same in scenes A and B: the case can detect nothing there")
    inst.load("A")                                                        # 4
    for o, a in zip(inst.Out, out_a):
        o.copy_(a)
    for w, a in zip(inst.Ws, ws_a):
        w.copy_(a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                                            # 5
    hold_done = torch.cuda.Event()
    with torch.cuda.stream(side):
        hold()
        hold_done.record(side)
        inst.load("B")
        for o, a in zip(inst.Out, out_a):
            o.copy_(a)
        for w, a in zip(inst.Ws, ws_a):
            w.copy_(a)
        before = hold_done.query()
        t0 = time.perf_counter()
        extra = inst.call() if not before else None
        host_time = time.perf_counter() - t0
        after = hold_done.query()
    side.synchronize()
    torch.cuda.synchronize()
    if report is not None:
        report.update(host_time=host_time, held_before=not before, held_after=not after)
    if before:
        raise ProtocolFailure("step 5: the hold had ended before the call started (hold too short)")
    if after and not synchronising:
        raise ProtocolFailure(f"step 5: the hold had ended when the call returned after {host_time * 1e3:.2f} ms on the host: "
                              "the call waited for its stream, or the hold is too short")
    _, host_s = _snapshot(inst, extra)                                    # 6
    wrong = [n for n in host_b if host_s[n].tobytes() != host_b[n].tobytes()]
    if wrong:
        stale = [n for n in wrong if host_s[n].tobytes() == host_a[n].tobytes()]
        raise ProtocolFailure(f"step 6: on the held side stream {wrong} differ from the default-stream result of scene B "
                              f"({stale} still hold scene A's result): a step of the call did not run on the caller's stream")


def host_time_on_idle_side_stream(inst):
    """Wall time of the call on the host, on an idle side stream, after one warm call."""
    torch = inst.torch
    inst.load("A")
    inst.call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        inst.load("B")
        side.synchronize()
        t0 = time.perf_counter()
        inst.call()
        elapsed = time.perf_counter() - t0
    side.synchronize()
    torch.cuda.synchronize()
    return elapsed


# ------------------------------------------------------------------------------------------------------
# scenes (the existing generators, two seeds)
# ------------------------------------------------------------------------------------------------------
THR, MIN_EXTRA, AGG_RMS = 1.5e-6, 10, 3
H_THR = 2e-5        # the homography / five-point threshold of tests/view_graph_oracle.py
PNP_THR = 4.0


def _two_view(n, seed):
    from oracle import sfm_oracle as orc

    pa, pb, K, _, _, _ = orc.synthetic_two_view(n, seed=seed, outlier_fraction=0.3)
    corr = orc.pack_correspondences(orc.to_normalized_image_coords(pa, K), orc.to_normalized_image_coords(pb, K))
    return np.ascontiguousarray(pa), np.ascontiguousarray(pb), K, np.ascontiguousarray(corr)


def _corr(n, seed, batch=1):
    return np.stack([_two_view(n, seed + 100 * b)[3] for b in range(batch)])


def _K():
    from structure_from_motion_amd import synthetic

    return synthetic.BENCH_K


def _lib():
    from structure_from_motion_amd import _native

    return _native.load()


def _st():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    from structure_from_motion_amd import _native

    _native.check(rc, what)


def _host_K():
    Kc = (C.c_double * 9)(*[float(v) for v in np.asarray(_K(), dtype=np.float64).reshape(9)])
    return Kc, C.cast(Kc, C.c_void_p)


def _finished_pass(dev, n, h, seed, solver="eight_point", batch=1):
    """A RansacWorkspace after one pass on the default stream (synchronised): the inputs of the stages behind a pass."""
    import torch

    from structure_from_motion_amd import device

    corr = torch.as_tensor(_corr(n, seed, batch)).to(dev)
    ws = device.RansacWorkspace(batch, n, h, dev)
    ws.run(corr, H_THR if solver == "five_point" else THR, MIN_EXTRA, AGG_RMS, philox=(seed, 0, 1), solver=solver)
    torch.cuda.synchronize()
    return corr, ws


def _pass_outputs(inst, batch, n, h, width=9):
    import torch

    S = inst.out("S", (batch, h, 8), torch.int32)
    model = inst.out("model", (batch, h, width), torch.float64)
    flags = inst.out("flags", (batch, h), torch.int32)
    cnt = inst.out("cnt", (batch, h), torch.int32)
    s1 = inst.out("s1", (batch, h), torch.float64)
    s2 = inst.out("s2", (batch, h), torch.float64)
    result = inst.out("result", (batch, 5), torch.int64)
    mask = inst.out("mask", (batch, n), torch.uint8)
    inst.constant.add("flags")   # no degenerate sample in either scene
    inst.host = {"A": 9, "B": 2**63 + 10}   # the Philox seed of the pass: the sample tables differ too
    return S, model, flags, cnt, s1, s2, result, mask


# ------------------------------------------------------------------------------------------------------
# two-view RANSAC
# ------------------------------------------------------------------------------------------------------
@case(["sfm_normalize_correspondences"], ["normalize_coords_"])
def normalize(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    a, b = _two_view(1000, 6), _two_view(1000, 7)
    pa, pb = i.inp(a[0], b[0]), i.inp(a[1], b[1])
    corr = i.out("corr", (1000, 4), torch.float64)
    i.call = lambda: device.normalize_correspondences(pa, pb, _K(), out=corr)
    return i


@case(["sfm_sample_philox"], ["sample_philox"])
def sample_philox(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    i.host = {"A": 5, "B": 6}
    S = i.out("S", (3, 1000, 8), torch.int32)

    def call():
        device.sample_philox(i.cur, 12345, 1000, 37, batch=3, out=S)
        return Returned([device.sample_philox(i.cur, 12345, 1000, 37, batch=3, device=dev)])
    i.call = call
    return i


@case(["sfm_sample_philox_dev"])
def sample_philox_dev(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    seed = i.inp(np.array([5], dtype=np.int64), np.array([2**62 + 11], dtype=np.int64))
    S = i.out("S", (2, 500, 8), torch.int32)
    i.call = lambda: device.sample_philox_dev(seed, 3, 500, 700, batch=2, out=S)
    return i


@case(["sfm_sample_philox_at"])
def sample_philox_at(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    at = i.inp(np.array([0, 77, 2**33 + 5, -1], dtype=np.int64), np.array([9, 78, 2**34 + 1, 3], dtype=np.int64))
    S = i.out("S", (4, 1, 8), torch.int32)
    i.call = lambda: device.sample_philox_at(9, at, 700, out=S)
    return i


def _table(dev, seed, h, n, batch=1):
    from structure_from_motion_amd import device

    return device.sample_philox(seed, 0, h, n, batch=batch, device=dev)


@case(["sfm_fit_eight_point"], ["fit_eight_point_"])
def fit_eight_point(dev):
    """Through the C ABI with lambda2, and through the in-place op."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    n, h = 700, 333
    corr = i.inp(_corr(n, 20), _corr(n, 21))
    S = i.inp(_table(dev, 7, h, n), _table(dev, 8, h, n))
    E, flags = i.out("E", (1, h, 9), torch.float64), i.out("flags", (1, h), torch.int32)
    lam = i.out("lambda2", (1, h), torch.float64)
    E2, flags2 = i.out("E_op", (1, h, 9), torch.float64), i.out("flags_op", (1, h), torch.int32)
    i.constant |= {"flags", "flags_op"}

    def call():
        device.fit_eight_point(corr, S, E, flags, lambda2=lam)
        device.fit_eight_point(corr, S, E2, flags2)
    i.call = call
    return i


@case(["sfm_sample_fit_philox"], ["sample_fit_philox_"])
def sample_fit_philox(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 3, 700, 333
    corr = i.inp(_corr(n, 20, B), _corr(n, 30, B))
    i.host = {"A": 41, "B": 2**63 + 5}
    S, E, flags = i.out("S", (B, h, 8), torch.int32), i.out("E", (B, h, 9), torch.float64), i.out("flags", (B, h), torch.int32)
    i.constant.add("flags")
    i.call = lambda: device.sample_fit_philox(corr, i.cur, 1000, S, E, flags, seed_stride=7)
    return i


def _score_case(dev, n, h, mode):
    """corr, E (fitted on the device), S -> cnt, s1, s2 with the VALU-filter kernel, the matrix kernel or the all-fp64 one."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    ca, cb = torch.as_tensor(_corr(n, 6)).to(dev), torch.as_tensor(_corr(n, 7)).to(dev)
    Sa, Sb = _table(dev, 11, h, n), _table(dev, 12, h, n)
    Ea, Eb = device.fit_eight_point(ca, Sa)[0], device.fit_eight_point(cb, Sb)[0]
    torch.cuda.synchronize()
    corr, E, S = i.inp(ca, cb), i.inp(Ea, Eb), i.inp(Sa, Sb)
    cnt, s1, s2 = i.out("cnt", (1, h), torch.int32), i.out("s1", (1, h), torch.float64), i.out("s2", (1, h), torch.float64)
    if mode == "exact":
        i.call = lambda: device.score_sed(corr, E, S, THR, cnt, s1, s2, exact_only=True)
        return i
    options = None if mode == "valu" else device.ScoreOptions(kernel="matrix", order=1)
    if options is not None:
        assert _lib().sfm_score_kernel_choice_ex(n, h, 1, C.byref(options)) == 2
    else:
        assert _lib().sfm_score_kernel_choice(n, h, 1) == 1
    ws = i.work(device.score_workspace_bytes(n, h, 1, options))
    i.call = lambda: device.score_sed(corr, E, S, THR, cnt, s1, s2, workspace=ws, options=options)
    return i


@case(["sfm_score_sed"], ["score_sed_"])
def score_sed_valu_filter(dev):
    return _score_case(dev, 4099, 300, "valu")


@case(["sfm_score_sed_ex"])
def score_sed_matrix_ordered(dev):
    """The matrix kernel with longest-first ordering: pre-pass, sort, score."""
    return _score_case(dev, 9000, 12000, "matrix")


@case(["sfm_score_sed"], ["score_sed_"])
def score_sed_exact(dev):
    return _score_case(dev, 1000, 130, "exact")


def _select_case(dev, h):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)

    def arrays(seed):
        rng = np.random.default_rng(seed)
        cnt = rng.integers(0, 40, (1, h)).astype(np.int32)
        flags = np.zeros((1, h), dtype=np.int32)
        flags[0, rng.integers(0, h, 3)] = 1
        return cnt, rng.random((1, h)), rng.random((1, h)), flags
    a, b = arrays(5), arrays(6)
    cnt, s1, s2, flags = (i.inp(x, y) for x, y in zip(a, b))
    result = i.out("result", (1, 5), torch.int64)
    i.call = lambda: device.select_best(cnt, s1, s2, flags, 10, AGG_RMS, 1_000_000, out=result)
    return i


@case(["sfm_select_best"], ["select_best_"])
def select_best_one_block(dev):
    return _select_case(dev, 5000)


@case(["sfm_select_best"], ["select_best_"])
def select_best_multi_block(dev):
    return _select_case(dev, 70000)


@case(["sfm_inlier_mask"], ["inlier_mask_"])
def inlier_mask(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    n, h = 1000, 300
    (ca, wa), (cb, wb) = _finished_pass(dev, n, h, 6), _finished_pass(dev, n, h, 7)
    corr, E, S, result = i.inp(ca, cb), i.inp(wa.E, wb.E), i.inp(wa.S, wb.S), i.inp(wa.result, wb.result)
    mask = i.out("mask", (1, n), torch.uint8)
    i.call = lambda: device.inlier_mask(corr, E, S, result, THR, out=mask)
    return i


def _single_pass_case(dev, n, h, entry, options):
    from structure_from_motion_amd import device

    i = Inst(dev)
    corr = i.inp(_corr(n, 12), _corr(n, 13))
    outs = _pass_outputs(i, 1, n, h)
    ws = i.work(device.score_workspace_bytes(n, h, 1, options))
    run = device.ransac_pass_small if entry == "small" else device.ransac_pass_large
    i.call = lambda: run(corr, *outs, ws, THR, MIN_EXTRA, AGG_RMS, 0, philox=(i.cur, 100), options=options)
    return i


@case(["sfm_ransac_pass_small"], ["ransac_pass_small_"])
def ransac_pass_small(dev):
    """600 x 4097: five selecting blocks (tests/test_gpu_parity.py::test_fused_pass_tie_between_selecting_blocks)."""
    return _single_pass_case(dev, 600, 4097, "small", None)


@case(["sfm_ransac_pass_large"])
def ransac_pass_large(dev):
    """2100 x 2064 with the matrix kernel forced: all seven launches, two ranges folded in the selection launch."""
    from structure_from_motion_amd import device

    options = device.ScoreOptions(kernel="matrix")
    assert _lib().sfm_score_kernel_choice_ex(2100, 2064, 1, C.byref(options)) == 2
    return _single_pass_case(dev, 2100, 2064, "large", options)


def _batch_pass_case(dev, batch, n, h, options):
    from structure_from_motion_amd import device

    i = Inst(dev)
    corr = i.inp(_corr(n, 50, batch), _corr(n, 60, batch))
    outs = _pass_outputs(i, batch, n, h)
    ws = i.work(device.score_workspace_bytes(n, h, batch, options))
    i.call = lambda: device.ransac_pass_batch(corr, *outs, ws, THR, MIN_EXTRA, AGG_RMS, philox=(i.cur, 100, 3), options=options)
    return i


@case(["sfm_ransac_pass_batch"])
def ransac_pass_batch(dev):
    """The smallest shape of tests/test_gpu_parity.py::test_fused_batch_pass_equals_separate_calls (the VALU filter)."""
    return _batch_pass_case(dev, 5, 700, 70, None)


@case(["sfm_ransac_pass_batch"])
def ransac_pass_batch_matrix(dev):
    """The smallest shape of that test that takes the matrix kernel: all eight launches."""
    from structure_from_motion_amd import device

    options = device.ScoreOptions(kernel="matrix")
    assert _lib().sfm_score_kernel_choice_ex(2100, 40, 17, C.byref(options)) == 2
    return _batch_pass_case(dev, 17, 2100, 40, options)


def _winner(ws):
    """(E [B,9] of the winners, err [B]) of a finished pass."""
    import torch

    rows = torch.arange(ws.batch, device=ws.result.device)
    best = ws.result[:, 1].clamp(min=0)
    return ws.model[rows, best].contiguous(), ws.result[:, 2].contiguous().view(torch.float64).clone()


@case(["sfm_refine_inliers"])
def refine_inliers(dev):
    import torch

    i = Inst(dev)
    B, n, h = 2, 1000, 300
    (ca, wa), (cb, wb) = _finished_pass(dev, n, h, 6, batch=B), _finished_pass(dev, n, h, 7, batch=B)
    (Ea, ea), (Eb, eb) = _winner(wa), _winner(wb)
    corr, E, mask, err = i.inp(ca, cb), i.inp(Ea, Eb), i.inp(wa.mask, wb.mask), i.inp(ea, eb)
    E_out, mask_out = i.out("E_out", (B, 9), torch.float64), i.out("mask_out", (B, n), torch.uint8)
    info = i.out("info", (B, 2), torch.int64)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_refine_inliers(corr.data_ptr(), n, B, E.data_ptr(), mask.data_ptr(), err.data_ptr(), THR,
                                                   AGG_RMS, 3, E_out.data_ptr(), mask_out.data_ptr(), info.data_ptr(), _st()),
                            "sfm_refine_inliers")
    return i


def _pose_stage_inputs(dev, seed, B, n, h):
    """What the pose stage reads after a pass: pixels, corr, the four candidate poses of each winner, the mask, the skip index."""
    import torch

    from structure_from_motion_amd import device

    views = [_two_view(n, seed + 100 * b) for b in range(B)]
    corr, ws = _finished_pass(dev, n, h, seed, batch=B)
    E, _ = _winner(ws)
    poses, _ = device.decompose_essential(E)
    rows = torch.arange(B, device=dev)
    skip = ws.S[rows, ws.result[:, 1].clamp(min=0), 0].contiguous()
    torch.cuda.synchronize()
    pix_a = torch.as_tensor(np.stack([v[0] for v in views])).to(dev)
    pix_b = torch.as_tensor(np.stack([v[1] for v in views])).to(dev)
    return dict(pix_a=pix_a, pix_b=pix_b, corr=corr, E=E, poses=poses, mask=ws.mask.clone(), skip=skip)


def _vote(dev, d, B, n):
    import torch

    lib = _lib()
    passes = torch.zeros((B, 4, n), dtype=torch.uint8, device=dev)
    votes, best = torch.zeros((B, 4), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
    _check(lib.sfm_cheirality_batched(d["corr"].data_ptr(), n, B, d["poses"].data_ptr(), d["mask"].data_ptr(), 50.0,
                                      passes.data_ptr(), _st()), "sfm_cheirality_batched")
    _check(lib.sfm_pose_vote(passes.data_ptr(), n, B, d["skip"].data_ptr(), votes.data_ptr(), best.data_ptr(), _st()),
           "sfm_pose_vote")
    torch.cuda.synchronize()
    return passes, best


@case(["sfm_cheirality_batched", "sfm_pose_vote"])
def cheirality_batched_pose_vote(dev):
    import torch

    i = Inst(dev)
    B, n, h = 2, 1000, 300
    a, b = _pose_stage_inputs(dev, 6, B, n, h), _pose_stage_inputs(dev, 7, B, n, h)
    corr, poses, mask, skip = (i.inp(a[k], b[k]) for k in ("corr", "poses", "mask", "skip"))
    passes = i.out("pass", (B, 4, n), torch.uint8)
    votes, best = i.out("votes", (B, 4), torch.int32), i.out("best", (B,), torch.int32)
    i.constant.add("best")   # both scenes share one true motion: the same candidate wins
    lib = _lib()

    def call():
        _check(lib.sfm_cheirality_batched(corr.data_ptr(), n, B, poses.data_ptr(), mask.data_ptr(), 50.0, passes.data_ptr(),
                                          _st()), "sfm_cheirality_batched")
        _check(lib.sfm_pose_vote(passes.data_ptr(), n, B, skip.data_ptr(), votes.data_ptr(), best.data_ptr(), _st()),
               "sfm_pose_vote")
    i.call = call
    return i


@case(["sfm_triangulate_selected"])
def triangulate_selected(dev):
    import torch

    i = Inst(dev)
    B, n, h = 2, 1000, 300
    a, b = _pose_stage_inputs(dev, 6, B, n, h), _pose_stage_inputs(dev, 7, B, n, h)
    (pass_a, best_a), (pass_b, best_b) = _vote(dev, a, B, n), _vote(dev, b, B, n)
    pix_a, pix_b, poses = (i.inp(a[k], b[k]) for k in ("pix_a", "pix_b", "poses"))
    best, passes = i.inp(best_a, best_b), i.inp(pass_a, pass_b)
    X, valid = i.out("X", (B, n, 3), torch.float64), i.out("valid", (B, n), torch.uint8)
    lib = _lib()
    Kc, Kp = _host_K()
    i.keep = Kc
    i.call = lambda: _check(lib.sfm_triangulate_selected(pix_a.data_ptr(), pix_b.data_ptr(), n, B, Kp, poses.data_ptr(),
                                                         best.data_ptr(), passes.data_ptr(), X.data_ptr(), valid.data_ptr(),
                                                         _st()), "sfm_triangulate_selected")
    return i


@case(["sfm_sed_values"])
def sed_values(dev):
    import torch

    i = Inst(dev)
    n = 3000
    rng = np.random.default_rng(0)
    corr, E = i.inp(_corr(n, 6)[0], _corr(n, 7)[0]), i.inp(rng.normal(size=9), rng.normal(size=9))
    out = i.out("sed", (n,), torch.float64)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_sed_values(corr.data_ptr(), n, E.data_ptr(), out.data_ptr(), _st()), "sfm_sed_values")
    return i


@case(["sfm_cheirality"], ["cheirality"])
def cheirality(dev):
    from structure_from_motion_amd import device

    i = Inst(dev)
    n = 1000
    a, b = _pose_stage_inputs(dev, 6, 1, n, 300), _pose_stage_inputs(dev, 7, 1, n, 300)
    corr, poses = i.inp(a["corr"][0], b["corr"][0]), i.inp(a["poses"][0], b["poses"][0])
    i.call = lambda: Returned([device.cheirality(corr, poses, 50.0)])
    return i


@case(["sfm_triangulate"], ["triangulate"])
def triangulate(dev):
    from structure_from_motion_amd import device

    i = Inst(dev)
    n = 1000
    a, b = _pose_stage_inputs(dev, 6, 1, n, 300), _pose_stage_inputs(dev, 7, 1, n, 300)
    corr = i.inp(a["corr"][0], b["corr"][0])
    P1 = i.same(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12))

    def camera(d):
        rt = d["poses"][0, 0].cpu().numpy()
        return np.hstack([rt[:9].reshape(3, 3), rt[9:].reshape(3, 1)]).reshape(12)
    P2 = i.inp(camera(a), camera(b))
    i.call = lambda: Returned([device.triangulate(corr, P1, P2)])
    return i


@case(["sfm_decompose_essential"])
def decompose_essential(dev):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    a, b = _pose_stage_inputs(dev, 6, 2, 1000, 300), _pose_stage_inputs(dev, 7, 2, 1000, 300)
    E = i.inp(a["E"], b["E"])
    poses, status = i.out("pose_rt", (2, 4, 12), torch.float64), i.out("status", (2,), torch.int32)
    i.constant.add("status")   # every winner is an essential matrix: status 0
    i.call = lambda: device.decompose_essential(E, out=(poses, status))
    return i


@case(["sfm_fold_select_records"])
def fold_select_records(dev):
    import torch

    i = Inst(dev)
    world, batch = 4, 3

    def records(seed):
        rng = np.random.default_rng(seed)
        rec = np.zeros((world, batch, 5), dtype=np.int64)
        err = rng.random((world, batch))
        rec[:, :, 0] = err.view(np.int64)
        rec[:, :, 1] = rng.integers(0, 1000, (world, batch)) + 1000 * np.arange(world)[:, None]
        rec[:, :, 2] = err.view(np.int64)
        rec[:, :, 3] = np.iinfo(np.int64).max
        rec[:, :, 4] = rng.integers(0, 50, (world, batch)).astype(np.int64) << 32
        return rec
    gathered = i.inp(records(1), records(2))
    glob, best_h = i.out("global", (batch, 5), torch.int64), i.out("best_h", (batch,), torch.int64)
    single = i.out("single", (batch, 5), torch.int64)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_fold_select_records(gathered.data_ptr(), world, batch, glob.data_ptr(), best_h.data_ptr(),
                                                        single.data_ptr(), _st()), "sfm_fold_select_records")
    return i


@case(["sfm_hartley_normalize"])
def hartley_normalize(dev):
    import torch

    i = Inst(dev)
    n = 300
    coords = i.inp(_two_view(n, 6)[0], _two_view(n, 7)[0])
    out = i.out("normalised", (2 * n + 3,), torch.float64)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_hartley_normalize(coords.data_ptr(), n, out.data_ptr(), _st()), "sfm_hartley_normalize")
    return i


# ------------------------------------------------------------------------------------------------------
# minimal-solver passes
# ------------------------------------------------------------------------------------------------------
def _pnp_pts(n, seed, batch=1):
    import pnp_oracle as po

    return np.stack([po.scene(n, seed + 100 * b, _K(), 0.3, 0.5)[0] for b in range(batch)])


def _pose_pass_case(dev, solver):
    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    pts = i.inp(_pnp_pts(n, 3, B), _pnp_pts(n, 4, B))
    ws = device.PnPWorkspace(B, n, h, dev)
    ws.S, ws.model, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask = _pass_outputs(i, B, n, h, 12)
    i.call = lambda: ws.run(pts, _K(), PNP_THR, MIN_EXTRA, AGG_RMS, philox=(i.cur, 100, 3), solver=solver)
    return i


@case(["sfm_pnp_ransac_pass"], ["pnp_ransac_pass_"])
def pnp_ransac_pass_dlt(dev):
    return _pose_pass_case(dev, "dlt")


@case(["sfm_pnp_ransac_pass"], ["p3p_ransac_pass_"])
def pnp_ransac_pass_p3p(dev):
    return _pose_pass_case(dev, "p3p")


def _pose_sample_fit_case(dev, entry):
    import torch

    i = Inst(dev)
    B, n, h = 2, 700, 257
    pts = i.inp(_pnp_pts(n, 3, B), _pnp_pts(n, 4, B))
    S, model = i.out("S", (B, h, 8), torch.int32), i.out("model", (B, h, 12), torch.float64)
    flags = i.out("flags", (B, h), torch.int32)
    i.constant.add("flags")
    i.host = {"A": 9, "B": 10}
    fn = getattr(_lib(), entry)
    Kc, Kp = _host_K()
    i.keep = Kc
    i.call = lambda: _check(fn(i.cur, 3, 100, pts.data_ptr(), n, h, B, Kp, S.data_ptr(), model.data_ptr(), flags.data_ptr(),
                               _st()), entry)
    return i


@case(["sfm_pnp_sample_fit_philox"])
def pnp_sample_fit_philox(dev):
    return _pose_sample_fit_case(dev, "sfm_pnp_sample_fit_philox")


@case(["sfm_p3p_sample_fit_philox"])
def p3p_sample_fit_philox(dev):
    return _pose_sample_fit_case(dev, "sfm_p3p_sample_fit_philox")


@case(["sfm_pnp_fit", "sfm_p3p_fit", "sfm_pnp_score", "sfm_pnp_inlier_mask"], ["pnp_fit_", "p3p_fit_", "pnp_score_"])
def pnp_stages(dev):
    """The separate stages of a PnP pass, each a single launch, chained on one stream: both fits, the scoring of the DLT
    models, the selection and the mask."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    pts = i.inp(_pnp_pts(n, 3, B), _pnp_pts(n, 4, B))
    S = i.inp(_table(dev, 7, h, n, B), _table(dev, 8, h, n, B))
    model, flags = i.out("model", (B, h, 12), torch.float64), i.out("flags", (B, h), torch.int32)
    model3, flags3 = i.out("model_p3p", (B, h, 12), torch.float64), i.out("flags_p3p", (B, h), torch.int32)
    cnt, s1, s2 = i.out("cnt", (B, h), torch.int32), i.out("s1", (B, h), torch.float64), i.out("s2", (B, h), torch.float64)
    result, mask = i.out("result", (B, 5), torch.int64), i.out("mask", (B, n), torch.uint8)
    i.constant |= {"flags", "flags_p3p"}

    def call():
        device.pnp_fit(pts, S, _K(), model, flags)
        device.p3p_fit(pts, S, _K(), model3, flags3)
        device.pnp_score(pts, model, S, _K(), PNP_THR, cnt, s1, s2)
        device.select_best(cnt, s1, s2, flags, MIN_EXTRA, AGG_RMS, 0, out=result, sample_size=6)
        device.pnp_inlier_mask(pts, model, S, _K(), result, PNP_THR, out=mask)
    i.call = call
    return i


@case(["sfm_pnp_refine"], ["pnp_refine"])
def pnp_refine(dev):
    """rounds = 3 through the C ABI on the test's buffers, and through the functional op (outputs only)."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257

    def finished(seed):
        pts = torch.as_tensor(_pnp_pts(n, seed, B)).to(dev)
        ws = device.PnPWorkspace(B, n, h, dev)
        ws.run(pts, _K(), PNP_THR, MIN_EXTRA, AGG_RMS, philox=(9, 100, 3))
        torch.cuda.synchronize()
        return (pts,) + _winner(ws) + (ws.mask,)
    a, b = finished(3), finished(4)
    pts, model, err, mask = (i.inp(x, y) for x, y in zip(a, b))
    model_out, mask_out = i.out("model_out", (B, 12), torch.float64), i.out("mask_out", (B, n), torch.uint8)
    info = i.out("info", (B, 3), torch.int64)
    lib = _lib()
    Kc, Kp = _host_K()
    i.keep = Kc

    def call():
        _check(lib.sfm_pnp_refine(pts.data_ptr(), n, B, Kp, model.data_ptr(), mask.data_ptr(), err.data_ptr(), PNP_THR, AGG_RMS,
                                  3, 20, model_out.data_ptr(), mask_out.data_ptr(), info.data_ptr(), _st()), "sfm_pnp_refine")
        return Returned(device.pnp_refine(pts, model, mask, err, _K(), PNP_THR, AGG_RMS, rounds=3, max_steps=20))
    i.call = call
    return i


def _h_corr(n, seed, batch=1, motion="bench"):
    import homography_oracle as ho

    return np.stack([np.ascontiguousarray(ho.motion_scene(motion, n, seed + 100 * b, 0.5, 0.3)["corr"]).reshape(n, 4)
                     for b in range(batch)])


@case(["sfm_five_point_ransac_pass"], ["five_point_ransac_pass_"])
def five_point_ransac_pass(dev):
    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    corr = i.inp(_h_corr(n, 40, B), _h_corr(n, 41, B))
    outs = _pass_outputs(i, B, n, h)
    i.call = lambda: device.five_point_ransac_pass(corr, *outs, H_THR, MIN_EXTRA, AGG_RMS, philox=(i.cur, 100, 3))
    return i


@case(["sfm_five_point_sample_fit_philox", "sfm_five_point_fit", "sfm_five_point_candidates", "sfm_score_sed_sample_ex"],
      ["five_point_fit_"])
def five_point_stages(dev):
    """Philox-sampled fit, the fit from that table, every candidate, six-item scoring, the selection and the six-item mask."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    corr = i.inp(_h_corr(n, 40, B), _h_corr(n, 41, B))
    S, E, flags = i.out("S", (B, h, 8), torch.int32), i.out("E", (B, h, 9), torch.float64), i.out("flags", (B, h), torch.int32)
    E2, flags2 = i.out("E_table", (B, h, 9), torch.float64), i.out("flags_table", (B, h), torch.int32)
    cand, count = i.out("candidates", (B, h, 10, 9), torch.float64), i.out("count", (B, h), torch.int32)
    cnt, s1, s2 = i.out("cnt", (B, h), torch.int32), i.out("s1", (B, h), torch.float64), i.out("s2", (B, h), torch.float64)
    result, mask = i.out("result", (B, 5), torch.int64), i.out("mask", (B, n), torch.uint8)
    i.constant |= {"flags", "flags_table"}
    i.host = {"A": 9, "B": 10}
    lib = _lib()

    def call():
        device.five_point_fit(corr, S, E, flags, philox=(i.cur, 100, 3))
        device.five_point_fit(corr, S, E2, flags2)
        _check(lib.sfm_five_point_candidates(corr.data_ptr(), n, S.data_ptr(), h, B, cand.data_ptr(), count.data_ptr(), _st()),
               "sfm_five_point_candidates")
        device.score_sed(corr, E, S, H_THR, cnt, s1, s2, sample_size=6)
        device.select_best(cnt, s1, s2, flags, MIN_EXTRA, AGG_RMS, 0, out=result, sample_size=6)
        device.inlier_mask(corr, E, S, result, H_THR, out=mask, sample_size=6)
    i.call = call
    return i


@case(["sfm_homography_ransac_pass"], ["homography_ransac_pass_"])
def homography_ransac_pass(dev):
    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    corr = i.inp(_h_corr(n, 40, B, "plane_bench"), _h_corr(n, 41, B, "plane_bench"))
    ws = device.HomographyWorkspace(B, n, h, dev)
    ws.S, ws.model, ws.flags, ws.cnt, ws.s1, ws.s2, ws.result, ws.mask = _pass_outputs(i, B, n, h)
    ws.H = ws.model
    i.call = lambda: ws.run(corr, H_THR, MIN_EXTRA, AGG_RMS, philox=(i.cur, 100, 3))
    return i


@case(["sfm_homography_fit", "sfm_homography_score", "sfm_homography_inlier_mask"],
      ["homography_fit", "homography_score", "homography_inlier_mask"])
def homography_stages(dev):
    """The three functional ops chained on one stream, with the selection between them (outputs only)."""
    from structure_from_motion_amd import device

    i = Inst(dev)
    B, n, h = 2, 700, 257
    corr = i.inp(_h_corr(n, 40, B, "plane_bench"), _h_corr(n, 41, B, "plane_bench"))
    S = i.inp(_table(dev, 7, h, n, B), _table(dev, 8, h, n, B))

    def call():
        H, flags = device.homography_fit(corr, S)
        cnt, s1, s2 = device.homography_score(corr, H, S, H_THR)
        result = device.select_best(cnt, s1, s2, flags, MIN_EXTRA, AGG_RMS, sample_size=4)
        mask = device.homography_inlier_mask(corr, H, S, result, H_THR)
        return Returned((H, cnt, s1, s2, result, mask))
    i.call = call
    return i


# ------------------------------------------------------------------------------------------------------
# graph stage
# ------------------------------------------------------------------------------------------------------
@case(["sfm_verify_pairs", "sfm_pair_poses"], ["verify_pairs_", "pair_poses"])
def view_graph(dev):
    """``ViewGraphWorkspace.run`` on the twelve-pair ragged fixture, then the poses: through the C ABI on the test's pose table
    and workspace, and through ``.poses`` (the functional op; outputs only)."""
    import torch

    import view_graph_oracle as vo
    from structure_from_motion_amd import device

    i = Inst(dev)
    a, b = vo.ragged_arrays(vo.ragged_scenes(seed=40)), vo.ragged_arrays(vo.ragged_scenes(seed=140))
    assert np.array_equal(a[1], b[1])
    Q, N, h = len(vo.SIZES), len(a[0]), 256
    corr = i.inp(a[0], b[0])
    offset, min_extra = i.same(a[1], torch.int64), i.same(a[2])
    ws = device.ViewGraphWorkspace(Q, N, h, dev)
    names = ("S", "H", "E", "h_flags", "h_cnt", "h_s1", "h_s2", "e_flags", "e_cnt", "e_s1", "e_s2", "h_result", "e_result",
             "h_mask", "e_mask", "verdict")
    for name, buf in zip(names, ws.buffers()):
        setattr(ws, name, i.out(name, tuple(buf.shape), buf.dtype))
    pose = i.out("pose", (Q, device.POSE_BYTES), torch.uint8)
    i.host = {"A": 0x9E3779B97F4A7C15, "B": 0x9E3779B97F4A7C16}
    i.constant |= {"h_flags", "e_flags"}   # the fillers of the pairs below a sample size, no degenerate sample elsewhere
    lib = _lib()
    pose_ws = i.work(lib.sfm_pair_poses_workspace_bytes(N, Q))

    def call():
        ws.run(corr, offset, min_extra, vo.THR, vo.RMS, 0.8, i.cur)
        _check(lib.sfm_pair_poses(corr.data_ptr(), N, offset.data_ptr(), Q, ws.E.data_ptr(), h, ws.e_result.data_ptr(),
                                  ws.e_mask.data_ptr(), ws.verdict.data_ptr(), 50.0, pose.data_ptr(), pose_ws.data_ptr(),
                                  pose_ws.numel(), _st()), "sfm_pair_poses")
        ws.poses(50.0)
        return Returned((ws.pose, ws.angle))
    i.call = call
    return i


def _track_graph(seed, images, features):
    from structure_from_motion_amd import synthetic

    g = synthetic.match_graph(images, features, 3, features // 3, wrong_fraction=0.05, seed=seed)
    return g["image_offset"], g["pairs"], g["match_offset"], g["match_index"]


@case(["sfm_build_tracks"], ["build_tracks_"])
def build_tracks(dev):
    """66 000 features (three radix passes) through the C ABI on the test's workspace; the in-place op on the same inputs."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    images, per = 33, 2000
    a, b = _track_graph(0, images, per), _track_graph(1, images, per)
    F, Q, M = images * per, len(a[1]), len(a[3])
    assert F >= 65537 and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    image_offset, match_offset = i.same(a[0], torch.int32), i.same(a[2], torch.int32)
    pair_images, match_index = i.inp(a[1], b[1], torch.int32), i.inp(a[3], b[3], torch.int32)

    def outputs(tag):
        outs = [i.out(k + tag, (F,), torch.uint8 if k == "status" else torch.int32)
                for k in ("component", "track", "status", "camera_index", "point_index", "feature_index")]
        return outs + [i.out("info" + tag, (6,), torch.int64)]
    own, op = outputs(""), outputs("_op")
    lib = _lib()
    ws = i.work(lib.sfm_build_tracks_workspace_bytes(images, F, M))

    def call():
        _check(lib.sfm_build_tracks(images, F, Q, M, image_offset.data_ptr(), pair_images.data_ptr(), match_offset.data_ptr(),
                                    match_index.data_ptr(), *[t.data_ptr() for t in own], ws.data_ptr(), ws.numel(), _st()),
               "sfm_build_tracks")
        device.build_tracks(image_offset, pair_images, match_offset, match_index, F, out=tuple(op))
    i.call = call
    return i


def _tracks_scene(seed):
    from structure_from_motion_amd import synthetic

    sc = synthetic.multi_view_scene(views=8, points=2000, seed=seed)
    return sc["poses_true"], sc["camera_indices"], sc["point_indices"], sc["pixels"]


def _triangulate_tracks_case(dev, refine):
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    a, b = _tracks_scene(21), _tracks_scene(22)
    # the observation count depends on the seed: both scenes cut to the shorter list (a track may lose views: a valid scene)
    M = min(len(a[1]), len(b[1]))
    a, b = (a[0], a[1][:M], a[2][:M], a[3][:M]), (b[0], b[1][:M], b[2][:M], b[3][:M])
    P, Cn = 2000, 8
    poses = i.same(a[0])
    cam, pt, pix = i.inp(a[1], b[1], torch.int32), i.inp(a[2], b[2], torch.int32), i.inp(a[3], b[3])

    def outputs(tag):
        return [i.out("points" + tag, (P, 3), torch.float64), i.out("status" + tag, (P,), torch.uint8),
                i.out("obs_error" + tag, (M,), torch.float64), i.out("angle" + tag, (P,), torch.float64),
                i.out("info" + tag, (4,), torch.int64)]
    own, op = outputs(""), outputs("_op")
    lib = _lib()
    ws = i.work(lib.sfm_tracks_workspace_bytes(P, M))
    Kc, Kp = _host_K()
    i.keep = Kc
    min_angle, max_error = float(np.radians(1.0)), 16.0

    def call():
        _check(lib.sfm_triangulate_tracks(Kp, Cn, P, M, poses.data_ptr(), cam.data_ptr(), pt.data_ptr(), pix.data_ptr(), 2,
                                          min_angle, max_error, refine, *[t.data_ptr() for t in own], ws.data_ptr(), ws.numel(),
                                          _st()), "sfm_triangulate_tracks")
        device.triangulate_tracks(poses, cam, pt, pix, P, _K(), 2, min_angle, max_error, refine, out=tuple(op))
    i.call = call
    return i


@case(["sfm_triangulate_tracks"], ["triangulate_tracks_"])
def triangulate_tracks(dev):
    return _triangulate_tracks_case(dev, 0)


@case(["sfm_triangulate_tracks"], ["triangulate_tracks_"])
def triangulate_tracks_refined(dev):
    return _triangulate_tracks_case(dev, 10)


def _bundle_case(dev, cameras, points, pcg, max_steps):
    """Both entry points of one adjuster (plain, and ``_ex`` with the Huber loss) through the C ABI on the test's workspace,
    and the two in-place ops."""
    import torch

    from structure_from_motion_amd import _native, device, synthetic

    i = Inst(dev)
    a = synthetic.corrupt_observations(synthetic.bundle_problem(cameras, points, seed=0), 0.05, 20.0, 5)[0]
    b = synthetic.corrupt_observations(synthetic.bundle_problem(cameras, points, seed=1), 0.05, 20.0, 6)[0]
    M = len(a["pixels"])
    assert M == len(b["pixels"])
    keys = ("poses", "points", "camera_indices", "point_indices", "pixels")
    poses, pts, cam, pt, pix = (i.inp(a[k], b[k]) for k in keys)
    words = 5 if pcg else 4

    def outputs(tag):
        return [i.out("poses" + tag, (cameras, 12), torch.float64), i.out("points" + tag, (points, 3), torch.float64),
                i.out("info" + tag, (words,), torch.int64)]
    plain, robust, op, op_robust = outputs(""), outputs("_huber"), outputs("_op"), outputs("_op_huber")
    lib = _lib()
    options = _native.BundleOptions(1, 0, 2.0)
    if pcg:
        ws = i.work(lib.sfm_bundle_pcg_workspace_bytes(cameras, points, M))
        ws_robust = i.work(lib.sfm_bundle_pcg_workspace_bytes_ex(cameras, points, M, C.byref(options)))
    else:
        ws = i.work(lib.sfm_bundle_workspace_bytes(cameras, points, M))
        ws_robust = i.work(lib.sfm_bundle_workspace_bytes(cameras, points, M))
    Kc, Kp = _host_K()
    fixed = (C.c_uint8 * cameras)(1, *([0] * (cameras - 1)))
    i.keep = (Kc, fixed, options)
    head = (Kp, cameras, points, M, C.cast(fixed, C.c_void_p), poses.data_ptr(), pts.data_ptr(), cam.data_ptr(), pt.data_ptr(),
            pix.data_ptr(), max_steps) + ((20, 0.1) if pcg else ())
    name = "sfm_bundle_adjust_pcg" if pcg else "sfm_bundle_adjust"
    run = device.bundle_adjust_pcg if pcg else device.bundle_adjust
    extra = dict(max_cg_iterations=20, cg_tolerance=0.1) if pcg else {}

    def call():
        _check(getattr(lib, name)(*head, *[t.data_ptr() for t in plain], ws.data_ptr(), ws.numel(), _st()), name)
        _check(getattr(lib, name + "_ex")(*head, *[t.data_ptr() for t in robust], ws_robust.data_ptr(), ws_robust.numel(), _st(),
                                         C.byref(options)), name + "_ex")
        for out, kw in ((op, {}), (op_robust, dict(loss="huber", loss_scale=2.0))):
            out[0].copy_(poses), out[1].copy_(pts)
            run(out[0], out[1], cam, pt, pix, _K(), (0,), max_steps, out=tuple(out), **extra, **kw)
    i.call = call
    return i


@case(["sfm_bundle_adjust", "sfm_bundle_adjust_ex"], ["bundle_adjust_", "bundle_adjust_robust_"])
def bundle_adjust(dev):
    """C = 8, three steps: the four calls of the case enqueue a few hundred launches in all."""
    return _bundle_case(dev, 8, 200, False, 3)


@case(["sfm_bundle_adjust_pcg", "sfm_bundle_adjust_pcg_ex"], ["bundle_adjust_pcg_", "bundle_adjust_pcg_robust_"])
def bundle_adjust_pcg(dev):
    """C = 65, two steps.  Documented as synchronising: the before-check only."""
    return _bundle_case(dev, 65, 600, True, 2)


@case(["sfm_average_rotations"], ["average_rotations"])
def average_rotations(dev):
    """The ``case_losses`` graph (Huber, five steps) through the C ABI on the test's workspace and through the functional op.
    Documented as synchronising: the before-check only."""
    import torch

    import rotation_averaging_oracle as ro
    from structure_from_motion_amd import _native, device

    i = Inst(dev)
    a, b = ro.case_losses(1), ro.case_losses(2)
    Cn, Q = a["C"], len(a["pairs"])
    pairs = i.inp(a["pairs"], b["pairs"], torch.int32)
    rel, w = i.inp(a["relative"].reshape(Q, 9), b["relative"].reshape(Q, 9)), i.same(a["weights"])
    R, reg = i.out("rotations", (Cn, 9), torch.float64), i.out("registered", (Cn,), torch.uint8)
    level, res = i.out("level", (Cn,), torch.int32), i.out("residual", (Q,), torch.float64)
    info = i.out("info", (5,), torch.int64)
    i.constant |= {"registered", "returned1"}   # both graphs hold a ring: every camera registers (returned1: the op's copy)
    lib = _lib()
    ws = i.work(lib.sfm_average_rotations_workspace_bytes(Cn, Q))
    scale = float(np.radians(1.0))
    opts = _native.RotavgOptions(1, 0, 5, 50, scale, 1e-10, 1e-300)
    i.keep = opts

    def call():
        _check(lib.sfm_average_rotations(Cn, Q, pairs.data_ptr(), rel.data_ptr(), w.data_ptr(), 0, None, C.byref(opts),
                                         R.data_ptr(), reg.data_ptr(), level.data_ptr(), res.data_ptr(), info.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _st()), "sfm_average_rotations")
        return Returned(device.average_rotations(pairs, rel.view(Q, 3, 3), w, Cn, 0, None, "huber", scale, max_steps=5,
                                                 max_cg_iterations=50, cg_tolerance=1e-10, step_tolerance=1e-300))
    i.call = call
    return i


@case(["sfm_average_translations"], ["average_translations"])
def average_translations(dev):
    """As ``average_rotations``, on the translation ``case_losses`` graph."""
    import torch

    import translation_averaging_oracle as to
    from structure_from_motion_amd import _native, device

    i = Inst(dev)
    a, b = to.case_losses(1), to.case_losses(2)
    Cn, Q = a["C"], len(a["pairs"])
    pairs = i.inp(a["pairs"], b["pairs"], torch.int32)
    v, w = i.inp(a["directions"], b["directions"]), i.same(a["weights"])
    pos, reg = i.out("positions", (Cn, 3), torch.float64), i.out("registered", (Cn,), torch.uint8)
    level, res = i.out("level", (Cn,), torch.int32), i.out("residual", (Q,), torch.float64)
    scale_out, info = i.out("scale", (Q,), torch.float64), i.out("info", (5,), torch.int64)
    i.constant |= {"registered", "returned1"}
    lib = _lib()
    ws = i.work(lib.sfm_average_translations_workspace_bytes(Cn, Q))
    opts = _native.TransavgOptions(1, 0, 6, 50, 2, 0, to.HUBER_SCALE, 1e-12, 1e-300)
    i.keep = opts

    def call():
        _check(lib.sfm_average_translations(Cn, Q, pairs.data_ptr(), v.data_ptr(), None, w.data_ptr(), 0, None, C.byref(opts),
                                            pos.data_ptr(), reg.data_ptr(), level.data_ptr(), res.data_ptr(),
                                            scale_out.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), _st()),
               "sfm_average_translations")
        return Returned(device.average_translations(pairs, v, w, Cn, 0, None, None, "huber", to.HUBER_SCALE, warmup_steps=2,
                                                    max_steps=6, max_cg_iterations=50, cg_tolerance=1e-12, step_tolerance=1e-300))
    i.call = call
    return i


# ------------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------------
N_A, N_B, STRIDE, WINDOW = 131, 203, 256, 9   # 131 x 203 in the padded layout: rows of two whole 128-feature tiles


def _texture(seed):
    """(image_a, image_b uint8, features of a [N_A, 2], features of b [N_B, 2]) of one rotated texture pair; some features
    hang over the border (ok = 0)."""
    from structure_from_motion_amd import synthetic

    img_a, img_b, pairs = synthetic.rotated_texture_pair(120, 160, 10.0, N_B, seed)
    fa, fb = pairs[:N_A, :2].copy(), pairs[:, 2:].copy()
    fa[3], fb[5] = (1.0, 2.0), (158.0, 118.0)
    return img_a, img_b, fa, fb


def _match_case(dev, ncc, fused):
    """Both patch extractions and either the fused summary or the score matrix and its row summary."""
    import torch

    from structure_from_motion_amd import _native

    i = Inst(dev)
    a, b = _texture(3), _texture(4)
    pixel = np.float64 if ncc else np.int64   # (integer SSD reads the pixels as int64 bit patterns)
    img_a, img_b = i.inp(a[0].astype(pixel), b[0].astype(pixel)), i.inp(a[1].astype(pixel), b[1].astype(pixel))
    fa, fb = i.inp(a[2], b[2]), i.inp(a[3], b[3])
    K = WINDOW * WINDOW
    metric = _native.MATCH_NCC if ncc else _native.match_ssd_int(8, False)
    mode = _native.PATCH_MEAN_REMOVED if ncc else _native.PATCH_RAW64
    pa, pb = i.out("patches_a", (K, STRIDE), torch.float64), i.out("patches_b", (K, STRIDE), torch.float64)
    qa, qb = i.out("ssq_a", (N_A,), torch.float64), i.out("ssq_b", (N_B,), torch.float64)
    oka, okb = i.out("ok_a", (N_A,), torch.uint8), i.out("ok_b", (N_B,), torch.uint8)
    best, arg = i.out("best", (N_A,), torch.float64), i.out("arg", (N_A,), torch.int32)
    second = i.out("second", (N_A,), torch.float64)
    i.constant |= {"ok_a", "ok_b"} | (set() if ncc else {"ssq_a", "ssq_b"})   # (RAW64 patches: ssq is 0)
    lib = _lib()
    if fused:
        ws = i.work(lib.sfm_match_summary_workspace_bytes(N_A, N_B))
    else:
        scores = i.out("scores", (N_A, N_B), torch.float64)
    H, W = a[0].shape

    def call():
        for img, ft, n, p, q, ok in ((img_a, fa, N_A, pa, qa, oka), (img_b, fb, N_B, pb, qb, okb)):
            _check(lib.sfm_patch_extract(img.data_ptr(), H, W, ft.data_ptr(), n, WINDOW, mode, STRIDE, p.data_ptr(), q.data_ptr(),
                                         ok.data_ptr(), _st()), "sfm_patch_extract")
        if fused:
            _check(lib.sfm_match_summary(metric, pa.data_ptr(), STRIDE, pb.data_ptr(), STRIDE, qa.data_ptr(), qb.data_ptr(),
                                         oka.data_ptr(), okb.data_ptr(), N_A, N_B, K, ws.data_ptr(), ws.numel(), best.data_ptr(),
                                         arg.data_ptr(), second.data_ptr(), _st()), "sfm_match_summary")
        else:
            _check(lib.sfm_pair_scores(metric, pa.data_ptr(), STRIDE, pb.data_ptr(), STRIDE, qa.data_ptr(), qb.data_ptr(),
                                       oka.data_ptr(), okb.data_ptr(), N_A, N_B, K, scores.data_ptr(), _st()), "sfm_pair_scores")
            _check(lib.sfm_match_row_summary(scores.data_ptr(), N_A, N_B, best.data_ptr(), arg.data_ptr(), second.data_ptr(),
                                             _st()), "sfm_match_row_summary")
    i.call = call
    return i


@case(["sfm_patch_extract", "sfm_match_summary"])
def match_summary_ncc(dev):
    return _match_case(dev, True, True)


@case(["sfm_patch_extract", "sfm_match_summary"])
def match_summary_ssd_uint8(dev):
    return _match_case(dev, False, True)


@case(["sfm_patch_extract", "sfm_pair_scores", "sfm_match_row_summary"])
def pair_scores_row_summary(dev):
    return _match_case(dev, True, False)


def _pattern(dev):
    from structure_from_motion_amd.feature_matching import brief

    return brief._pattern_on(dev)


@case(["sfm_brief_describe"])
def brief_describe(dev):
    import torch

    i = Inst(dev)
    n = 130
    a, b = _texture(3), _texture(4)
    img, ft = i.inp(a[0], b[0]), i.inp(a[2][:n], b[2][:n])
    offsets, boundaries = _pattern(dev)
    desc, ok, bins = i.out("desc", (n, 32), torch.uint8), i.out("ok", (n,), torch.uint8), i.out("angle_bin", (n,), torch.uint8)
    i.constant.add("ok")
    lib = _lib()
    H, W = a[0].shape
    i.call = lambda: _check(lib.sfm_brief_describe(img.data_ptr(), H, W, ft.data_ptr(), n, offsets.data_ptr(),
                                                   boundaries.data_ptr(), 30, desc.data_ptr(), ok.data_ptr(), bins.data_ptr(),
                                                   _st()), "sfm_brief_describe")
    return i


def _descriptors(seed, n):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), (rng.random(n) < 0.9).astype(np.uint8)


@case(["sfm_hamming_summary"])
def hamming_summary(dev):
    import torch

    i = Inst(dev)
    nA, nB = 130, 700
    (da, va), (db, vb) = _descriptors(1, nA), _descriptors(2, nA)
    (ea, wa), (eb, wb) = _descriptors(3, nB), _descriptors(4, nB)
    desc_a, ok_a, desc_b, ok_b = i.inp(da, db), i.inp(va, vb), i.inp(ea, eb), i.inp(wa, wb)
    best, arg = i.out("best", (nA,), torch.float64), i.out("arg", (nA,), torch.int32)
    second = i.out("second", (nA,), torch.float64)
    lib = _lib()
    ws = i.work(lib.sfm_hamming_summary_workspace_bytes(nA, nB))
    i.call = lambda: _check(lib.sfm_hamming_summary(desc_a.data_ptr(), ok_a.data_ptr(), nA, desc_b.data_ptr(), ok_b.data_ptr(),
                                                    nB, ws.data_ptr(), ws.numel(), best.data_ptr(), arg.data_ptr(),
                                                    second.data_ptr(), _st()), "sfm_hamming_summary")
    return i


@case(["sfm_match_pairs"])
def match_pairs(dev):
    """Six ordered pairs over images of 255 / 513 / 1030 descriptors, cross-check on."""
    import torch

    from structure_from_motion_amd import device

    i = Inst(dev)
    sizes = np.array([255, 513, 1030], dtype=np.int64)
    pairs = np.array([(x, y) for x in range(3) for y in range(3) if x != y], dtype=np.int32)

    def collection(seed):
        rng = np.random.default_rng(seed)
        pool = rng.integers(0, 256, (400, 32), dtype=np.uint8)
        bits = []
        for n in sizes:   # pool descriptors with up to 40 flipped bits: real matches (tests/test_gpu_graph_matching.py, "noisy")
            flips = np.zeros((n, 256), dtype=np.uint8)
            for row, count in zip(flips, rng.integers(0, 41, n)):
                row[rng.choice(256, count, replace=False)] = 1
            bits.append(pool[rng.integers(0, len(pool), n)] ^ np.packbits(flips, axis=1, bitorder="little"))
        return np.concatenate(bits), (rng.random(int(sizes.sum())) < 0.9).astype(np.uint8)
    a, b = collection(40), collection(41)
    desc, ok = i.inp(a[0], b[0]), i.inp(a[1], b[1])
    offset = np.zeros(4, dtype=np.int32)
    offset[1:] = np.cumsum(sizes)
    row_offset = np.zeros(len(pairs) + 1, dtype=np.int64)
    row_offset[1:] = np.cumsum(sizes[pairs[:, 0]])
    rows, F = int(row_offset[-1]), int(sizes.sum())
    image_offset, pair_images, rows_dev = i.same(offset), i.same(pairs), i.same(row_offset)
    partner, distance = i.out("partner", (rows,), torch.int32), i.out("distance", (rows,), torch.int32)
    status = i.out("pair_status", (len(pairs),), torch.int32)
    i.constant.add("pair_status")
    ws = i.work(_lib().sfm_match_pairs_workspace_bytes(len(pairs), rows, 1030))
    i.call = lambda: device.match_pairs(3, F, image_offset, desc, ok, pair_images, rows_dev, rows, 1030, 64, 0.8, True, partner,
                                        distance, status, workspace=ws)
    return i


@case(["sfm_detect_keypoints"])
def detect_keypoints(dev):
    """Four images of ``test_gpu_keypoints.COLLECTION``'s shapes — the three with three or more levels, 97 x 131, 200 x 263 and
    100 x 110, and 129 x 64 with two — at a capacity that holds every candidate.  The candidates and their rows come in no
    particular slot order: compared sorted by (plane, y, x)."""
    import torch

    import test_gpu_keypoints as tk
    from structure_from_motion_amd import device
    from structure_from_motion_amd.feature_matching import keypoints as kp

    i = Inst(dev)
    shapes = ((97, 131, "tiled"), (200, 263, "texture"), (100, 110, "noise"), (129, 64, "texture"))
    layout = kp.plan([s[:2] for s in shapes], 100000, 8)
    assert sum(1 for s in shapes if len(kp.level_shapes(s[0], s[1], 8)) >= 3) == 3
    capacity = sum(kp._survivor_bound(h, w) for _, _, h, w, _, _ in layout.rows)

    def pool_of(seed):
        host = np.zeros(layout.pool_bytes, dtype=np.uint8)
        flat = np.concatenate([tk._image(h, w, content, seed + k).reshape(-1) for k, (h, w, content) in enumerate(shapes)])
        host[:flat.size] = flat
        return host
    pool = i.inp(pool_of(100), pool_of(200))
    i.watch.append(("pool", pool))   # the call fills the planes above level 0 in place
    offsets, boundaries = _pattern(dev)
    score, kept = i.out("score", (layout.pool_bytes,), torch.int16), i.out("kept", (layout.pool_bytes,), torch.int16)
    counter = i.out("counter", (4,), torch.int32)
    cand = i.out("candidates", (capacity, 4), torch.int32)
    desc, ok = i.out("desc", (capacity, 32), torch.uint8), i.out("ok", (capacity,), torch.uint8)
    bins = i.out("angle_bin", (capacity,), torch.uint8)
    i.constant.add("ok")
    table = device.keypoint_plane_table(layout.rows)
    ws = i.work(_lib().sfm_detect_keypoints_workspace_bytes(len(layout.rows)))

    def canon(host):
        found = int(host["counter"][0])
        assert 0 < found <= capacity
        c = host["candidates"][:found]
        order = np.lexsort((c[:, 1], c[:, 2], c[:, 0]))
        out = dict(host)
        for name in ("candidates", "desc", "ok", "angle_bin"):
            out[name] = np.ascontiguousarray(host[name][:found][order])
        return out
    i.canon = canon
    i.call = lambda: device.detect_keypoints(table, len(layout.rows), len(shapes), pool, 20, offsets, boundaries, 30, score, kept,
                                             capacity, counter[:1], cand, desc, ok, bins, workspace=ws)
    return i


def _cornerness(seed, shape=(97, 131)):
    """A suppressed-cornerness-like image: sparse positive values on zeros, with ties."""
    rng = np.random.default_rng(seed)
    image = np.floor(rng.random(shape) * 50.0)
    image[rng.random(shape) < 0.6] = 0.0
    return image


@case(["sfm_cross_correlate", "sfm_harris_cornerness"])
def harris_cornerness(dev):
    import torch

    from structure_from_motion_amd import synthetic

    i = Inst(dev)
    a = synthetic.rotated_texture_pair(97, 131, 5.0, 4, 3)[0].astype(np.float64)
    b = synthetic.rotated_texture_pair(97, 131, 5.0, 4, 4)[0].astype(np.float64)
    h, w = a.shape
    image = i.inp(a, b)
    sobel = np.array([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]])
    kx, ky = i.same(sobel), i.same(np.ascontiguousarray(sobel.T))
    sx, sy = i.out("sobel_x", (h, w), torch.float64), i.out("sobel_y", (h, w), torch.float64)
    out = i.out("cornerness", (h - 1, w - 1), torch.float64)
    lib = _lib()

    def call():
        _check(lib.sfm_cross_correlate(image.data_ptr(), h, w, kx.data_ptr(), 3, sx.data_ptr(), _st()), "sfm_cross_correlate")
        _check(lib.sfm_cross_correlate(image.data_ptr(), h, w, ky.data_ptr(), 3, sy.data_ptr(), _st()), "sfm_cross_correlate")
        _check(lib.sfm_harris_cornerness(sx.data_ptr(), sy.data_ptr(), h, w, 2, 0.04, 1, h - 1, w - 1, out.data_ptr(), _st()),
               "sfm_harris_cornerness")
    i.call = call
    return i


@case(["sfm_nms_round", "sfm_nms_finalize"])
def nms_rounds(dev):
    """Twelve rounds on a zeroed state (the detector's batch), then the finalisation.  The image is input and output: a copy
    on the stream first, as the detector's caller hands over a fresh cornerness image."""
    import torch

    i = Inst(dev)
    a, b = _cornerness(1), _cornerness(2)
    h, w = a.shape
    source = i.inp(a, b)
    image = i.out("image", (h, w), torch.float64)
    state, left = i.out("state", (h, w), torch.uint8), i.out("unresolved", (12,), torch.int32)
    lib = _lib()

    def call():
        image.copy_(source)
        state.zero_(), left.zero_()
        for k in range(12):
            _check(lib.sfm_nms_round(image.data_ptr(), state.data_ptr(), h, w, left[k:].data_ptr(), _st()), "sfm_nms_round")
        _check(lib.sfm_nms_finalize(image.data_ptr(), state.data_ptr(), h, w, _st()), "sfm_nms_finalize")
    i.call = call
    return i


@case(["sfm_nms_inplace"])
def nms_inplace(dev):
    import torch

    i = Inst(dev)
    a, b = _cornerness(1), _cornerness(2)
    h, w = a.shape
    source = i.inp(a, b)
    image = i.out("image", (h, w), torch.float64)
    lib = _lib()

    def call():
        image.copy_(source)
        _check(lib.sfm_nms_inplace(image.data_ptr(), h, w, _st()), "sfm_nms_inplace")
    i.call = call
    return i


def _by_index(counter_name, capacity):
    """canon of an (index, value) list whose slot order is arbitrary: the first min(counter, capacity) entries by flat index."""
    def canon(host):
        found = min(int(host[counter_name][0]), capacity)
        order = np.argsort(host["index"][:found], kind="stable")
        out = dict(host)
        out["index"] = np.ascontiguousarray(host["index"][:found][order])
        out["value"] = np.ascontiguousarray(host["value"][:found][order])
        return out
    return canon


@case(["sfm_compact_nonzero"])
def compact_nonzero(dev):
    import torch

    i = Inst(dev)
    a, b = _cornerness(1, (200, 263)), _cornerness(2, (200, 263))
    count = a.size
    image = i.inp(a.reshape(-1), b.reshape(-1))
    counter = i.out("counter", (1,), torch.int32)
    index, value = i.out("index", (count,), torch.int32), i.out("value", (count,), torch.float64)
    i.canon = _by_index("counter", count)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_compact_nonzero(image.data_ptr(), count, count, counter.data_ptr(), index.data_ptr(),
                                                    value.data_ptr(), _st()), "sfm_compact_nonzero")
    return i


@case(["sfm_prune_top"])
def prune_top(dev):
    """The candidates of ``sfm_compact_nonzero`` (in index order here), the 300 largest wanted in scene A and the 280 largest in
    scene B, so that the counter differs too."""
    import torch

    i = Inst(dev)
    n, room = 20000, 4096

    def candidates(seed):
        rng = np.random.default_rng(seed)
        return rng.random(n) * 1000.0, rng.permutation(4 * n)[:n].astype(np.int32), np.array([n], dtype=np.int32)
    a, b = candidates(1), candidates(2)
    value, index, found = i.inp(a[0], b[0]), i.inp(a[1], b[1]), i.inp(a[2], b[2])
    i.B[-1][0] = n - 7   # (a count of its own in scene B)
    i.host = {"A": 300, "B": 280}
    counter = i.out("counter", (1,), torch.int32)
    index_out, value_out = i.out("index", (room,), torch.int32), i.out("value", (room,), torch.float64)
    i.canon = _by_index("counter", room)
    ws = i.work(4 * 8192)
    lib = _lib()
    i.call = lambda: _check(lib.sfm_prune_top(value.data_ptr(), index.data_ptr(), found.data_ptr(), n, i.cur, ws.data_ptr(), room,
                                              counter.data_ptr(), index_out.data_ptr(), value_out.data_ptr(), _st()),
                            "sfm_prune_top")
    return i
