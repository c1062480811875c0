"""Device plumbing: torch ROCm tensors for memory and streams; the kernels are reached as PyTorch-ROCm custom ops
(``torch.ops.sfm_hip.*``, csrc/sfm_torch_ops.cpp — the op set of SURVEY.md §8b) and, for the entry points outside
that set, by ctypes calls into the same C ABI (libsfm_hip.so) underneath.

Nothing here computes on the CPU.  Every wrapper only enqueues work on the current torch HIP stream;
host synchronisation happens where a caller reads a result back (``.cpu()`` / ``read_select``).
"""
from __future__ import annotations

import ctypes as C
import os
import random as _pyrandom
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _native, ops
from ._native import ScoreOptions, SelectResult, check  # noqa: F401  (ScoreOptions: re-exported for callers and tests)
from .ransac.ransac import solver_sample_size

F64 = torch.float64
SELECT_BYTES = C.sizeof(SelectResult)
assert SELECT_BYTES == 40


def require_gpu() -> torch.device:
    """The hot path has no CPU fallback: fail loudly without a ROCm device or the HIP library."""
    ops.load()
    if not torch.cuda.is_available():
        raise RuntimeError(
            "structure_from_motion_amd: no ROCm GPU visible; the RANSAC / triangulation hot path "
            "only runs as HIP kernels on MI355X (there is no CPU fallback)."
        )
    return torch.device("cuda", torch.cuda.current_device())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device wrappers need contiguous ROCm tensors"
    return t.data_ptr()


def _as_int64(seed: int) -> int:
    """A 64-bit seed as the signed value torch op schemas carry (same bit pattern)."""
    seed &= 2**64 - 1
    return seed - 2**64 if seed >= 2**63 else seed


def _score_buffers(cnt, s1, s2, B: int, H: int, device):
    """cnt, s1, s2 [B,H]: the caller's buffers, new ones where it gave none."""
    if cnt is None:
        cnt = torch.empty((B, H), dtype=torch.int32, device=device)
    if s1 is None:
        s1 = torch.empty((B, H), dtype=F64, device=device)
    if s2 is None:
        s2 = torch.empty((B, H), dtype=F64, device=device)
    return cnt, s1, s2


def _fit_buffers(model, flags, B: int, H: int, width: int, device):
    """model [B,H,12] or E [B,H,9], and flags [B,H]: the caller's buffers, new ones where it gave none."""
    if model is None:
        model = torch.empty((B, H, width), dtype=F64, device=device)
    if flags is None:
        flags = torch.empty((B, H), dtype=torch.int32, device=device)
    return model, flags


def to_device(array, dtype=F64) -> torch.Tensor:
    dev = require_gpu()
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(dev)


# ------------------------------------------------------------------------------------------------------
# thin wrappers, one per C-ABI entry point
# ------------------------------------------------------------------------------------------------------
def normalize_correspondences(pix_a: torch.Tensor, pix_b: torch.Tensor, K, out=None) -> torch.Tensor:
    """pix_a, pix_b: [..., 2] f64 on device -> corr [..., 4]."""
    op = ops.load()
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    if out is None:
        return op.normalize_coords(pix_a, pix_b, fx, fy, cx, cy)
    op.normalize_coords_(pix_a, pix_b, fx, fy, cx, cy, out)
    return out


def sample_philox(seed: int, h_begin: int, h_count: int, n: int, batch: int = 1, seed_stride: int = 1,
                  out=None, device=None) -> torch.Tensor:
    if out is None:
        return ops.load().sample_philox(_as_int64(seed), seed_stride, h_begin, h_count, n, batch,
                                        device or require_gpu())
    lib = _native.load()  # filling a caller's buffer: straight through the C ABI
    check(lib.sfm_sample_philox(seed & (2**64 - 1), seed_stride, h_begin, h_count, n, batch, _ptr(out),
                                _stream()), "sfm_sample_philox")
    return out


def sample_philox_dev(seed_dev: torch.Tensor, h_begin: int, h_count: int, n: int, batch: int = 1,
                      seed_stride: int = 1, out=None) -> torch.Tensor:
    """Philox sampler whose seed is the int64 word ``seed_dev[0]`` in device memory (graph-replayable)."""
    lib = _native.load()
    if out is None:
        out = torch.empty((batch, h_count, 8), dtype=torch.int32, device=seed_dev.device)
    check(lib.sfm_sample_philox_dev(_ptr(seed_dev), seed_stride, h_begin, h_count, n, batch, _ptr(out),
                                    _stream()), "sfm_sample_philox_dev")
    return out


def sample_philox_at(seed: int, h_index: torch.Tensor, n: int, seed_stride: int = 1, out=None) -> torch.Tensor:
    """h_index: int64 [B] on device -> S [B,1,8]: the sample of hypothesis h_index[b] (no host sync)."""
    lib = _native.load()
    B = h_index.shape[0]
    if out is None:
        out = torch.empty((B, 1, 8), dtype=torch.int32, device=h_index.device)
    check(lib.sfm_sample_philox_at(seed & (2**64 - 1), seed_stride, _ptr(h_index), n, B, _ptr(out),
                                   _stream()), "sfm_sample_philox_at")
    return out


def fit_eight_point(corr: torch.Tensor, S: torch.Tensor, E=None, flags=None, lambda2=None):
    """corr [B,N,4], S [B,H,8] -> E [B,H,9], flags [B,H]."""
    B, N, _ = corr.shape
    H = S.shape[1]
    assert S.shape == (B, H, 8) and S.dtype == torch.int32
    if lambda2 is None and E is None and flags is None:
        return ops.load().fit_eight_point(corr, S)
    E, flags = _fit_buffers(E, flags, B, H, 9, corr.device)
    if lambda2 is None:
        ops.load().fit_eight_point_(corr, S, E, flags)
        return E, flags
    lib = _native.load()  # with the second-smallest eigenvalue written out: a diagnostic outside the op set
    check(lib.sfm_fit_eight_point(_ptr(corr), N, _ptr(S), H, B, _ptr(E), _ptr(flags), _ptr(lambda2),
                                  _stream()), "sfm_fit_eight_point")
    return E, flags


TRACE_FIELDS = {  # name -> (offset, shape) inside one trace record of sfm_fit_eight_point_traced
    "norm_a": (0, (8, 2)), "norm_b": (16, (8, 2)), "T1": (32, (3,)), "T2": (35, (3,)),
    "yty": (38, (9, 9)), "eigenvalues": (119, (9,)), "f_est": (128, (3, 3)), "f_rank2": (137, (3, 3)),
}


def sample_fit_philox(corr: torch.Tensor, seed, h_begin: int, S: torch.Tensor, E: torch.Tensor, flags: torch.Tensor,
                      seed_stride: int = 1) -> None:
    """Philox sampling and the eight-point fit in one launch (fills S, E, flags).  ``seed``: an int, or an int64
    device tensor whose first word is read at kernel run time (graph replay)."""
    on_device = isinstance(seed, torch.Tensor)
    ops.load().sample_fit_philox_(corr, 0 if on_device else _as_int64(seed), seed if on_device else None,
                                  seed_stride, h_begin, S, E, flags)


def fit_eight_point_traced(corr: torch.Tensor, S: torch.Tensor):
    """corr [B,N,4], S [B,H,8] -> E [B,H,9], flags [B,H], dict of intermediate arrays (numpy, [B,H,...])."""
    lib = _native.load()
    B, N, _ = corr.shape
    H = S.shape[1]
    nd = lib.sfm_fit_trace_doubles()
    E = torch.empty((B, H, 9), dtype=F64, device=corr.device)
    flags = torch.empty((B, H), dtype=torch.int32, device=corr.device)
    trace = torch.empty((B, H, nd), dtype=F64, device=corr.device)
    check(lib.sfm_fit_eight_point_traced(_ptr(corr), N, _ptr(S), H, B, _ptr(E), _ptr(flags), _ptr(trace),
                                         _stream()), "sfm_fit_eight_point_traced")
    raw = trace.cpu().numpy()
    fields = {}
    for name, (off, shape) in TRACE_FIELDS.items():
        size = int(np.prod(shape))
        fields[name] = raw[..., off:off + size].reshape((B, H) + shape)
    return E, flags, fields


def fit_stage(stage: int, data: np.ndarray, out_size: int) -> np.ndarray:
    """Run one single-problem stage of the fit (see sfm_fit_stage in include/sfm_hip.h)."""
    lib = _native.load()
    inp = to_device(np.ascontiguousarray(data, dtype=np.float64).reshape(-1))
    out = torch.empty((out_size,), dtype=F64, device=inp.device)
    check(lib.sfm_fit_stage(stage, _ptr(inp), _ptr(out), _stream()), "sfm_fit_stage")
    return out.cpu().numpy()


def hartley_normalize(coords: np.ndarray):
    """(n,2) -> normalised (n,2), forward transform T (3,3) (reference _normalize_coords)."""
    lib = _native.load()
    n = coords.shape[0]
    inp = to_device(np.ascontiguousarray(coords, dtype=np.float64))
    out = torch.empty((2 * n + 3,), dtype=F64, device=inp.device)
    check(lib.sfm_hartley_normalize(_ptr(inp), n, _ptr(out), _stream()), "sfm_hartley_normalize")
    raw = out.cpu().numpy()
    scale, cx, cy = raw[2 * n:]
    T = np.array([[scale, 0.0, -scale * cx], [0.0, scale, -scale * cy], [0.0, 0.0, 1.0]])
    return raw[:2 * n].reshape(n, 2).copy(), T


def score_workspace_bytes(n: int, h_count: int, batch: int, options: Optional[ScoreOptions] = None) -> int:
    """Bytes of scoring workspace a call with ``options`` (default: the process-wide set) needs — sized by what it will launch
    (``sfm_score_workspace_bytes_ex``)."""
    size = int(_native.load().sfm_score_workspace_bytes_ex(n, h_count, batch, None if options is None else C.byref(options)))
    if size < 0:
        raise ValueError("sfm_score_workspace_bytes_ex: negative size or an option out of range")
    return size


def score_workspace(n: int, h_count: int, batch: int, device, options: Optional[ScoreOptions] = None) -> torch.Tensor:
    """Scratch buffer that enables the two-tier scoring kernels (see include/sfm_hip.h), sized for calls made with
    ``options`` (default: the process-wide set)."""
    return torch.empty((score_workspace_bytes(n, h_count, batch, options),), dtype=torch.uint8, device=device)


def score_sed(corr: torch.Tensor, E: torch.Tensor, S: torch.Tensor, thr: float, cnt=None, s1=None,
              s2=None, workspace: Optional[torch.Tensor] = None, exact_only: bool = False,
              options: Optional[ScoreOptions] = None, sample_size: int = 8):
    """Per-hypothesis (extra-inlier count, sum sed, sum sed^2).  Uses the two-tier kernel (fp32 pre-filter
    + exact fp64) unless ``exact_only``; both give identical counts / decisions.  ``options`` (launch options of the
    two-tier kernels: which filter kernel, ranges, order ...; ``sfm_score_sed_ex``) default to the process-wide set, which
    the SFM_SCORE_* variables initialised when the library was loaded.  ``sample_size=6``: the first six entries of a row of
    S are the sample (the five-point fit), scored by the all-fp64 kernel (``sfm_score_sed_sample_ex``)."""
    op = ops.load()
    B, N, _ = corr.shape
    H = E.shape[1]
    if sample_size != 8:
        if workspace is not None or options is not None:
            raise ValueError("score_sed(sample_size != 8) runs the all-fp64 kernel: it takes no workspace and no launch options")
        cnt, s1, s2 = _score_buffers(cnt, s1, s2, B, H, corr.device)
        assert S.dtype == torch.int32 and corr.dtype == F64 and E.dtype == F64
        with torch.cuda.device(corr.device):
            check(_native.load().sfm_score_sed_sample_ex(_ptr(corr), N, _ptr(E), _ptr(S), H, B, float(thr), int(sample_size),
                                                         _ptr(cnt), _ptr(s1), _ptr(s2), _stream()), "sfm_score_sed_sample_ex")
        return cnt, s1, s2
    exact = exact_only or os.environ.get("SFM_SCORE_KERNEL", "filtered") == "exact"
    if options is not None:   # per-call launch options (and timing events): straight through the C ABI
        cnt, s1, s2 = _score_buffers(cnt, s1, s2, B, H, corr.device)
        if exact:
            workspace = None   # NULL selects the all-fp64 kernel
        elif workspace is None:
            workspace = score_workspace(N, H, B, corr.device, options)
        assert S.dtype == torch.int32 and corr.dtype == F64 and E.dtype == F64
        with torch.cuda.device(corr.device):
            check(_native.load().sfm_score_sed_ex(_ptr(corr), N, _ptr(E), _ptr(S), H, B, float(thr), _ptr(cnt), _ptr(s1),
                                                  _ptr(s2), _ptr(workspace), workspace.numel() if workspace is not None else 0,
                                                  _stream(), C.byref(options)), "sfm_score_sed_ex")
        return cnt, s1, s2
    if cnt is None and s1 is None and s2 is None and (exact or workspace is None):
        return op.score_sed(corr, E, S, float(thr), exact)
    cnt, s1, s2 = _score_buffers(cnt, s1, s2, B, H, corr.device)
    if exact:
        workspace = None
    elif workspace is None:
        workspace = score_workspace(N, H, B, corr.device)
    op.score_sed_(corr, E, S, float(thr), cnt, s1, s2, workspace)
    return cnt, s1, s2


def default_score_options() -> ScoreOptions:
    """The process-wide launch options of the scoring kernels (what calls without ``options`` use)."""
    out = ScoreOptions()
    check(_native.load().sfm_score_get_default_options(C.byref(out)), "sfm_score_get_default_options")
    return out


def set_default_score_options(options: Optional[ScoreOptions]) -> None:
    """Replace the process-wide launch options (``None`` = the library's built-in defaults).  The package sets them once
    from the SFM_SCORE_* variables when the library is loaded; bench.py switches kernels with this for its variants."""
    check(_native.load().sfm_score_set_default_options(None if options is None else C.byref(options)),
          "sfm_score_set_default_options")


SMALL_PASS_MAX_POINTS, SMALL_PASS_MAX_HYPOTHESES = 8192, 32768


def small_pass_eligible(batch: int, n: int, h: int) -> bool:
    """Whether a pass can run as the lean small pass (``sfm_ransac_pass_small``): one pair, at most 8192
    correspondences and 32768 hypotheses, the default two-tier scoring kernel.  ``SFM_SMALL_PASS=0`` keeps the
    separate calls (for A/B comparisons)."""
    return (batch == 1 and 8 <= n <= SMALL_PASS_MAX_POINTS and 1 <= h <= SMALL_PASS_MAX_HYPOTHESES
            and os.environ.get("SFM_SMALL_PASS", "1") != "0"
            and os.environ.get("SFM_SCORE_KERNEL", "filtered") != "exact")


def _pass_with_options(entry: str, corr, seed, seed_dev, use_philox, h_begin, thr, min_extra, aggregation, h_offset, S, E, flags,
                       cnt, s1, s2, result, mask, workspace, options: ScoreOptions) -> None:
    """A fused pass with per-call launch options (``sfm_ransac_pass_small`` / ``_large`` through the C ABI: the torch ops carry
    no options argument and run with the process-wide defaults)."""
    assert corr.shape[0] == 1, "one image pair per call"
    n, h = corr.shape[1], S.shape[1]
    with torch.cuda.device(corr.device):
        check(getattr(_native.load(), entry)(seed & (2**64 - 1), _ptr(seed_dev), 1 if use_philox else 0, h_begin, _ptr(corr), n, h,
                                             float(thr), float(min_extra), int(aggregation), h_offset, _ptr(S), _ptr(E),
                                             _ptr(flags), _ptr(cnt), _ptr(s1), _ptr(s2), _ptr(result), _ptr(mask),
                                             _ptr(workspace), workspace.numel(), _stream(), C.byref(options)), entry)


def _philox_args(philox):
    """``philox`` of a pass, decoded -> (seed as 64 unsigned bits, seed_dev, use_philox, h_begin, seed_stride).  ``None``: the table
    already in S.  Else ``(seed, h_begin[, seed_stride])`` with ``seed`` an int or an int64 device tensor read at kernel run time."""
    if philox is None:
        return 0, None, False, 0, 0
    seed, h_begin, *stride = philox
    on_device = isinstance(seed, torch.Tensor)
    return 0 if on_device else seed & (2**64 - 1), seed if on_device else None, True, h_begin, stride[0] if stride else 1


def _single_pair_pass(op, entry: str, corr, S, E, flags, cnt, s1, s2, result, mask, workspace, thr, min_extra, aggregation,
                      h_offset, philox, options) -> None:
    """``sfm_ransac_pass_small`` / ``_large``: the torch op ``op``, or with per-call ``options`` the C-ABI ``entry``."""
    seed, seed_dev, use_philox, h_begin, _ = _philox_args(philox)
    if options is not None:
        return _pass_with_options(entry, corr, seed, seed_dev, use_philox, h_begin, thr, min_extra, aggregation,
                                  h_offset, S, E, flags, cnt, s1, s2, result, mask, workspace, options)
    op(corr, _as_int64(seed), seed_dev, use_philox, h_begin, float(thr), float(min_extra), int(aggregation), h_offset, S, E, flags,
       cnt, s1, s2, result, mask, workspace)


def ransac_pass_small(corr, S, E, flags, cnt, s1, s2, result, mask, workspace, thr: float, min_extra: float,
                      aggregation: int, h_offset: int = 0, philox=None, options: Optional[ScoreOptions] = None) -> None:
    """One whole pass of a small problem with lean launches (fit + workspace preparation, scoring, sharded selection, mask).
    ``philox=(seed, h_begin)``: samples drawn in the kernel (``seed`` an int or an int64 device tensor), else the
    table already in ``S``.  Same outputs as the separate calls.  ``options``: launch options of this call (default: the
    process-wide set)."""
    _single_pair_pass(ops.load().ransac_pass_small_, "sfm_ransac_pass_small", corr, S, E, flags, cnt, s1, s2, result, mask, workspace,
                      thr, min_extra, aggregation, h_offset, philox, options)


def ransac_pass_large(corr, S, E, flags, cnt, s1, s2, result, mask, workspace, thr: float, min_extra: float,
                      aggregation: int, h_offset: int = 0, philox=None, options: Optional[ScoreOptions] = None) -> None:
    """One whole pass of a large problem (one pair), ``sfm_ransac_pass_large``.  With the matrix-pipe scoring kernel, seven
    launches: partial maxima + zeroing; the fit, whose lanes also write the hypotheses' operand rows and sample corrections and
    whose extra blocks write the point operand table; cost pre-pass, class histogram, scan + scatter (these three only in cost
    order); the scoring kernel; fold of the point ranges + selection + mask.  With the VALU filter: the fit, ``score_sed``'s
    launches, the selection.  Arguments and outputs as ``ransac_pass_small``."""
    _single_pair_pass(ops.load().ransac_pass_large_, "sfm_ransac_pass_large", corr, S, E, flags, cnt, s1, s2, result, mask, workspace,
                      thr, min_extra, aggregation, h_offset, philox, options)


def ransac_pass_batch(corr, S, E, flags, cnt, s1, s2, result, mask, workspace, thr: float, min_extra: float, aggregation: int,
                      philox=None, options: Optional[ScoreOptions] = None) -> None:
    """One whole pass of a BATCH of image pairs (``sfm_ransac_pass_batch``): corr [B,N,4], every other array with the leading
    pair dimension.  ``philox=(seed, h_begin, seed_stride)``: pair b draws from Philox(seed + b * seed_stride) inside the fit
    kernel (``seed`` an int or an int64 device tensor), else the tables already in ``S``.  Same outputs as the separate calls."""
    B, N, _ = corr.shape
    H = S.shape[1]
    seed, seed_dev, use_philox, h_begin, seed_stride = _philox_args(philox)
    with torch.cuda.device(corr.device):
        check(_native.load().sfm_ransac_pass_batch(seed, _ptr(seed_dev), seed_stride, 1 if use_philox else 0, h_begin, _ptr(corr), N, H, B,
                                                   float(thr), float(min_extra), int(aggregation), _ptr(S), _ptr(E), _ptr(flags),
                                                   _ptr(cnt), _ptr(s1), _ptr(s2), _ptr(result), _ptr(mask), _ptr(workspace),
                                                   workspace.numel(), _stream(), None if options is None else C.byref(options)),
              "sfm_ransac_pass_batch")


def batch_pass_eligible(batch: int) -> bool:
    """Whether ``RansacWorkspace.run`` takes the fused batched pass (several pairs; ``SFM_LARGE_PASS=0`` keeps the separate calls)."""
    return (batch > 1 and os.environ.get("SFM_LARGE_PASS", "1") != "0"
            and os.environ.get("SFM_SCORE_KERNEL", "filtered") != "exact")


def large_pass_eligible(batch: int, n: int, h: int) -> bool:
    """Whether ``RansacWorkspace.run`` takes the fused large pass: one pair whose scoring call would launch the matrix-pipe
    kernel (the size rule of ``sfm_score_kernel_choice``).  ``SFM_LARGE_PASS=0`` keeps the separate calls."""
    if batch != 1 or os.environ.get("SFM_LARGE_PASS", "1") == "0" or os.environ.get("SFM_SCORE_KERNEL", "filtered") == "exact":
        return False
    return _native.load().sfm_score_kernel_choice(n, h, 1) == _native.SCORE_KERNEL_MATRIX


def select_best(cnt, s1, s2, flags, min_extra: float, aggregation: int, h_offset: int = 0, out=None, sample_size: int = 8):
    """-> int64 tensor [B,5] viewing the sfm_select_result records.  ``sample_size``: items of a sample in the mean / RMS (8 for
    the eight-point fit, 6 for the five-point fit and the DLT, 4 for P3P)."""
    op = ops.load()
    if out is None:
        return op.select_best(cnt, s1, s2, flags, float(min_extra), int(aggregation), h_offset, int(sample_size))
    op.select_best_(cnt, s1, s2, flags, float(min_extra), int(aggregation), h_offset, out, int(sample_size))
    return out


def inlier_mask(corr, E, S, result, thr: float, out=None, sample_size: int = 8):
    """uint8 [B,N]: 2 on the winner's ``sample_size`` sample items (8, or 6 for the five-point fit), 1 other inlier, 0 outlier."""
    op = ops.load()
    if out is None:
        return op.inlier_mask(corr, E, S, result, float(thr), int(sample_size))
    op.inlier_mask_(corr, E, S, result, float(thr), out, int(sample_size))
    return out


def refine_inliers(corr, E, mask, err, thr: float, aggregation: int, iterations: int = 1):
    """Local optimisation: refit E on all inliers, re-score, keep if better.
    corr [B,N,4], E [B,9], mask uint8 [B,N], err f64 [B] -> (E_out [B,9], mask_out uint8 [B,N],
    info int64 view [B,2]: {error bits, count | accepted << 32}).  No host synchronisation."""
    lib = _native.load()
    B, N, _ = corr.shape
    E_out = torch.empty((B, 9), dtype=F64, device=corr.device)
    mask_out = torch.empty((B, N), dtype=torch.uint8, device=corr.device)
    info = torch.empty((B, 2), dtype=torch.int64, device=corr.device)
    check(lib.sfm_refine_inliers(_ptr(corr), N, B, _ptr(E.contiguous()), _ptr(mask.contiguous()),
                                 _ptr(err.contiguous()), float(thr), int(aggregation), int(iterations),
                                 _ptr(E_out), _ptr(mask_out), _ptr(info), _stream()), "sfm_refine_inliers")
    return E_out, mask_out, info


def _read_records(info: torch.Tensor, doubles: int, ints: int) -> List[tuple]:
    """Host copy of info records held as int64 words (one record, or [B, words]): ``doubles`` leading float64 fields, then
    ``ints`` int32 fields -> one tuple of Python numbers per record (synchronises)."""
    raw = np.ascontiguousarray(info.cpu().numpy()).reshape(-1, info.shape[-1])
    return [tuple(float(v) for v in row[:doubles].view(np.float64)) + tuple(int(v) for v in row[doubles:].view(np.int32)[:ints])
            for row in raw]


def read_refine_info(info: torch.Tensor):
    """Host copy of sfm_refine_info records -> list of (error, count, accepted) (synchronises)."""
    return _read_records(info, 1, 2)


def five_point_fit(corr: torch.Tensor, S: torch.Tensor, E=None, flags=None, philox=None):
    """Five-point fit of every hypothesis from the first six entries of each row of S (``sfm_five_point_fit``): corr [B,N,4],
    S [B,H,8] -> E [B,H,9] (9 NaNs: no real solution), flags [B,H] (SFM_FIT_DEGENERATE).  ``philox=(seed, h_begin,
    seed_stride)``: the samples are drawn in the fit launch, which also fills S."""
    B, N, _ = corr.shape
    H = S.shape[1]
    assert S.shape == (B, H, 8) and S.dtype == torch.int32 and corr.dtype == F64
    op = ops.load()
    if philox is None and E is None and flags is None:
        return op.five_point_fit(corr, S)
    E, flags = _fit_buffers(E, flags, B, H, 9, corr.device)
    if philox is None:
        op.five_point_fit_(corr, S, E, flags)
        return E, flags
    seed, h_begin, stride = philox   # Philox fused into the fit: a diagnostic entry outside the op set, through the C ABI
    with torch.cuda.device(corr.device):
        check(_native.load().sfm_five_point_sample_fit_philox(seed & (2**64 - 1), stride & (2**64 - 1), h_begin, _ptr(corr), N, H, B,
                                                              _ptr(S), _ptr(E), _ptr(flags), _stream()),
              "sfm_five_point_sample_fit_philox")
    return E, flags


def five_point_candidates(corr: torch.Tensor, S: torch.Tensor):
    """Every candidate of items 0-4 of each sample (``sfm_five_point_candidates``) -> (out [B,H,10,9] NaN beyond the count,
    count int32 [B,H], -1 for a degenerate sample)."""
    B, N, _ = corr.shape
    H = S.shape[1]
    assert S.shape == (B, H, 8) and S.dtype == torch.int32 and corr.dtype == F64
    out = torch.empty((B, H, 10, 9), dtype=F64, device=corr.device)
    count = torch.empty((B, H), dtype=torch.int32, device=corr.device)
    with torch.cuda.device(corr.device):
        check(_native.load().sfm_five_point_candidates(_ptr(corr), N, _ptr(S), H, B, _ptr(out), _ptr(count), _stream()),
              "sfm_five_point_candidates")
    return out, count


def five_point_ransac_pass(corr, S, E, flags, cnt, s1, s2, result, mask, thr: float, min_extra: float, aggregation: int,
                           philox=None) -> None:
    """One five-point pass (the ``five_point_ransac_pass_`` op, ``sfm_five_point_ransac_pass``): fit, six-item scoring,
    selection, mask (``mask=None``: none).  ``philox=(seed, h_begin, seed_stride)``: samples drawn in the fit launch."""
    seed, h_begin, stride = (0, 0, 1) if philox is None else philox
    ops.load().five_point_ransac_pass_(corr, _as_int64(seed), _as_int64(stride), philox is not None, h_begin, float(thr),
                                       float(min_extra), int(aggregation), S, E, flags, cnt, s1, s2, result, mask)


def read_select(result: torch.Tensor) -> List[SelectResult]:
    """Copy the select records to the host (synchronises)."""
    raw = result.cpu().numpy().tobytes()
    return [SelectResult.from_buffer_copy(raw[i * SELECT_BYTES:(i + 1) * SELECT_BYTES])
            for i in range(result.shape[0])]


def sed_values(corr: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    lib = _native.load()
    n = corr.shape[0]
    out = torch.empty((n,), dtype=F64, device=corr.device)
    check(lib.sfm_sed_values(_ptr(corr), n, _ptr(E), _ptr(out), _stream()), "sfm_sed_values")
    return out


def cheirality(corr: torch.Tensor, pose_rt: torch.Tensor, distance_threshold: float) -> torch.Tensor:
    return ops.load().cheirality(corr, pose_rt, float(distance_threshold))


def triangulate(corr: torch.Tensor, P1: torch.Tensor, P2: torch.Tensor) -> torch.Tensor:
    return ops.load().triangulate(corr, P1, P2)


def decompose_essential(E: torch.Tensor, out=None):
    """E [B,9] -> pose_rt [B,4,12] (rows R(9)|t(3) in the reference's candidate order), status [B]."""
    lib = _native.load()
    B = E.shape[0]
    if out is None:
        poses = torch.empty((B, 4, 12), dtype=F64, device=E.device)
        status = torch.empty((B,), dtype=torch.int32, device=E.device)
    else:
        poses, status = out
    check(lib.sfm_decompose_essential(_ptr(E), B, _ptr(poses), _ptr(status), _stream()),
          "sfm_decompose_essential")
    return poses, status


# ------------------------------------------------------------------------------------------------------
# host sampler: exact replay of the reference's cumulative random.shuffle (ransac.py:59-64)
# ------------------------------------------------------------------------------------------------------
def pyshuffle_table(n: int, iterations: int, rng=_pyrandom, snapshot_iteration: int = -1,
                    advance: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """Sample table S[iterations, 8] the reference would draw from the current state of ``rng``
    (the ``random`` module or a ``random.Random``), via the C++ MT19937 replay.  With ``advance`` the
    generator state is advanced exactly as ``iterations`` calls of ``random.shuffle`` would.
    Optionally also returns the full permutation after ``snapshot_iteration``."""
    lib = _native.load()
    version, internal, gauss = rng.getstate()
    state = (C.c_uint32 * 624)(*internal[:624])
    index = C.c_int32(internal[624])
    S = np.empty((iterations, 8), dtype=np.int32)
    snap = np.empty((n,), dtype=np.int32) if snapshot_iteration >= 0 else None
    check(lib.sfm_pyshuffle_table(
        C.cast(state, C.c_void_p), C.cast(C.byref(index), C.c_void_p), n, iterations,
        S.ctypes.data_as(C.c_void_p), None, snapshot_iteration,
        snap.ctypes.data_as(C.c_void_p) if snap is not None else None), "sfm_pyshuffle_table")
    if advance:
        rng.setstate((version, tuple(state) + (index.value,), gauss))
    return S, snap


class PyShuffleTable:
    """The sample table of ``iterations`` cumulative ``random.shuffle`` calls (``pyshuffle_table``) that also keeps
    up to ``checkpoints`` snapshots of (generator state, permutation) on the way, so that the full permutation after
    any iteration — the order in which the reference returns the winner's inliers — is re-derived by replaying at
    most ``iterations / checkpoints`` shuffles instead of all of them up to the winner."""

    def __init__(self, n: int, iterations: int, rng=_pyrandom, advance: bool = True, checkpoints: int = 32):
        lib = _native.load()
        self.n, self.iterations = n, iterations
        self.stride = max(1, -(-iterations // max(1, checkpoints)))
        version, internal, gauss = rng.getstate()
        state = (C.c_uint32 * 624)(*internal[:624])
        index = C.c_int32(internal[624])
        perm = np.arange(n, dtype=np.int32)
        self.S = np.empty((iterations, 8), dtype=np.int32)
        self._saved = []  # (state bytes, index, permutation) before each segment
        for start in range(0, iterations, self.stride):
            count = min(self.stride, iterations - start)
            self._saved.append((bytes(state), index.value, perm.copy()))
            check(lib.sfm_pyshuffle_table(
                C.cast(state, C.c_void_p), C.cast(C.byref(index), C.c_void_p), n, count,
                self.S[start:].ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p), -1, None),
                "sfm_pyshuffle_table")
        if advance:
            rng.setstate((version, tuple(state) + (index.value,), gauss))

    def permutation_after(self, iteration: int) -> np.ndarray:
        """The shuffled index list as it stood after ``iteration`` (0-based) — ``data`` of ransac.py:62-64."""
        if not 0 <= iteration < self.iterations:
            raise IndexError(iteration)
        lib = _native.load()
        state_bytes, index_value, perm = self._saved[iteration // self.stride]
        state = (C.c_uint32 * 624).from_buffer_copy(state_bytes)
        index = C.c_int32(index_value)
        perm = perm.copy()
        count = iteration % self.stride + 1
        scratch = np.empty((count, 8), dtype=np.int32)
        check(lib.sfm_pyshuffle_table(
            C.cast(state, C.c_void_p), C.cast(C.byref(index), C.c_void_p), self.n, count,
            scratch.ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p), -1, None), "sfm_pyshuffle_table")
        return perm


# ------------------------------------------------------------------------------------------------------
# the RANSAC engine: sample table -> fit -> score -> select -> mask, all enqueued on one stream
# ------------------------------------------------------------------------------------------------------
def model_matrix(row: np.ndarray) -> np.ndarray:
    """A 9-entry model row (E or H, row-major) as a fresh (3,3) array."""
    return row.reshape(3, 3).copy()


def model_pose(row: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """A 12-entry model row R (9) | t (3) as fresh (3,3) and (3,) arrays."""
    return row[:9].reshape(3, 3).copy(), row[9:].copy()


@dataclass
class PassOutcome:
    """What one entry of a RANSAC pass left, on the host (``_PassWorkspace.outcome``)."""
    best_h: int                # winning hypothesis (global index), -1 if none
    error: float               # aggregated inlier error of the winner
    model: Optional[np.ndarray]    # the winner's row, a flat copy: 9 entries (E or H) or 12 (R | t); None without a winner
    sample: Optional[np.ndarray]   # indices of the winner's sample, in sample order (as many as the pass's solver takes)
    mask: Optional[np.ndarray]     # (N,) uint8: 1 survivor, 2 sample point, 0 outlier
    n_flagged: int             # hypotheses whose sample was degenerate (eight_point.py:415-421)
    first_flagged: int         # lowest such hypothesis index, or -1
    extra_inliers: int

    @property
    def E(self) -> Optional[np.ndarray]:
        """(3,3) of the winner of an essential or homography pass."""
        return None if self.model is None else model_matrix(self.model)

    H = E

    @property
    def R(self) -> Optional[np.ndarray]:
        """(3,3) of the winner of a pose pass."""
        return None if self.model is None else model_pose(self.model)[0]

    @property
    def t(self) -> Optional[np.ndarray]:
        """(3,) of the winner of a pose pass."""
        return None if self.model is None else model_pose(self.model)[1]


def checked_mask(mask: np.ndarray) -> np.ndarray:
    """Inlier mask as read back from the device (0 out, 1 inlier, 2 sample).  The mask blocks of a small pass's
    selection launch wait for the selecting blocks' record with a bounded number of polls and fill their slice with
    0xFF if it never arrives (``select_grid_kernel``): that must surface here, not as an empty inlier list."""
    if mask.size and int(mask.max()) > 2:
        raise RuntimeError("sfm_hip: the inlier mask was not written (the selection record of the pass never arrived)")
    return mask


class _PassWorkspace:
    """What the RANSAC workspaces share: the device buffers of a pass over B entries x H hypotheses x N items whose models are
    ``width`` doubles, and the decoding of the select record it leaves."""

    def __init__(self, batch: int, n: int, h: int, width: int, sample_size: int, device=None):
        dev = device or require_gpu()
        self.batch, self.n, self.h = batch, n, h
        self.S = torch.empty((batch, h, 8), dtype=torch.int32, device=dev)
        self.model = torch.empty((batch, h, width), dtype=F64, device=dev)
        self.flags = torch.empty((batch, h), dtype=torch.int32, device=dev)
        self.cnt = torch.empty((batch, h), dtype=torch.int32, device=dev)
        self.s1 = torch.empty((batch, h), dtype=F64, device=dev)
        self.s2 = torch.empty((batch, h), dtype=F64, device=dev)
        self.result = torch.empty((batch, SELECT_BYTES // 8), dtype=torch.int64, device=dev)
        self.mask = torch.empty((batch, n), dtype=torch.uint8, device=dev)
        self.sample_size = sample_size   # of the last pass (outcome reads it)

    def outcome(self, b: int = 0, h_offset: int = 0) -> PassOutcome:
        """Entry b's record and winner on the host (synchronises); ``h_offset``: the global index of this pass's hypothesis 0."""
        rec = read_select(self.result)[b]
        first = -1 if rec.first_flagged == _native.INT64_MAX else int(rec.first_flagged)
        if rec.best_h < 0:
            return PassOutcome(-1, float("inf"), None, None, None, int(rec.n_flagged), first, 0)
        local = int(rec.best_h) - h_offset
        model = self.model[b, local].cpu().numpy()
        sample = self.S[b, local, :self.sample_size].cpu().numpy().astype(np.int64)
        mask = checked_mask(self.mask[b].cpu().numpy().copy())
        return PassOutcome(int(rec.best_h), float(rec.best_err), model, sample, mask, int(rec.n_flagged), first,
                           int(rec.best_cnt))


class RansacWorkspace(_PassWorkspace):
    """Pre-allocated device buffers for B pairs x H hypotheses x N correspondences."""

    def __init__(self, batch: int, n: int, h: int, device=None):
        super().__init__(batch, n, h, 9, solver_sample_size("essential", "eight_point"), device)
        self.E = self.model
        self.score_ws = score_workspace(n, h, batch, self.S.device)   # (for the process-wide options of this moment: see _fit_workspace)
        self.frozen = False   # set by ShardedRansac.capture: the buffers' addresses are baked into a graph

    def _fit_workspace(self, options: Optional[ScoreOptions]) -> None:
        """The scoring workspace is sized by what a call launches: other options (per call, or process-wide defaults changed
        since this engine was built) may need more — grown here, outside any captured graph, rather than refused by the library."""
        need = score_workspace_bytes(self.n, self.h, self.batch, options)
        if need > self.score_ws.numel():
            if self.frozen:   # a captured HIP graph holds the address of the present buffer
                raise RuntimeError("RansacWorkspace: these launch options need a larger scoring workspace than the one a captured "
                                   "graph of this engine refers to; build a new engine (or capture again) with them")
            self.score_ws = torch.empty((need,), dtype=torch.uint8, device=self.score_ws.device)

    def run(self, corr: torch.Tensor, thr: float, min_extra: float, aggregation: int,
            h_offset: int = 0, with_mask: bool = True, philox=None, options: Optional[ScoreOptions] = None,
            solver: str = "eight_point") -> None:
        """fit + score + select (+ mask) for the sample table currently in ``self.S`` — or, with
        ``philox=(seed, h_begin, seed_stride)``, for Philox samples drawn inside the fit kernel (which also fills
        ``self.S``); ``seed`` may be an int64 device tensor (read at kernel run time).  ``options``: launch options of the
        scoring launch of THIS pass (timing events included); default: the process-wide set.  ``solver="five_point"``: the
        five-point fit on six-item samples (``sfm_five_point_ransac_pass``; an int seed, h_offset 0, no launch options)."""
        self.sample_size = solver_sample_size("essential", solver)
        if solver == "five_point":
            if h_offset != 0 or options is not None or isinstance(philox and philox[0], torch.Tensor):
                raise ValueError("RansacWorkspace.run(solver='five_point'): h_offset, options and a device seed are not supported")
            five_point_ransac_pass(corr, self.S, self.E, self.flags, self.cnt, self.s1, self.s2, self.result,
                                   self.mask if with_mask else None, thr, min_extra, aggregation, philox)
            return
        if not torch.cuda.is_current_stream_capturing():
            self._fit_workspace(options)
        if small_pass_eligible(self.batch, self.n, self.h):
            # workspace preparation rides in the fit launch, selection over 32 blocks (seed_stride only matters for batches)
            ransac_pass_small(corr, self.S, self.E, self.flags, self.cnt, self.s1, self.s2, self.result,
                              self.mask if with_mask else None, self.score_ws, thr, min_extra, aggregation, h_offset,
                              None if philox is None else (philox[0], philox[1]), options)
            return
        if large_pass_eligible(self.batch, self.n, self.h) and (not with_mask or h_offset == 0):
            # seven launches: the operand tables written by the fit launch, the ranges folded inside the selection launch
            ransac_pass_large(corr, self.S, self.E, self.flags, self.cnt, self.s1, self.s2, self.result,
                              self.mask if with_mask else None, self.score_ws, thr, min_extra, aggregation, h_offset,
                              None if philox is None else (philox[0], philox[1]), options)
            return
        if batch_pass_eligible(self.batch) and h_offset == 0:
            # a batch of pairs: partial maxima + zeroing, point tables, fits (+ the hypotheses' operand rows), pre-pass, sort,
            # scoring, and per pair one block that folds the ranges, selects and writes the mask
            ransac_pass_batch(corr, self.S, self.E, self.flags, self.cnt, self.s1, self.s2, self.result,
                              self.mask if with_mask else None, self.score_ws, thr, min_extra, aggregation, philox, options)
            return
        if philox is None:
            fit_eight_point(corr, self.S, self.E, self.flags)
        else:
            seed, h_begin, seed_stride = philox
            sample_fit_philox(corr, seed, h_begin, self.S, self.E, self.flags, seed_stride)
        score_sed(corr, self.E, self.S, thr, self.cnt, self.s1, self.s2, workspace=self.score_ws, options=options)
        select_best(self.cnt, self.s1, self.s2, self.flags, min_extra, aggregation, h_offset,
                    self.result)
        if with_mask:
            assert h_offset == 0, "mask needs local hypothesis indices"
            inlier_mask(corr, self.E, self.S, self.result, thr, self.mask)


def ransac_essential(corr: torch.Tensor, S, thr: float, min_extra: float, aggregation: int) -> PassOutcome:
    """One image pair: corr [N,4] on device, S [H,8] (numpy or tensor) -> PassOutcome."""
    n = corr.shape[0]
    S_t = S if isinstance(S, torch.Tensor) else to_device(S, torch.int32)
    h = S_t.shape[0]
    ws = RansacWorkspace(1, n, h, corr.device)
    ws.S.copy_(S_t.reshape(1, h, 8))
    ws.run(corr.reshape(1, n, 4), thr, min_extra, aggregation)
    return ws.outcome(0)


# ------------------------------------------------------------------------------------------------------
# RANSAC absolute pose (PnP, csrc/sfm_pnp.hip): pts [B,N,5] = {X, Y, Z, u, v}, K (3,3) with row 2 = (0, 0, 1),
# S [B,H,8] (first 6 entries used), model [B,H,12] = R (9) | t (3)
# ------------------------------------------------------------------------------------------------------
def _camera_list(K) -> List[float]:
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"camera matrix must be 3x3, got shape {K.shape}")
    return [float(v) for v in K.reshape(9)]


def _pose_fit(fit, fit_, pts, S, K, model, flags):
    """``fit`` / ``fit_``: the functional and the in-place op of one pose solver."""
    if model is None and flags is None:
        return fit(pts, S, _camera_list(K))
    model, flags = _fit_buffers(model, flags, S.shape[0], S.shape[1], 12, pts.device)
    fit_(pts, S, _camera_list(K), model, flags)
    return model, flags


def pnp_fit(pts: torch.Tensor, S: torch.Tensor, K, model=None, flags=None):
    """Six-point DLT fit of every hypothesis -> model [B,H,12], flags [B,H] (SFM_FIT_DEGENERATE)."""
    op = ops.load()
    return _pose_fit(op.pnp_fit, op.pnp_fit_, pts, S, K, model, flags)


def p3p_fit(pts: torch.Tensor, S: torch.Tensor, K, model=None, flags=None):
    """P3P fit of every hypothesis from the first four entries of each row of S -> model [B,H,12] (12 NaNs: no solution),
    flags [B,H] (SFM_FIT_DEGENERATE: collinear solve points or an index out of range)."""
    op = ops.load()
    return _pose_fit(op.p3p_fit, op.p3p_fit_, pts, S, K, model, flags)


def pnp_score(pts: torch.Tensor, model: torch.Tensor, S: torch.Tensor, K, thr: float, cnt=None, s1=None, s2=None,
              sample_size: int = 6):
    """Per hypothesis (extra-inlier count, sum e, sum e^2) of the squared reprojection error e; the first ``sample_size``
    (6 or 4) entries of each row of S are the sample.  Selection: ``select_best`` with the same ``sample_size``."""
    op = ops.load()
    if cnt is None and s1 is None and s2 is None:
        return op.pnp_score(pts, model, S, _camera_list(K), float(thr), int(sample_size))
    op.pnp_score_(pts, model, S, _camera_list(K), float(thr), cnt, s1, s2, int(sample_size))
    return cnt, s1, s2


def pnp_inlier_mask(pts, model, S, K, result, thr: float, out=None, sample_size: int = 6):
    """uint8 [B,N]: 2 sample point of the winner (the first ``sample_size`` entries of its row of S), 1 other inlier,
    0 outlier."""
    B, N, _ = pts.shape
    if out is None:
        out = torch.empty((B, N), dtype=torch.uint8, device=pts.device)
    Kc = (C.c_double * 9)(*_camera_list(K))
    check(_native.load().sfm_pnp_inlier_mask(_ptr(pts), N, _ptr(model), _ptr(S), S.shape[1], B, C.cast(Kc, C.c_void_p),
                                              _ptr(result), float(thr), int(sample_size), _ptr(out), _stream()),
          "sfm_pnp_inlier_mask")
    return out


def pnp_refine(pts, model, mask, err, K, thr: float, aggregation: int, rounds: int = 1, max_steps: int = 20):
    """Levenberg-Marquardt refinement of one pose per view on its inliers, re-scored and kept only if better
    (``sfm_pnp_refine``).  pts [B,N,5], model f64 [B,12] (R | t), mask uint8 [B,N] (non-zero = inlier), err f64 [B] (the
    aggregated error of ``model``) -> (model_out [B,12], mask_out uint8 [B,N] (1 = inlier), info int64 [B,3] viewing
    sfm_pnp_refine_info records; ``read_pnp_refine_info``).  No host synchronisation."""
    return ops.load().pnp_refine(pts, model.contiguous(), mask.contiguous(), err.contiguous(), _camera_list(K), float(thr),
                                 int(aggregation), int(rounds), int(max_steps))


@dataclass
class PnPRefineInfo:
    error: float     # aggregated error of the model left in model_out, over its `count` inliers
    count: int       # inliers of that model
    accepted: int    # rounds whose result was kept (0: model_out is the input model)
    lm_steps: int    # Levenberg-Marquardt trial steps over all rounds


def read_pnp_refine_info(info: torch.Tensor) -> List[PnPRefineInfo]:
    """Host copy of sfm_pnp_refine_info records (int64 [B,3]) (synchronises)."""
    return [PnPRefineInfo(*fields) for fields in _read_records(info, 1, 3)]


# ------------------------------------------------------------------------------------------------------
# bundle adjustment (csrc/sfm_bundle.hip): poses [C,12] = R (9) | t (3) world -> camera, points [P,3], observations
# (camera index, point index) int32 [M] each and pixels [M,2]
# ------------------------------------------------------------------------------------------------------
BUNDLE_LOSSES = _native.BUNDLE_LOSSES   # "squared", "huber", "cauchy": the index is the SFM_BUNDLE_LOSS_* code


def _bundle_loss(loss: str, loss_scale: float):
    """(code, scale) of a loss name; ValueError for an unknown name or a scale that is not positive with a normal finite
    square (``_native.loss_scale_ok``)."""
    if loss not in BUNDLE_LOSSES:
        raise ValueError(f"loss must be one of {BUNDLE_LOSSES}, got {loss!r}")
    scale = float(loss_scale)
    if not _native.loss_scale_ok(scale):
        raise ValueError(f"loss_scale must be positive with a normal finite square, got {loss_scale!r}")
    return BUNDLE_LOSSES.index(loss), scale


def _bundle(name: str, poses, points, camera_indices, point_indices, pixels, K, fixed, max_steps, cg, out, loss, loss_scale):
    """The op ``name`` (its ``_robust`` form for a loss other than "squared", its ``_`` form with ``out``); ``cg`` is () or
    (max_cg_iterations, cg_tolerance)."""
    code, scale = _bundle_loss(loss, loss_scale)
    op = ops.load()
    args = (camera_indices.contiguous(), point_indices.contiguous(), pixels.contiguous(), _camera_list(K),
            [int(c) for c in fixed], int(max_steps), *((int(cg[0]), float(cg[1])) if cg else ()))
    if code != 0:
        name, args = name + "_robust", args + (code, scale)
    if out is None:
        return getattr(op, name)(poses.contiguous(), points.contiguous(), *args)
    getattr(op, name + "_")(out[0], out[1], *args, out[2])
    return out


def bundle_adjust(poses, points, camera_indices, point_indices, pixels, K, fixed=(0,), max_steps: int = 50, out=None, *,
                  loss: str = "squared", loss_scale: float = 1.0):
    """Levenberg-Marquardt over the free cameras and the points seen at least twice (``sfm_bundle_adjust``) ->
    (poses [C,12], points [P,3], info int64 [4] viewing the sfm_bundle_info record; ``read_bundle_info``).  ``out`` =
    (poses, points, info) runs the in-place op on those tensors instead (poses and points there are the input).  No host
    synchronisation: the whole call is enqueued at once.  ``loss`` in ``BUNDLE_LOSSES`` with ``loss_scale`` in pixels
    (DESIGN.md §6n): ``"squared"`` is the op without a loss, the others run ``bundle_adjust_robust`` and the costs in
    ``info`` are sums of rho."""
    return _bundle("bundle_adjust", poses, points, camera_indices, point_indices, pixels, K, fixed, max_steps, (), out, loss,
                   loss_scale)


@dataclass
class BundleInfo:
    initial_cost: float   # cost of the input (NaN when an index is out of range)
    final_cost: float     # cost of the last accepted trial (initial_cost when none was accepted)
    steps: int            # Levenberg-Marquardt trial steps
    accepted: int         # accepted steps
    status: int           # BUNDLE_OK, BUNDLE_BAD_START or BUNDLE_BAD_INDEX


BUNDLE_OK, BUNDLE_BAD_START, BUNDLE_BAD_INDEX = 0, 1, 2


def read_bundle_info(info: torch.Tensor) -> BundleInfo:
    """Host copy of an sfm_bundle_info record (int64 [4]) (synchronises)."""
    return BundleInfo(*_read_records(info, 2, 3)[0])


BUNDLE_REFINE = _native.BUNDLE_REFINE   # "focal", "principal_point": the SFM_BUNDLE_REFINE_* bit of each name


def bundle_adjust_calibrated(poses, points, camera_indices, point_indices, pixels, K, fixed=(0,), max_steps: int = 50,
                             out=None, *, refine=("focal",), loss: str = "squared", loss_scale: float = 1.0):
    """``bundle_adjust`` that also refines intrinsics shared by all cameras (``sfm_bundle_adjust_calibrated``, DESIGN.md
    §6ab) -> (poses [C,12], points [P,3], info int64 [4], K_out [3,3]; ``read_bundle_calibration_info``).  ``refine``: a
    non-empty collection of ``BUNDLE_REFINE`` names; ``K`` is the start.  ``out`` = (poses, points, info, K_out) runs the
    in-place op on those tensors instead.  No host synchronisation: ``K_out`` is written on the device."""
    mask = _native.bundle_refine_mask(refine)
    if mask == 0:
        raise ValueError("bundle_adjust_calibrated needs at least one intrinsic to refine; bundle_adjust refines none")
    code, scale = _bundle_loss(loss, loss_scale)
    args = (camera_indices.contiguous(), point_indices.contiguous(), pixels.contiguous(), _camera_list(K),
            [int(c) for c in fixed], int(max_steps), code, scale, mask)
    if out is None:
        return ops.load().bundle_adjust_calibrated(poses.contiguous(), points.contiguous(), *args)
    ops.load().bundle_adjust_calibrated_(out[0], out[1], *args, out[2], out[3])
    return out


@dataclass
class BundleCalibrationInfo(BundleInfo):   # sfm_bundle_info, then
    camera_matrix: np.ndarray   # the refined K (3, 3); the input K for BUNDLE_BAD_START and BUNDLE_BAD_INDEX


def read_bundle_calibration_info(info: torch.Tensor, K_out: torch.Tensor) -> BundleCalibrationInfo:
    """Host copy of the sfm_bundle_info record and the camera matrix of a calibrating call (synchronises)."""
    return BundleCalibrationInfo(*_read_records(info, 2, 3)[0], K_out.cpu().numpy().reshape(3, 3).copy())


def bundle_adjust_pcg(poses, points, camera_indices, point_indices, pixels, K, fixed=(0,), max_steps: int = 50,
                      max_cg_iterations: int = 100, cg_tolerance: float = 0.1, out=None, *, loss: str = "squared",
                      loss_scale: float = 1.0):
    """``bundle_adjust`` over any number of cameras with the iterative Schur solver (``sfm_bundle_adjust_pcg``,
    DESIGN.md §6j) -> (poses [C,12], points [P,3], info int64 [5] viewing the sfm_bundle_pcg_info record;
    ``read_bundle_pcg_info``).  ``out`` = (poses, points, info) runs the in-place op on those tensors instead.  The call
    synchronises the current stream: the host reads the stop flags between LM steps and CG chunks.  ``loss`` and
    ``loss_scale`` as in ``bundle_adjust`` (``bundle_adjust_pcg_robust`` for a non-squared loss)."""
    return _bundle("bundle_adjust_pcg", poses, points, camera_indices, point_indices, pixels, K, fixed, max_steps,
                   (max_cg_iterations, cg_tolerance), out, loss, loss_scale)


@dataclass
class BundlePcgInfo(BundleInfo):   # sfm_bundle_pcg_info: the fields of sfm_bundle_info, then
    cg_iterations: int    # conjugate-gradient iterations over all trial steps
    cg_max: int           # the most conjugate-gradient iterations of one trial step


def read_bundle_pcg_info(info: torch.Tensor) -> BundlePcgInfo:
    """Host copy of an sfm_bundle_pcg_info record (int64 [5]) (synchronises)."""
    return BundlePcgInfo(*_read_records(info, 2, 5)[0])


# ------------------------------------------------------------------------------------------------------
# the solvers over a view graph: one set of statuses and one info record (sfm_rotavg_info and sfm_transavg_info have one
# layout) under the names of both
# ------------------------------------------------------------------------------------------------------
GRAPH_STATUS = ROTAVG_STATUS = TRANSAVG_STATUS = _native.GRAPH_STATUS   # the index is the SFM_ROTAVG_* / SFM_TRANSAVG_* code
ROTAVG_CONVERGED, ROTAVG_MAX_STEPS, ROTAVG_CG_FAILED, ROTAVG_BAD_INDEX = 0, 1, 2, 3
TRANSAVG_CONVERGED, TRANSAVG_MAX_STEPS, TRANSAVG_CG_FAILED, TRANSAVG_BAD_INDEX = 0, 1, 2, 3


@dataclass
class GraphInfo:
    initial_cost: float   # sum of w rho(e) over the used edges at the first linearisation (NaN for *_BAD_INDEX)
    final_cost: float     # ... at the result
    steps: int            # completed steps
    status: int           # ROTAVG_* / TRANSAVG_*
    cg_iterations: int    # conjugate-gradient iterations over all steps
    cg_max: int           # the most conjugate-gradient iterations of one step
    registered: int       # cameras with a level, the root included
    rounds: int           # the largest level


def read_graph_info(info: torch.Tensor) -> GraphInfo:
    """Host copy of an sfm_rotavg_info or sfm_transavg_info record (int64 [5]) (synchronises)."""
    return GraphInfo(*_read_records(info, 2, 6)[0])


RotavgInfo = TransavgInfo = GraphInfo
read_rotavg_info = read_transavg_info = read_graph_info


# ------------------------------------------------------------------------------------------------------
# rotation averaging over a view graph (csrc/sfm_rotation_averaging.hip): pairs int32 [Q,2], relative rotations [Q,3,3]
# (R_q ~ R_j R_i^T), weights [Q]
# ------------------------------------------------------------------------------------------------------
def average_rotations(pairs, relative, weights, cameras: int, root: int = 0, initial=None, loss: str = "squared",
                      loss_scale: float = 1.0, max_steps: int = 50, max_cg_iterations: int = 500, cg_tolerance: float = 1e-6,
                      step_tolerance: float = 1e-8):
    """One absolute rotation per camera from the relative rotations of a graph (``sfm_average_rotations``)
    -> (rotations [C,3,3], registered uint8 [C], level int32 [C] (-1: unregistered), residual [Q] in radians, info int64 [5] viewing the sfm_rotavg_info record;
    ``read_rotavg_info``).  ``initial`` [C,3,3] starts from those rotations instead of the spanning tree.  ``loss`` in
    ``BUNDLE_LOSSES`` with ``loss_scale`` in radians.  The call synchronises the current stream: the host reads the stop
    flags between level rounds, steps and CG chunks."""
    code, scale = _bundle_loss(loss, loss_scale)
    op = ops.load()
    return op.average_rotations(pairs.contiguous(), relative.contiguous(), weights.contiguous(), int(cameras), int(root),
                                None if initial is None else initial.contiguous(), code, scale, int(max_steps),
                                int(max_cg_iterations), float(cg_tolerance), float(step_tolerance))


# ------------------------------------------------------------------------------------------------------
# translation averaging over a view graph (csrc/sfm_translation_averaging.hip): pairs int32 [Q,2], directions [Q,3] (the world
# directions v_q ~ c_j - c_i, or with ``rotations`` the pairs' t_q), weights [Q]
# ------------------------------------------------------------------------------------------------------
def average_translations(pairs, directions, weights, cameras: int, root: int = 0, rotations=None, initial=None,
                         loss: str = "squared", loss_scale: float = 1.0, warmup_steps: int = 10, max_steps: int = 500,
                         max_cg_iterations: int = 500, cg_tolerance: float = 1e-6, step_tolerance: float = 1e-8):
    """One position per camera from one direction per edge of a graph (``sfm_average_translations``)
    -> (positions [C,3], registered uint8 [C], level int32 [C] (-1: unregistered), residual [Q] in radians, scale [Q], info
    int64 [5] viewing the sfm_transavg_info record; ``read_transavg_info``).  ``rotations`` [C,3,3] (world -> camera): the
    directions are the pairs' ``t_q`` and the world directions are computed on the device.  ``initial`` [C,3] starts from
    those positions instead of the spanning tree.  ``loss`` in ``BUNDLE_LOSSES`` with ``loss_scale`` a sine.  The call
    synchronises the current stream: the host reads the stop flags between level rounds, steps and CG chunks."""
    code, scale = _bundle_loss(loss, loss_scale)
    op = ops.load()
    return op.average_translations(pairs.contiguous(), directions.contiguous(),
                                   None if rotations is None else rotations.contiguous(), weights.contiguous(), int(cameras),
                                   int(root), None if initial is None else initial.contiguous(), code, scale,
                                   int(warmup_steps), int(max_steps), int(max_cg_iterations), float(cg_tolerance),
                                   float(step_tolerance))


# ------------------------------------------------------------------------------------------------------
# triangulation of multi-view tracks (csrc/sfm_tracks.hip): poses [C,12] = R (9) | t (3) world -> camera, observations
# (camera index, point index) int32 [M] each and pixels [M,2]
# ------------------------------------------------------------------------------------------------------
def triangulate_tracks(poses, camera_indices, point_indices, pixels, points: int, K, min_views: int = 2,
                       min_angle: float = 0.0, max_error: float = float("inf"), refine_steps: int = 0, out=None):
    """N-view DLT of every point from its observations, optional per-point LM and the quality checks
    (``sfm_triangulate_tracks``) -> (points [P,3], status uint8 [P] (TRACKS_*), obs_error [M] (px^2), angle [P]
    (radians), info int64 [4] viewing the sfm_tracks_info record; ``read_tracks_info``).  ``out`` = those five tensors runs
    the in-place op on them instead.  No host synchronisation."""
    op = ops.load()
    args = (poses.contiguous(), camera_indices.contiguous(), point_indices.contiguous(), pixels.contiguous(), int(points),
            _camera_list(K), int(min_views), float(min_angle), float(max_error), int(refine_steps))
    if out is None:
        return op.triangulate_tracks(*args)
    op.triangulate_tracks_(*args, *out)
    return out


@dataclass
class TracksInfo:
    status: int                  # 0, or 1 when a camera or point index is out of range (every point TRACKS_BAD_INDEX)
    points_ok: int               # points with TRACKS_OK
    max_refine_steps_taken: int  # the most LM trial steps of any point


TRACKS_OK, TRACKS_FEW_VIEWS, TRACKS_DEGENERATE, TRACKS_BEHIND, TRACKS_SMALL_ANGLE, TRACKS_LARGE_ERROR, TRACKS_BAD_INDEX = range(7)


def read_tracks_info(info: torch.Tensor) -> TracksInfo:
    """Host copy of an sfm_tracks_info record (int64 [4]) (synchronises)."""
    raw = info.cpu().numpy()
    return TracksInfo(int(raw[0]), int(raw[1]), int(raw[2]))


# ------------------------------------------------------------------------------------------------------
# outlier-robust triangulation of multi-view tracks (csrc/sfm_tracks_robust.hip): the inputs of triangulate_tracks
# ------------------------------------------------------------------------------------------------------
TRACKS_NO_CONSENSUS = 7


def triangulate_tracks_robust(poses, camera_indices, point_indices, pixels, points: int, K, max_error: float, min_views: int = 2,
                              min_angle: float = 0.0, refine_steps: int = 0, max_hypotheses: int = 64, out=None, workspace=None):
    """Per-track RANSAC over two-view hypotheses, MSAC scoring, refit on the winner's inliers (``sfm_triangulate_tracks_robust``,
    DESIGN.md section 6ae; ctypes: there is no torch op) -> ((points [P,3], status uint8 [P] (TRACKS_*), obs_error [M] (px^2),
    inlier uint8 [M], angle [P] (radians), info int64 [6] viewing the sfm_tracks_robust_info record; ``read_robust_tracks_info``),
    the workspace it used: ``workspace`` when that is large enough, else a new one).  ``out`` = those six tensors are written
    instead of new ones.  No host synchronisation."""
    lib = _native.load()
    P, M, Cn = int(points), int(pixels.shape[0]), int(poses.shape[0])
    need = int(lib.sfm_tracks_robust_workspace_bytes(P, M))
    if need < 0:
        raise ValueError("triangulate_tracks_robust: sizes out of range (observations below 2^31, points below 2^31 - 1)")
    dev = pixels.device
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty((P, 3), dtype=F64, device=dev), torch.empty((P,), dtype=torch.uint8, device=dev),
               torch.empty((M,), dtype=F64, device=dev), torch.empty((M,), dtype=torch.uint8, device=dev),
               torch.empty((P,), dtype=F64, device=dev), torch.empty((6,), dtype=torch.int64, device=dev))
    X, status, err, inlier, angle, info = out
    poses, camera_indices, point_indices, pixels = (t.contiguous() for t in (poses, camera_indices, point_indices, pixels))
    Kc = (C.c_double * 9)(*_camera_list(K))
    check(lib.sfm_triangulate_tracks_robust(Kc, Cn, P, M, _ptr(poses), _ptr(camera_indices), _ptr(point_indices), _ptr(pixels),
                                            int(min_views), float(min_angle), float(max_error), int(refine_steps),
                                            int(max_hypotheses), _ptr(X), _ptr(status), _ptr(err), _ptr(inlier), _ptr(angle),
                                            _ptr(info), _ptr(workspace), workspace.numel(), _stream()),
          "sfm_triangulate_tracks_robust")
    return out, workspace


@dataclass
class RobustTracksInfo:
    status: int                  # 0, or 1 when a camera or point index is out of range (every point TRACKS_BAD_INDEX)
    points_ok: int               # points with TRACKS_OK
    max_refine_steps_taken: int  # the most LM trial steps of any point
    inlier_observations: int     # the inlier flags set on points with TRACKS_OK
    hypotheses: int              # valid hypotheses scored, summed over the points


def read_robust_tracks_info(info: torch.Tensor) -> RobustTracksInfo:
    """Host copy of an sfm_tracks_robust_info record (int64 [6]) (synchronises)."""
    raw = info.cpu().numpy()
    return RobustTracksInfo(*(int(v) for v in raw[:5]))


# ------------------------------------------------------------------------------------------------------
# multi-view tracks from pairwise matches (csrc/sfm_track_build.hip): image_offset int32 [I+1], pair_images int32 [Q,2],
# match_offset int32 [Q+1], match_index int32 [E,2] (local indices in the pair's two images)
# ------------------------------------------------------------------------------------------------------
def build_tracks(image_offset, pair_images, match_offset, match_index, features: int, out=None):
    """Connected components of the match graph, conflicts dropped, tracks numbered by smallest feature id
    (``sfm_build_tracks``) -> (component, track, status uint8 (BUILD_*), camera_index, point_index, feature_index, info
    int64 [6] viewing the sfm_build_tracks_info record; ``read_track_build_info``).  Every array but info has ``features``
    entries; the observation arrays hold info.observations valid entries, then -1.  ``out`` = those seven tensors runs the
    in-place op on them instead.  No host synchronisation."""
    op = ops.load()
    args = (image_offset.contiguous(), pair_images.contiguous(), match_offset.contiguous(), match_index.contiguous(),
            int(features))
    if out is None:
        return op.build_tracks(*args)
    op.build_tracks_(*args, *out)
    return out


BUILD_OK, BUILD_UNMATCHED, BUILD_CONFLICT, BUILD_BAD_INDEX = range(4)


@dataclass
class TrackBuildInfo:
    status: int        # 0; 1 an input out of range (every feature BUILD_BAD_INDEX); 2 a bounded device loop gave up
    components: int    # components of two or more features
    tracks: int        # OK components
    observations: int  # M, the features of OK components
    conflicts: int     # components holding two features of one image (dropped)
    unmatched: int     # features no match touches


def read_track_build_info(info: torch.Tensor) -> TrackBuildInfo:
    """Host copy of an sfm_build_tracks_info record (int64 [6]) (synchronises)."""
    raw = info.cpu().numpy()
    return TrackBuildInfo(*(int(v) for v in raw[:6]))


# ------------------------------------------------------------------------------------------------------
# descriptor matching of every image pair of a collection (csrc/sfm_match_pairs.hip): image_offset int32 [I+1] and pair_images
# int32 [Q,2] as above, row_offset int64 [Q+1] = running sum of the first images' sizes
# ------------------------------------------------------------------------------------------------------
def match_pairs_options(max_distance: int = 64, ratio: Optional[float] = 0.8, cross_check: bool = True):
    """The sfm_match_pairs_options record of these choices (``ratio=None``: no ratio test)."""
    return _native.MatchPairsOptions(int(max_distance), int(bool(cross_check)), int(ratio is not None), 0,
                                     0.0 if ratio is None else float(ratio))


def match_pairs(images: int, features: int, image_offset, desc, ok, pair_images, row_offset, rows: int, max_image_features: int,
                max_distance: int, ratio: Optional[float], cross_check: bool, partner, distance, pair_status, workspace=None):
    """Nearest, ratio-tested and cross-checked partner of every row of every pair (``sfm_match_pairs``; ctypes: there is no
    torch op, like the other matchers) into ``partner`` / ``distance`` int32 [rows] and ``pair_status`` int32 [Q].  Returns the
    workspace it used: ``workspace`` when that is large enough, else a new one.  No host synchronisation."""
    lib = _native.load()
    Q = int(pair_images.shape[0])
    need = int(lib.sfm_match_pairs_workspace_bytes(Q, int(rows), int(max_image_features)))
    if need < 0:
        raise ValueError("match_pairs: sizes out of range (at most 65535 pairs per call, rows and image sizes below 2^31)")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=desc.device)
    options = match_pairs_options(max_distance, ratio, cross_check)
    check(lib.sfm_match_pairs(int(images), int(features), Q, int(rows), int(max_image_features), _ptr(image_offset), _ptr(desc),
                              _ptr(ok), _ptr(pair_images), _ptr(row_offset), C.byref(options), _ptr(partner),
                              _ptr(distance), _ptr(pair_status), _ptr(workspace), workspace.numel(), _stream()),
          "sfm_match_pairs")
    return workspace


def match_pairs_guided(images: int, features: int, image_offset, desc, ok, xy, pair_images, row_offset, model, model_kind,
                       threshold, rows: int, max_image_features: int, max_distance: int, ratio: Optional[float],
                       cross_check: bool, partner, distance, pair_status, workspace=None):
    """``match_pairs`` restricted to the partners each pair's two-view model admits (``sfm_match_pairs_guided``, DESIGN.md
    section 6ad; ctypes like ``match_pairs``): ``xy`` float64 [F, 2] K-normalised, ``model`` float64 [Q, 9], ``model_kind`` int32
    [Q] (0 none, 1 essential, 2 homography) and ``threshold`` float64 [Q].  Returns the workspace it used, which is
    ``match_pairs``'s.  No host synchronisation."""
    lib = _native.load()
    Q = int(pair_images.shape[0])
    need = int(lib.sfm_match_pairs_workspace_bytes(Q, int(rows), int(max_image_features)))
    if need < 0:
        raise ValueError("match_pairs_guided: sizes out of range (at most 65535 pairs per call, rows and image sizes below 2^31)")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=desc.device)
    options = match_pairs_options(max_distance, ratio, cross_check)
    check(lib.sfm_match_pairs_guided(int(images), int(features), Q, int(rows), int(max_image_features), _ptr(image_offset),
                                     _ptr(desc), _ptr(ok), _ptr(xy), _ptr(pair_images), _ptr(row_offset), _ptr(model),
                                     _ptr(model_kind), _ptr(threshold), C.byref(options), _ptr(partner), _ptr(distance),
                                     _ptr(pair_status), _ptr(workspace), workspace.numel(), _stream()),
          "sfm_match_pairs_guided")
    return workspace


# ------------------------------------------------------------------------------------------------------
# multi-scale FAST keypoints with BRIEF per pyramid level (csrc/sfm_keypoints.hip)
# ------------------------------------------------------------------------------------------------------
def keypoint_plane_table(rows):
    """The sfm_keypoint_plane array (HOST memory) of ``rows`` = (image, level, height, width, offset, quota) per plane."""
    table = (_native.KeypointPlane * max(len(rows), 1))()
    for entry, (image, level, height, width, offset, quota) in zip(table, rows):
        entry.image, entry.level, entry.height, entry.width = int(image), int(level), int(height), int(width)
        entry.offset, entry.quota, entry.reserved = int(offset), int(quota), 0
    return table


def detect_keypoints(table, planes: int, images: int, pool, threshold: int, offsets, boundaries, bins: int, score, kept,
                     capacity: int, counter, candidates, desc, ok, angle_bin, workspace=None):
    """Pyramid, FAST score, suppression, cutoff, candidates and descriptors of every plane of ``table`` in one submission
    (``sfm_detect_keypoints``; ctypes: there is no torch op, like the matchers).  ``pool`` uint8 holds the level-0 planes and
    receives the others, ``score`` / ``kept`` uint16 of the pool's length receive both maps, ``counter`` int32 [1] the number of
    candidates (it may exceed ``capacity``), ``candidates`` int32 [capacity, 4] = (plane, x, y, score), ``desc`` uint8
    [capacity, 32], ``ok`` / ``angle_bin`` uint8 [capacity].  Returns the workspace it used: ``workspace`` when that is large
    enough, else a new one.  No host synchronisation beyond the upload of the table."""
    lib = _native.load()
    need = int(lib.sfm_detect_keypoints_workspace_bytes(int(planes)))
    if need < 0:
        raise ValueError("detect_keypoints: at most 65535 planes per call")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=pool.device)
    check(lib.sfm_detect_keypoints(table, int(planes), int(images), _ptr(pool), pool.numel(), int(threshold), _ptr(offsets),
                                   _ptr(boundaries), int(bins), _ptr(score), _ptr(kept), int(capacity), _ptr(counter),
                                   _ptr(candidates), _ptr(desc), _ptr(ok), _ptr(angle_bin), _ptr(workspace), workspace.numel(),
                                   _stream()), "sfm_detect_keypoints")
    return workspace


def build_pyramid(table, planes: int, images: int, pool, workspace=None):
    """The planes above level 0 of every image of ``table`` into ``pool`` (``sfm_build_pyramid``; ctypes like
    ``detect_keypoints``, whose pyramid it is): the caller has put every image into its level-0 plane.  Returns the workspace it
    used: ``workspace`` when that is large enough, else a new one.  No host synchronisation beyond the upload of the table."""
    lib = _native.load()
    need = int(lib.sfm_build_pyramid_workspace_bytes(int(planes)))
    if need < 0:
        raise ValueError("build_pyramid: at most 65535 planes per call")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=pool.device)
    check(lib.sfm_build_pyramid(table, int(planes), int(images), _ptr(pool), pool.numel(), _ptr(workspace), workspace.numel(),
                                _stream()), "sfm_build_pyramid")
    return workspace


# the statuses of refine_observations (SFM_REFINE_* of include/sfm_hip.h)
(REFINE_OK, REFINE_REFERENCE, REFINE_BAD_INDEX, REFINE_OUTSIDE, REFINE_FLAT, REFINE_SINGULAR, REFINE_DIVERGED,
 REFINE_LOW_CORRELATION) = range(8)


def refine_observations(table, planes: int, images: int, pool, plane, x, y, reference, warp0, radius: int, max_iterations: int,
                        min_step: float, max_shift: float, min_correlation: float, xy, warp, correlation, iterations, status,
                        workspace=None):
    """Sub-pixel alignment of every observation with its reference observation (``sfm_refine_observations``, DESIGN.md section
    6al; ctypes like ``detect_keypoints``).  ``table`` / ``pool``: the plane table and the filled pixel pool; ``plane``, ``x``,
    ``y``, ``reference`` int32 [M]; ``warp0`` float64 [M, 4]; outputs ``xy`` float64 [M, 2] (level pixels), ``warp`` float64
    [M, 4], ``correlation`` float64 [M], ``iterations`` / ``status`` int32 [M].  Returns the workspace it used.  No host
    synchronisation beyond the upload of the table."""
    lib = _native.load()
    need = int(lib.sfm_refine_observations_workspace_bytes(int(planes)))
    if need < 0:
        raise ValueError("refine_observations: at most 65535 planes per call")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=pool.device)
    check(lib.sfm_refine_observations(table, int(planes), int(images), _ptr(pool), pool.numel(), int(plane.numel()), _ptr(plane),
                                      _ptr(x), _ptr(y), _ptr(reference), _ptr(warp0), int(radius), int(max_iterations),
                                      float(min_step), float(max_shift), float(min_correlation), _ptr(xy), _ptr(warp),
                                      _ptr(correlation), _ptr(iterations), _ptr(status), _ptr(workspace), workspace.numel(),
                                      _stream()), "sfm_refine_observations")
    return workspace


class PnPWorkspace(_PassWorkspace):
    """Pre-allocated device buffers of a PnP pass for B views x H hypotheses x N 2D-3D pairs (as RansacWorkspace)."""

    def __init__(self, batch: int, n: int, h: int, device=None):
        super().__init__(batch, n, h, 12, solver_sample_size("pose", "dlt"), device)   # (refine reads sample_size too)

    def run(self, pts: torch.Tensor, K, thr: float, min_extra: float, aggregation: int, with_mask: bool = True,
            philox=None, solver: str = "dlt") -> None:
        """fit + score + select (+ mask) in one call (``sfm_pnp_ransac_pass``) for the sample table in ``self.S`` — or, with
        ``philox=(seed, h_begin, seed_stride)``, for Philox samples drawn inside the fit launch (which also fills ``self.S``).
        ``solver="p3p"``: the P3P fit on four-item samples; ``outcome`` and ``refine`` then read this pass."""
        self.sample_size = solver_sample_size("pose", solver)
        seed, h_begin, stride = (0, 0, 1) if philox is None else philox
        op = ops.load()
        run_pass = op.p3p_ransac_pass_ if solver == "p3p" else op.pnp_ransac_pass_
        run_pass(pts, _as_int64(seed), _as_int64(stride), philox is not None, h_begin, _camera_list(K), float(thr),
                 float(min_extra), int(aggregation), self.S, self.model, self.flags, self.cnt, self.s1, self.s2, self.result,
                 self.mask if with_mask else None)

    def refine(self, pts: torch.Tensor, K, thr: float, aggregation: int, rounds: int = 1, max_steps: int = 20):
        """``pnp_refine`` of every view's winner, chained on this pass's buffers: model[b, best_h] (row 0 when a view has no
        winner: its mask is all zero and it keeps that row), the pass's mask and the record's best_err.  Stream-ordered
        after ``run``: no host round trip.  -> (model_out [B,12], mask_out [B,N], info [B,3]).

        After a P3P pass the winner's sample item 3 does not seed the refinement: P3P reproduces items 0-2 exactly, while
        item 3 only picked the solution and can be an outlier of a good pose, which would then dominate the least squares.
        The re-score of every item counts it again if it fits."""
        rows = torch.arange(self.batch, device=self.result.device)
        best_h = self.result[:, 1].clamp(min=0)
        model = self.model[rows, best_h]
        err = self.result[:, 2].contiguous().view(F64)
        mask = self.mask
        if self.sample_size == solver_sample_size("pose", "p3p"):
            mask = mask.clone()
            mask[rows, self.S[rows, best_h, 3].long().clamp(min=0)] = 0
        return pnp_refine(pts, model, mask, err, K, thr, aggregation, rounds, max_steps)


# ------------------------------------------------------------------------------------------------------
# RANSAC homography (csrc/sfm_homography.hip): corr [B,N,4] = {xa, ya, xb, yb}, S [B,H,8] (first 4 entries used),
# H [B,H,9] row-major with x_b ~ H x_a, ||H||_F = 1, det H >= 0
# ------------------------------------------------------------------------------------------------------
def homography_fit(corr: torch.Tensor, S: torch.Tensor):
    """Four-point DLT fit of every hypothesis -> H [B,H,9], flags [B,H] (SFM_FIT_DEGENERATE)."""
    return ops.load().homography_fit(corr, S)


def homography_score(corr: torch.Tensor, H: torch.Tensor, S: torch.Tensor, thr: float):
    """Per hypothesis (extra-inlier count, sum e, sum e^2) of the symmetric transfer error e; the first four entries of each
    row of S are the sample.  Selection: ``select_best`` with ``sample_size=4``."""
    return ops.load().homography_score(corr, H, S, float(thr))


def homography_inlier_mask(corr: torch.Tensor, H: torch.Tensor, S: torch.Tensor, result: torch.Tensor, thr: float):
    """uint8 [B,N]: 2 sample item of the winner (the first four entries of its row of S), 1 other inlier, 0 outlier."""
    return ops.load().homography_inlier_mask(corr, H, S, result, float(thr))


class HomographyWorkspace(_PassWorkspace):
    """Pre-allocated device buffers of a homography pass for B pairs x H hypotheses x N correspondences."""

    def __init__(self, batch: int, n: int, h: int, device=None):
        super().__init__(batch, n, h, 9, solver_sample_size("homography", "homography"), device)
        self.H = self.model

    def run(self, corr: torch.Tensor, thr: float, min_extra: float, aggregation: int, with_mask: bool = True, philox=None) -> None:
        """fit + score + select (+ mask) in one call (``sfm_homography_ransac_pass``) for the sample table in ``self.S`` — or,
        with ``philox=(seed, h_begin, seed_stride)``, for Philox samples drawn inside the fit launch (which also fills ``self.S``)."""
        seed, h_begin, stride = (0, 0, 1) if philox is None else philox
        ops.load().homography_ransac_pass_(corr, _as_int64(seed), _as_int64(stride), philox is not None, h_begin, float(thr),
                                           float(min_extra), int(aggregation), self.S, self.H, self.flags, self.cnt, self.s1,
                                           self.s2, self.result, self.mask if with_mask else None)


# ------------------------------------------------------------------------------------------------------
# RANSAC similarity alignment of two reconstructions (csrc/sfm_similarity.hip): pairs [B,N,6] =
# {ax, ay, az, bx, by, bz}, S [B,H,8] (first 3 entries used), model [B,H,13] = R (row-major) | t | s with b ~ s R a + t
# ------------------------------------------------------------------------------------------------------
SIMILARITY_SAMPLE, SIMILARITY_MODEL = 3, 13


def model_similarity(row: np.ndarray) -> Tuple[float, np.ndarray, np.ndarray]:
    """A 13-entry model row R (9) | t (3) | s as (s, fresh (3,3), fresh (3,))."""
    return float(row[12]), row[:9].reshape(3, 3).copy(), row[9:12].copy()


def fit_similarity(pairs: torch.Tensor, mask: Optional[torch.Tensor] = None, out=None):
    """The least-squares model of the items with a non-zero mask (``mask=None``: of all items), one per entry
    (``sfm_similarity_fit_masked``).  pairs [B,N,6], mask uint8 [B,N] -> (model [B,13], flags int32 [B], SFM_FIT_DEGENERATE
    where the set does not determine a model).  ``out=(model, flags)``: the caller's buffers.  No host synchronisation."""
    if out is None:
        return ops.load().similarity_fit(pairs, mask)
    ops.load().similarity_fit_(pairs, mask, out[0], out[1])
    return out


def similarity_refine(pairs, model, mask, err, thr: float, aggregation: int, rounds: int = 2, out=None):
    """Closed-form refit of one model per entry on its inliers, re-scored and kept only if better (``sfm_similarity_refine``).
    pairs [B,N,6], model f64 [B,13], mask uint8 [B,N] (non-zero = inlier), err f64 [B] (the aggregated error of ``model``) ->
    (model_out [B,13], mask_out uint8 [B,N] (1 = inlier), info int64 [B,3] viewing sfm_similarity_refine_info records;
    ``read_similarity_refine_info``).  ``out``: the caller's three buffers.  No host synchronisation."""
    if out is None:
        return ops.load().similarity_refine(pairs, model.contiguous(), mask.contiguous(), err.contiguous(), float(thr),
                                            int(aggregation), int(rounds))
    ops.load().similarity_refine_(pairs, model.contiguous(), mask.contiguous(), err.contiguous(), float(thr), int(aggregation),
                                  int(rounds), out[0], out[1], out[2])
    return out


@dataclass
class SimilarityRefineInfo:
    error: float      # aggregated error of the model left in model_out, over its `count` inliers
    count: int        # inliers of that model
    accepted: int     # rounds whose result was kept (0: model_out is the input model)
    rounds_run: int   # rounds that fitted a model (entered with at least three inliers)


def read_similarity_refine_info(info: torch.Tensor) -> List[SimilarityRefineInfo]:
    """Host copy of sfm_similarity_refine_info records (int64 [B,3]) (synchronises)."""
    return [SimilarityRefineInfo(*fields) for fields in _read_records(info, 1, 3)]


class SimilarityWorkspace(_PassWorkspace):
    """Pre-allocated device buffers of a similarity pass for B entries x H hypotheses x N 3-D / 3-D pairs (as RansacWorkspace),
    and those of the refinement behind it."""

    def __init__(self, batch: int, n: int, h: int, device=None):
        super().__init__(batch, n, h, SIMILARITY_MODEL, SIMILARITY_SAMPLE, device)
        dev = self.S.device
        self.model_out = torch.empty((batch, SIMILARITY_MODEL), dtype=F64, device=dev)
        self.mask_out = torch.empty((batch, n), dtype=torch.uint8, device=dev)
        self.info = torch.empty((batch, 3), dtype=torch.int64, device=dev)

    def buffers(self):
        """Every output buffer, in the order a test names them."""
        return (self.S, self.model, self.flags, self.cnt, self.s1, self.s2, self.result, self.mask, self.model_out, self.mask_out,
                self.info)

    def run(self, pairs: torch.Tensor, thr: float, min_extra: float, aggregation: int, with_mask: bool = True, philox=None) -> None:
        """fit + score + select (+ mask) in one call (``sfm_similarity_ransac_pass``) for the sample table in ``self.S`` — or,
        with ``philox=(seed, h_begin, seed_stride)``, for Philox samples drawn inside the fit launch (which also fills ``self.S``)."""
        seed, h_begin, stride = (0, 0, 1) if philox is None else philox
        ops.load().similarity_ransac_pass_(pairs, _as_int64(seed), _as_int64(stride), philox is not None, h_begin, float(thr),
                                           float(min_extra), int(aggregation), self.S, self.model, self.flags, self.cnt, self.s1,
                                           self.s2, self.result, self.mask if with_mask else None)

    def refine(self, pairs: torch.Tensor, thr: float, aggregation: int, rounds: int = 2):
        """``similarity_refine`` of every entry's winner, chained on this pass's buffers: model[b, best_h] (row 0 when an entry
        has no winner: its mask is all zero and it keeps that row), the pass's mask and the record's best_err.  Stream-ordered
        after ``run``: no host round trip.  -> (model_out [B,13], mask_out [B,N], info [B,3]), this workspace's buffers."""
        rows = torch.arange(self.batch, device=self.result.device)
        model = self.model[rows, self.result[:, 1].clamp(min=0)]
        err = self.result[:, 2].contiguous().view(F64)
        return similarity_refine(pairs, model, self.mask, err, thr, aggregation, rounds, out=(self.model_out, self.mask_out, self.info))


# ------------------------------------------------------------------------------------------------------
# Two-view verification of every pair of a match graph in one call (csrc/sfm_view_graph.hip): corr [N,4], the
# pairs' K-normalised correspondences concatenated; offset int64 [Q+1]; per pair the homography pass and the five-point pass
# ------------------------------------------------------------------------------------------------------
PAIR_NONE, PAIR_ESSENTIAL, PAIR_HOMOGRAPHY, PAIR_BAD_OFFSETS = range(4)
PAIR_KINDS = _native.PAIR_KINDS
VERDICT_BYTES = C.sizeof(_native.PairVerdict)
POSE_OK, POSE_NO_MODEL, POSE_NOT_ESSENTIAL, POSE_NO_VOTE, POSE_BAD_OFFSETS = range(5)
POSE_STATUS = _native.POSE_STATUS
POSE_BYTES = C.sizeof(_native.PairPose)
# sfm_pair_pose as a NumPy record: one row of the pose table of ``ViewGraphWorkspace.poses``
POSE_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("median_angle", "<f8"), ("votes", "<i4", (4,)), ("best", "<i4"),
                       ("status", "<i4")])

PAIR_REFINE_OK, PAIR_REFINE_NO_POSE, PAIR_REFINE_TOO_FEW = range(3)
PAIR_REFINE_STATUS = _native.PAIR_REFINE_STATUS
PAIR_REFINE_INFO_BYTES = C.sizeof(_native.PairRefineInfo)
# sfm_pair_refine_info as a NumPy record: one row of the info table of ``refine_pair_poses``
PAIR_REFINE_INFO_DTYPE = np.dtype([("start_error", "<f8"), ("error", "<f8"), ("start_count", "<i4"), ("count", "<i4"),
                                   ("accepted", "<i4"), ("lm_steps", "<i4"), ("status", "<i4"), ("reserved", "<i4")])


def refine_pair_poses(corr: torch.Tensor, offset: torch.Tensor, pose: torch.Tensor, thr: float, aggregation: int,
                      rounds: int = 2, max_steps: int = 20):
    """Refine every pair's relative pose on its inliers (``sfm_refine_pair_poses``): corr f64 [N,4], offset
    int64 [Q+1], pose uint8 [Q,128] as ``pair_poses`` left it.  Returns (pose_out uint8 [Q,128], mask uint8 [N]: 1 = within
    ``thr`` under the kept pose, info int64 [Q,5] viewing the sfm_pair_refine_info records; ``read_pair_refine_info``).  No
    host synchronisation."""
    return ops.load().refine_pair_poses(corr, offset, pose, float(thr), int(aggregation), int(rounds), int(max_steps))


def read_pair_refine_info(info: torch.Tensor) -> np.ndarray:
    """Host copy of sfm_pair_refine_info records (int64 [Q,5]) as a (Q,) array of ``PAIR_REFINE_INFO_DTYPE`` (synchronises)."""
    return info.cpu().numpy().reshape(-1).view(PAIR_REFINE_INFO_DTYPE).copy()



@dataclass
class ViewGraphOutcome:
    """What a ``ViewGraphWorkspace`` holds after a call, on the host: one row per pair."""
    kind: np.ndarray               # (Q,) int32, PAIR_*
    homography_count: np.ndarray   # (Q,) int32: the winner's sample size plus its extra inliers, 0 without a winner
    essential_count: np.ndarray    # (Q,) int32
    ratio: np.ndarray              # (Q,) homography_count / essential_count, inf when the latter is 0
    H: np.ndarray                  # (Q, 3, 3), NaN where there is no homography
    E: np.ndarray                  # (Q, 3, 3), NaN where there is no essential matrix
    homography_best: np.ndarray    # (Q,) int64 winning hypothesis of the pair, -1 if none
    essential_best: np.ndarray     # (Q,) int64
    homography_sample: np.ndarray  # (Q, 4) int64 items of the winner's sample (local to the pair), -1 without a winner
    essential_sample: np.ndarray   # (Q, 6) int64
    homography_mask: np.ndarray    # (N,) uint8: 2 sample item of its pair's winner, 1 other inlier, 0 otherwise
    essential_mask: np.ndarray     # (N,) uint8
    # after ``poses``, else None
    pose_R: Optional[np.ndarray] = None             # (Q, 3, 3) x_b ~ R x_a + t, NaN unless pose_status is POSE_OK
    pose_t: Optional[np.ndarray] = None             # (Q, 3) unit length
    pose_votes: Optional[np.ndarray] = None         # (Q, 4) int32 passing inliers per candidate
    pose_best: Optional[np.ndarray] = None          # (Q,) int32 first maximum of the votes, -1 if all are zero
    pose_median_angle: Optional[np.ndarray] = None  # (Q,) radians, NaN unless pose_status is POSE_OK
    pose_status: Optional[np.ndarray] = None        # (Q,) int32, POSE_*
    # after ``refine_poses``, else None; pose_R and pose_t are then the refined ones
    refine_start_error: Optional[np.ndarray] = None  # (Q,) aggregated error of the start pose over its start set, NaN without a pose
    refine_error: Optional[np.ndarray] = None        # (Q,) the same of the kept pose over its inliers
    refine_start_count: Optional[np.ndarray] = None  # (Q,) int32 items within the threshold under the start pose
    refine_count: Optional[np.ndarray] = None        # (Q,) int32 the same under the kept pose
    refine_accepted: Optional[np.ndarray] = None     # (Q,) int32 rounds whose result was kept
    refine_lm_steps: Optional[np.ndarray] = None     # (Q,) int32 LM trial steps over all rounds
    refine_status: Optional[np.ndarray] = None       # (Q,) int32, PAIR_REFINE_*
    refine_mask: Optional[np.ndarray] = None         # (N,) uint8: 1 = within the threshold under its pair's kept pose


class ViewGraphWorkspace:
    """Pre-allocated device buffers of ``sfm_verify_pairs`` for Q pairs x H hypotheses over N items in all (about 224 bytes
    per pair-hypothesis), and the decoding of what a call leaves in them."""

    def __init__(self, pairs: int, n_total: int, h: int, device=None):
        dev = device or require_gpu()
        self.pairs, self.n_total, self.h = pairs, n_total, h
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=F64, device=dev)
        self.S = torch.empty((pairs, h, 8), **i32)
        self.H = torch.empty((pairs, h, 9), **f64)
        self.E = torch.empty((pairs, h, 9), **f64)
        self.h_flags, self.h_cnt = torch.empty((pairs, h), **i32), torch.empty((pairs, h), **i32)
        self.h_s1, self.h_s2 = torch.empty((pairs, h), **f64), torch.empty((pairs, h), **f64)
        self.e_flags, self.e_cnt = torch.empty((pairs, h), **i32), torch.empty((pairs, h), **i32)
        self.e_s1, self.e_s2 = torch.empty((pairs, h), **f64), torch.empty((pairs, h), **f64)
        self.h_result = torch.empty((pairs, SELECT_BYTES // 8), dtype=torch.int64, device=dev)
        self.e_result = torch.empty((pairs, SELECT_BYTES // 8), dtype=torch.int64, device=dev)
        self.h_mask = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.e_mask = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.verdict = torch.empty((pairs, VERDICT_BYTES // 8), dtype=torch.int64, device=dev)
        self.pose = self.angle = self._corr = self._offset = None   # set by run / poses
        self.refine_mask = self.refine_info = None                  # set by refine_poses

    def buffers(self):
        """The output tensors in the order of the ``verify_pairs_`` op."""
        return (self.S, self.H, self.E, self.h_flags, self.h_cnt, self.h_s1, self.h_s2, self.e_flags, self.e_cnt, self.e_s1,
                self.e_s2, self.h_result, self.e_result, self.h_mask, self.e_mask, self.verdict)

    def run(self, corr: torch.Tensor, offset: torch.Tensor, min_extra: torch.Tensor, thr: float, aggregation: int,
            max_ratio: float, seed: int, seed_stride: int = 1, h_begin: int = 0) -> None:
        """One ``sfm_verify_pairs`` call (the ``verify_pairs_`` op), enqueue-only: corr f64 [N,4], offset int64 [Q+1],
        min_extra f64 [Q] on the device; pair q draws its Philox samples with ``seed + q * seed_stride``."""
        ops.load().verify_pairs_(corr, offset, min_extra, _as_int64(seed), _as_int64(seed_stride), int(h_begin), float(thr),
                                 int(aggregation), float(max_ratio), *self.buffers())
        self._corr, self._offset, self.pose, self.angle = corr, offset, None, None
        self.refine_mask = self.refine_info = None

    def poses(self, distance_threshold: float = 50.0) -> None:
        """One ``sfm_pair_poses`` call (the ``pair_poses`` op) on what ``run`` took and left, enqueue-only: ``pose`` uint8
        [Q,128] (``sfm_pair_pose`` records) and ``angle`` f64 [N], each item's angle under its pair's best pose, NaN off the
        passing inliers."""
        if self._corr is None:
            raise RuntimeError("ViewGraphWorkspace.poses: call run first")
        if self.h < 1:
            raise ValueError("ViewGraphWorkspace.poses needs at least one hypothesis per pair")
        self.pose, self.angle = ops.load().pair_poses(self._corr, self._offset, self.E, self.e_result, self.e_mask, self.verdict,
                                                       float(distance_threshold))
        self.refine_mask = self.refine_info = None

    def refine_poses(self, thr: float, aggregation: int, rounds: int = 2, max_steps: int = 20) -> None:
        """One ``sfm_refine_pair_poses`` call (the ``refine_pair_poses`` op) on what ``run`` took and ``poses`` left,
        enqueue-only: ``pose`` becomes the refined table (R and t replaced where a round was kept, the rest carried over),
        ``refine_mask`` uint8 [N] and ``refine_info`` int64 [Q,5] (``sfm_pair_refine_info`` records)."""
        if self.pose is None:
            raise RuntimeError("ViewGraphWorkspace.refine_poses: call run and poses first")
        self.pose, self.refine_mask, self.refine_info = refine_pair_poses(self._corr, self._offset, self.pose, thr, aggregation,
                                                                          rounds, max_steps)

    def read_poses(self) -> np.ndarray:
        """The pose table on the host as a (Q,) array of ``POSE_DTYPE`` records (synchronises)."""
        return self.pose.cpu().numpy().reshape(-1).view(POSE_DTYPE).copy()

    def read_verdicts(self) -> List["_native.PairVerdict"]:
        """Copy the verdict records to the host (synchronises)."""
        raw = self.verdict.cpu().numpy().tobytes()
        return [_native.PairVerdict.from_buffer_copy(raw[i * VERDICT_BYTES:(i + 1) * VERDICT_BYTES]) for i in range(self.pairs)]

    def outcome(self) -> ViewGraphOutcome:
        """Verdicts, winners and masks on the host (synchronises); the winners' rows are gathered on the device first."""
        Q = self.pairs
        verdicts = self.read_verdicts()
        rows = torch.arange(Q, device=self.S.device)
        out = {}
        for name, result, model, size in (("homography", self.h_result, self.H, 4), ("essential", self.e_result, self.E, 6)):
            best = result[:, 1]
            if self.h:
                at = best.clamp(min=0)
                m = model[rows, at].cpu().numpy().reshape(Q, 3, 3).copy()
                smp = self.S[rows, at, :size].cpu().numpy().astype(np.int64)
            else:
                m, smp = np.empty((Q, 3, 3)), np.empty((Q, size), dtype=np.int64)
            best = best.cpu().numpy()
            m[best < 0] = np.nan
            smp[best < 0] = -1
            out[name] = (m, best, smp)
        return ViewGraphOutcome(
            kind=np.array([v.kind for v in verdicts], dtype=np.int32),
            homography_count=np.array([v.homography_count for v in verdicts], dtype=np.int32),
            essential_count=np.array([v.essential_count for v in verdicts], dtype=np.int32),
            ratio=np.array([v.ratio for v in verdicts], dtype=np.float64),
            H=out["homography"][0], E=out["essential"][0],
            homography_best=out["homography"][1], essential_best=out["essential"][1],
            homography_sample=out["homography"][2], essential_sample=out["essential"][2],
            homography_mask=checked_mask(self.h_mask.cpu().numpy().copy()),
            essential_mask=checked_mask(self.e_mask.cpu().numpy().copy()), **self._pose_fields())

    def _pose_fields(self) -> dict:
        if self.pose is None:
            return {}
        table = self.read_poses()
        fields = dict(pose_R=table["R"].copy(), pose_t=table["t"].copy(), pose_votes=table["votes"].copy(),
                      pose_best=table["best"].copy(), pose_median_angle=table["median_angle"].copy(),
                      pose_status=table["status"].copy())
        if self.refine_info is not None:
            info = read_pair_refine_info(self.refine_info)
            fields.update({"refine_" + k: info[k].copy() for k in ("start_error", "error", "start_count", "count", "accepted",
                                                                   "lm_steps", "status")})
            fields["refine_mask"] = self.refine_mask.cpu().numpy().copy()
        return fields


# ------------------------------------------------------------------------------------------------------
# Absolute pose of every candidate view in one call (csrc/sfm_register_views.hip): pts [N,5], the views'
# 2D-3D items concatenated; offset int64 [V+1]; per view the P3P pass and the refinement of its winner
# ------------------------------------------------------------------------------------------------------
REGISTER_OK, REGISTER_NO_MODEL, REGISTER_TOO_FEW, REGISTER_BAD_OFFSETS = range(4)
REGISTER_STATUS = _native.REGISTER_STATUS


def read_register_status(status: torch.Tensor) -> np.ndarray:
    """Host copy of the statuses of a ``sfm_register_views`` call (int32 [V], REGISTER_*) (synchronises)."""
    return status.cpu().numpy().astype(np.int32)


class RegisterViewsWorkspace:
    """Pre-allocated device buffers of ``sfm_register_views`` for V views x H hypotheses over N items in all (about 152 bytes
    per view-hypothesis).  ``run`` fills them; nothing is read back until the caller asks."""

    def __init__(self, views: int, n_total: int, h: int, device=None):
        dev = device or require_gpu()
        self.views, self.n_total, self.h = views, n_total, h
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=F64, device=dev)
        self.S = torch.empty((views, h, 8), **i32)
        self.model = torch.empty((views, h, 12), **f64)
        self.flags, self.cnt = torch.empty((views, h), **i32), torch.empty((views, h), **i32)
        self.s1, self.s2 = torch.empty((views, h), **f64), torch.empty((views, h), **f64)
        self.result = torch.empty((views, SELECT_BYTES // 8), dtype=torch.int64, device=dev)
        self.mask = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.pose_out = torch.empty((views, 12), **f64)
        self.mask_out = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.info = torch.empty((views, 3), dtype=torch.int64, device=dev)
        self.status = torch.empty((views,), **i32)

    def buffers(self):
        """The output tensors in the order of the ``register_views_`` op."""
        return (self.S, self.model, self.flags, self.cnt, self.s1, self.s2, self.result, self.mask, self.pose_out, self.mask_out,
                self.info, self.status)

    def run(self, pts: torch.Tensor, offset: torch.Tensor, min_extra: torch.Tensor, K, thr: float, aggregation: int, seed: int,
            seed_stride: int = 1, h_begin: int = 0, refine_rounds: int = 2, refine_max_steps: int = 20) -> None:
        """One ``sfm_register_views`` call (the ``register_views_`` op), enqueue-only: pts f64 [N,5], offset int64 [V+1],
        min_extra f64 [V] on the device; view v draws its Philox samples with ``seed + v * seed_stride``."""
        ops.load().register_views_(pts, offset, min_extra, _camera_list(K), _as_int64(seed), _as_int64(seed_stride), int(h_begin),
                                   float(thr), int(aggregation), int(refine_rounds), int(refine_max_steps), *self.buffers())


# ------------------------------------------------------------------------------------------------------
# Similarity alignment of every pair of sub-models in one call (csrc/sfm_align_models.hip): pairs [N,6], the
# sub-model pairs' 3-D / 3-D items concatenated; offset int64 [Q+1]; per pair the similarity pass and the refinement of its winner
# ------------------------------------------------------------------------------------------------------
ALIGN_OK, ALIGN_NO_MODEL, ALIGN_TOO_FEW, ALIGN_BAD_OFFSETS = range(4)
ALIGN_STATUS = _native.ALIGN_STATUS


def read_align_status(status: torch.Tensor) -> np.ndarray:
    """Host copy of the statuses of a ``sfm_align_models`` call (int32 [Q], ALIGN_*) (synchronises)."""
    return status.cpu().numpy().astype(np.int32)


class AlignModelsWorkspace:
    """Pre-allocated device buffers of ``sfm_align_models`` for Q pairs x H hypotheses over N items in all, none of the pairs
    with more than ``max_items`` (about 160 bytes per pair-hypothesis).  ``run`` fills them; nothing is read back until the
    caller asks."""

    def __init__(self, pairs: int, n_total: int, h: int, max_items: int, device=None):
        dev = device or require_gpu()
        self.pairs, self.n_total, self.h, self.max_items = pairs, n_total, h, max_items
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=F64, device=dev)
        self.S = torch.empty((pairs, h, 8), **i32)
        self.model = torch.empty((pairs, h, SIMILARITY_MODEL), **f64)
        self.flags, self.cnt = torch.empty((pairs, h), **i32), torch.empty((pairs, h), **i32)
        self.s1, self.s2 = torch.empty((pairs, h), **f64), torch.empty((pairs, h), **f64)
        self.result = torch.empty((pairs, SELECT_BYTES // 8), dtype=torch.int64, device=dev)
        self.mask = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.model_out = torch.empty((pairs, SIMILARITY_MODEL), **f64)
        self.mask_out = torch.empty((n_total,), dtype=torch.uint8, device=dev)
        self.info = torch.empty((pairs, 3), dtype=torch.int64, device=dev)
        self.status = torch.empty((pairs,), **i32)

    def buffers(self):
        """The output tensors in the order of the ``align_models_`` op."""
        return (self.S, self.model, self.flags, self.cnt, self.s1, self.s2, self.result, self.mask, self.model_out, self.mask_out,
                self.info, self.status)

    def run(self, pairs: torch.Tensor, offset: torch.Tensor, thr: torch.Tensor, min_extra: torch.Tensor, aggregation: int,
            seed: int, seed_stride: int = 1, h_begin: int = 0, refine_rounds: int = 2) -> None:
        """One ``sfm_align_models`` call (the ``align_models_`` op), enqueue-only: pairs f64 [N,6], offset int64 [Q+1], thr and
        min_extra f64 [Q] on the device; pair q draws its Philox samples with ``seed + q * seed_stride``."""
        ops.load().align_models_(pairs, offset, thr, min_extra, int(self.max_items), _as_int64(seed), _as_int64(seed_stride),
                                 int(h_begin), int(aggregation), int(refine_rounds), *self.buffers())


# ------------------------------------------------------------------------------------------------------
# Plane-sweep depth maps and their consistency filter (csrc/sfm_plane_sweep.hip): images uint8 [V,H,W], K [9] and
# poses [V,12] on the device; per reference view a source list int32 [S] and a depth list [D]
# ------------------------------------------------------------------------------------------------------
SWEEP_OK, SWEEP_BAD_REFERENCE = range(2)
SWEEP_STATUS = _native.SWEEP_STATUS


def read_sweep_status(status: torch.Tensor) -> np.ndarray:
    """Host copy of the statuses of a ``sfm_plane_sweep`` or ``sfm_filter_depth_maps`` call (int32 [R], SWEEP_*) (synchronises)."""
    return status.cpu().numpy().astype(np.int32)


class PlaneSweepWorkspace:
    """Pre-allocated device buffers of ``sfm_plane_sweep`` for R reference views of H x W pixels and D depth hypotheses each
    (20 bytes per pixel, and 8 D more with the cost volume).  ``run`` fills them; nothing is read back until the caller asks."""

    def __init__(self, refs: int, height: int, width: int, depths: int, device=None, volume: bool = False):
        dev = device or require_gpu()
        self.refs, self.height, self.width, self.depths = refs, height, width, depths
        self.depth = torch.empty((refs, height, width), dtype=F64, device=dev)
        self.index = torch.empty((refs, height, width), dtype=torch.int32, device=dev)
        self.cost = torch.empty((refs, height, width), dtype=F64, device=dev)
        self.status = torch.empty((refs,), dtype=torch.int32, device=dev)
        self.volume = torch.empty((refs, depths, height, width), dtype=F64, device=dev) if volume else None

    def buffers(self):
        """The output tensors in the order of the ``plane_sweep_`` op (``volume`` may be None)."""
        return (self.depth, self.index, self.cost, self.status, self.volume)

    def run(self, images: torch.Tensor, K: torch.Tensor, poses: torch.Tensor, refs: torch.Tensor, sources: torch.Tensor,
            depths: torch.Tensor, radius: int = 3, top_k: int = 0, min_sources: int = 1, min_variance: float = 1.0) -> None:
        """One ``sfm_plane_sweep`` call (the ``plane_sweep_`` op), enqueue-only: images uint8 [V,H,W], K f64 [9], poses f64
        [V,12], refs int32 [R], sources int32 [R,S], depths f64 [R,D] on the device."""
        ops.load().plane_sweep_(images, K, poses, refs, sources, depths, int(radius), int(top_k), int(min_sources), float(min_variance),
                                *self.buffers())


def filter_depth_maps(depth: torch.Tensor, K: torch.Tensor, poses: torch.Tensor, refs: torch.Tensor, sources: torch.Tensor,
                      max_pixel_error: float = 1.0, max_relative_depth_error: float = 0.01, min_consistent: int = 2, out=None):
    """One ``sfm_filter_depth_maps`` call, enqueue-only: depth f64 [V,H,W] (NaN = none) -> (count int32 [R,H,W], filtered f64
    [R,H,W], points f64 [R,H,W,3], status int32 [R]); ``out``: the caller's four buffers."""
    op = ops.load()
    if out is None:
        return op.filter_depth_maps(depth, K, poses, refs, sources, float(max_pixel_error), float(max_relative_depth_error),
                                    int(min_consistent))
    op.filter_depth_maps_(depth, K, poses, refs, sources, float(max_pixel_error), float(max_relative_depth_error), int(min_consistent),
                          *out)
    return out


# ------------------------------------------------------------------------------------------------------
# Semi-global smoothing of the plane-sweep cost volume (csrc/sfm_sgm.hip): volume f64 [R,D,H,W] and depths f64 [R,D]
# on the device, as ``sfm_plane_sweep`` writes and reads them
# ------------------------------------------------------------------------------------------------------
class SgmWorkspace:
    """Pre-allocated device buffers of ``sfm_sgm_aggregate`` for R reference views of H x W pixels and D depth hypotheses each
    (20 bytes per pixel, and 8 D more with the aggregated volume; without it the call takes as much from the caching allocator
    for the time it runs).  ``run`` fills them; nothing is read back until the caller asks."""

    def __init__(self, refs: int, height: int, width: int, depths: int, device=None, aggregated: bool = False):
        dev = device or require_gpu()
        self.refs, self.height, self.width, self.depths = refs, height, width, depths
        self.depth = torch.empty((refs, height, width), dtype=F64, device=dev)
        self.index = torch.empty((refs, height, width), dtype=torch.int32, device=dev)
        self.cost = torch.empty((refs, height, width), dtype=F64, device=dev)
        self.aggregated = torch.empty((refs, depths, height, width), dtype=F64, device=dev) if aggregated else None

    def buffers(self):
        """The output tensors in the order of the ``sgm_aggregate_`` op (``aggregated`` may be None)."""
        return (self.depth, self.index, self.cost, self.aggregated)

    def run(self, volume: torch.Tensor, depths: torch.Tensor, p1: float = 0.1, p2: float = 0.8, invalid_cost: float = 1.0,
            paths: int = 8) -> None:
        """One ``sfm_sgm_aggregate`` call (the ``sgm_aggregate_`` op), enqueue-only: volume f64 [R,D,H,W], depths f64 [R,D]."""
        ops.load().sgm_aggregate_(volume, depths, float(p1), float(p2), float(invalid_cost), int(paths), *self.buffers())


def sgm_aggregate(volume: torch.Tensor, depths: torch.Tensor, p1: float = 0.1, p2: float = 0.8, invalid_cost: float = 1.0,
                  paths: int = 8, aggregated: bool = False, workspace: Optional[SgmWorkspace] = None) -> SgmWorkspace:
    """One ``sfm_sgm_aggregate`` call, enqueue-only -> the ``SgmWorkspace`` that holds its results (``workspace``, or a new one of
    the volume's shape)."""
    R, D, H, W = volume.shape
    ws = workspace or SgmWorkspace(R, H, W, D, volume.device, aggregated=aggregated)
    ws.run(volume, depths, p1, p2, invalid_cost, paths)
    return ws


# ------------------------------------------------------------------------------------------------------
# Fusion of depth maps into a TSDF volume and its mesh (csrc/sfm_tsdf.hip): the state sum f64 [nz,ny,nx], count
# int32 [nz,ny,nx] and grey_sum int32 [nz,ny,nx] or None on the device; origin a triple of floats
# ------------------------------------------------------------------------------------------------------
TSDF_OK, TSDF_BAD_VIEW = range(2)
TSDF_STATUS = _native.TSDF_STATUS


def read_tsdf_status(status: torch.Tensor) -> np.ndarray:
    """Host copy of the statuses of a ``sfm_tsdf_integrate`` call (int32 [N], TSDF_*) (synchronises)."""
    return status.cpu().numpy().astype(np.int32)


def tsdf_integrate(state, depth: torch.Tensor, images, K: torch.Tensor, poses: torch.Tensor, views: torch.Tensor, origin,
                   voxel_size: float, truncation: float, status=None):
    """One ``sfm_tsdf_integrate`` call, enqueue-only.  ``state``: (sum, count, grey_sum or None); depth f64 [V,H,W], images uint8
    [V,H,W] or None (None exactly when grey_sum is), K f64 [9], poses f64 [V,12], views int32 [N].  Without ``status`` the state
    is left as it is and -> (sum, count, grey_sum or None, status), new tensors; with ``status`` (int32 [N]) the state is
    updated in place and ``status`` filled."""
    op = ops.load()
    total, count, grey_sum = state
    scalars = (float(origin[0]), float(origin[1]), float(origin[2]), float(voxel_size), float(truncation))
    if status is None:
        total, count, grey, status = op.tsdf_integrate(total, count, grey_sum, depth, images, K, poses, views, *scalars)
        return total, count, (None if grey_sum is None else grey), status
    op.tsdf_integrate_(total, count, grey_sum, depth, images, K, poses, views, *scalars, status)
    return total, count, grey_sum, status


def tsdf_extract_mesh(state, origin, voxel_size: float, min_count: int = 1, max_triangles: int = 0, out=None):
    """One ``sfm_tsdf_extract_mesh`` call, enqueue-only: -> (vertices f64 [max_triangles,3,3], grey f64 [max_triangles,3] or None,
    total int64 [1]); ``out``: the caller's three buffers (grey None without a grey_sum), whose row count is max_triangles."""
    op = ops.load()
    total, count, grey_sum = state
    scalars = (float(origin[0]), float(origin[1]), float(origin[2]), float(voxel_size), int(min_count))
    if out is None:
        vertices, grey, found = op.tsdf_extract_mesh(total, count, grey_sum, *scalars, int(max_triangles))
        return vertices, (None if grey_sum is None else grey), found
    op.tsdf_extract_mesh_(total, count, grey_sum, *scalars, *out)
    return out
