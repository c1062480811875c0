"""The C ABI of the matchers without a GPU: every refusal of sfm_patch_extract, sfm_pair_scores, sfm_match_summary,
sfm_match_row_summary and sfm_hamming_summary with its status and message, the order in which they fire where two apply, the
two workspace formulas, and the calls that return SFM_OK without touching anything.  A refused call enqueues nothing, so
host memory stands in for every device pointer."""
import ctypes as C

import pytest

EINVAL = -1   # SFM_EINVAL of include/sfm_hip.h
NCC, SSD, U8, I8, I32 = 0, 1, 0x100 | 8, 0x100 | 0x80 | 8, 0x100 | 0x80 | 32
TOO_LARGE = b"size exceeds what one launch covers"


@pytest.fixture(scope="module")
def abi(native_lib):
    from structure_from_motion_amd import _native

    lib = _native.load()
    buf = (C.c_int64 * 64)()   # never read or written: every call below returns before its first launch
    base = C.addressof(buf)
    base += (-base) % 16

    def refused(status, message):
        return status == EINVAL and message in lib.sfm_last_error()

    refused.keep = buf
    return lib, base, refused


def _refusals(call, defaults, refused, prefix, cases):
    """Each case (changed arguments, piece of the message): the call with the defaults otherwise is refused with it."""
    for changed, message in cases:
        assert set(changed) <= set(defaults), changed
        args = dict(defaults, **changed)
        assert refused(call(*args.values()), prefix + message), (changed, message)


def test_patch_extract_refusals(abi):
    lib, base, refused = abi
    d = C.c_void_p(base)
    defaults = dict(image=d, height=48, width=64, feats=d, n=5, window_size=5, mode=0, stride=128, patches=d, ssq=d, ok=d,
                    stream=None)
    cases = [({"n": -1}, b"bad size"), ({"height": 0}, b"bad size"), ({"height": -3}, b"bad size"), ({"width": 0}, b"bad size"),
             ({"window_size": 0}, b"bad size"), ({"window_size": -5}, b"bad size"),
             ({"mode": 3}, b"unknown patch mode"), ({"mode": -1}, b"unknown patch mode"),
             ({"mode": 3, "n": 0}, b"unknown patch mode"),                      # the mode is judged before n == 0 returns
             ({"stride": 4}, b"stride < n"), ({"stride": -128}, b"stride < n"),
             ({"stride": 4, "image": None}, b"stride < n"),                     # ... and the stride before the pointers
             ({"n": 2**32, "stride": 2**32}, TOO_LARGE)]
    cases += [({name: None}, b"null pointer") for name in ("image", "feats", "patches", "ssq", "ok")]
    _refusals(lib.sfm_patch_extract, defaults, refused, b"sfm_patch_extract: ", cases)
    for mode in (0, 1, 2):   # no features: nothing to do, nothing touched
        assert lib.sfm_patch_extract(None, 48, 64, None, 0, 5, mode, 0, None, None, None, None) == 0


PAIR_NAMES = ("patches_a", "patches_b", "ssq_a", "ssq_b", "ok_a", "ok_b")
UNKNOWN_METRICS = (2, -1, 0x100 | 24, 0x100, 0x100 | 0x80, 0x100 | 0x80 | 24, 0x200 | 8, 0x100 | 12)


def _pair_defaults(base, **tail):
    d = C.c_void_p(base)
    return dict(metric=NCC, patches_a=d, stride_a=256, patches_b=d, stride_b=256, ssq_a=d, ssq_b=d, ok_a=d, ok_b=d, n_a=131,
                n_b=203, window_elements=49, **tail)


def test_pair_scores_refusals(abi):
    lib, base, refused = abi
    defaults = _pair_defaults(base, scores=C.c_void_p(base), stream=None)
    cases = [({"n_a": -1}, b"bad size"), ({"n_b": -1}, b"bad size"), ({"window_elements": 0}, b"bad size"),
             ({"window_elements": -49}, b"bad size"), ({"metric": 2, "n_a": -1}, b"bad size")]
    cases += [({"metric": m}, b"unknown metric") for m in UNKNOWN_METRICS]
    cases += [({"metric": 2, "n_a": 0}, b"unknown metric"), ({"metric": 0x100 | 24, "n_b": 0}, b"unknown metric"),
              ({"metric": 2, "scores": None}, b"unknown metric")]
    cases += [({name: None}, b"null pointer") for name in PAIR_NAMES + ("scores",)]
    # 65536 x 65536 tiles of 128 x 128: 2^32 blocks
    cases += [({"n_a": 128 * 65536, "n_b": 128 * 65536, "metric": m}, b"too many tiles") for m in (NCC, SSD, U8, I32)]
    cases += [({"n_a": 128 * 65536, "n_b": 128 * 65536, "scores": None}, b"null pointer")]   # the pointers come first
    _refusals(lib.sfm_pair_scores, defaults, refused, b"sfm_pair_scores: ", cases)
    for metric in (NCC, SSD, U8, I8, I32, 0x100 | 64):
        for n_a, n_b in ((0, 203), (131, 0), (0, 0)):   # an empty side: nothing to do, nothing touched, any stride
            assert lib.sfm_pair_scores(metric, None, 0, None, 0, None, None, None, None, n_a, n_b, 49, None, None) == 0


def test_match_summary_refusals(abi):
    lib, base, refused = abi
    d = C.c_void_p(base)
    ws = lib.sfm_match_summary_workspace_bytes
    assert ws(131, 203) == 32 * 131 * 2 and ws(1, 128) == 32 and ws(1, 129) == 64 and ws(20000, 20000) == 32 * 20000 * 157
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == -1 and ws(5, -1) == -1
    defaults = _pair_defaults(base, workspace=d, workspace_bytes=1 << 62, best=d, arg=d, second=d, stream=None)
    cases = [({"n_a": -1}, b"bad size"), ({"n_b": -1}, b"bad size"), ({"window_elements": 0}, b"bad size"),
             ({"metric": 2, "n_b": -1}, b"bad size")]
    cases += [({"metric": m}, b"unknown metric") for m in UNKNOWN_METRICS]
    cases += [({"metric": 2, "n_a": 0}, b"unknown metric"), ({"metric": 0x100 | 24, "n_b": 0}, b"unknown metric"),
              ({"n_b": 0}, b"empty rows"), ({"n_b": 0, "best": None}, b"empty rows"),
              ({"n_b": 2**31}, b"rows too long"), ({"n_b": 2**31, "workspace": None}, b"rows too long")]
    cases += [({name: None}, b"null pointer") for name in PAIR_NAMES + ("workspace", "best", "arg", "second")]
    cases += [({"workspace_bytes": ws(131, 203) - 1}, b"workspace smaller than"), ({"workspace_bytes": 0}, b"workspace smaller than"),
              ({"workspace_bytes": -1}, b"workspace smaller than"),
              ({"workspace_bytes": 0, "workspace": C.c_void_p(base + 8)}, b"workspace smaller than"),   # size before alignment
              ({"workspace": C.c_void_p(base + 8)}, b"workspace must be 16-byte aligned"),
              ({"workspace": C.c_void_p(base + 4)}, b"workspace must be 16-byte aligned"),
              ({"n_a": 2**32, "n_b": 1}, TOO_LARGE)]
    cases += [({"n_a": 128 * 65536, "n_b": 128 * 65536, "metric": m}, b"too many tiles") for m in (NCC, SSD, I8, I32)]
    cases += [({"n_a": 128 * 65536, "n_b": 128 * 65536, "workspace": C.c_void_p(base + 8)}, b"workspace must be 16-byte aligned")]
    _refusals(lib.sfm_match_summary, defaults, refused, b"sfm_match_summary: ", cases)
    for metric in (NCC, SSD, U8, I8, I32):
        for n_b in (203, 0):   # no rows: nothing to do, nothing touched — even with nothing to match against
            assert lib.sfm_match_summary(metric, None, 0, None, 0, None, None, None, None, 0, n_b, 49, None, 0, None, None, None,
                                         None) == 0


def test_match_row_summary_refusals(abi):
    lib, base, refused = abi
    d = C.c_void_p(base)
    defaults = dict(scores=d, n_a=131, n_b=203, best=d, arg=d, second=d, stream=None)
    cases = [({"n_a": -1}, b"negative size"), ({"n_b": -1}, b"negative size"), ({"n_b": 0}, b"empty rows"),
             ({"n_b": 0, "scores": None}, b"empty rows"), ({"n_b": 2**31}, b"rows too long"), ({"n_a": 2**26}, TOO_LARGE),
             ({"n_a": 2**26, "best": None}, b"null pointer")]
    cases += [({name: None}, b"null pointer") for name in ("scores", "best", "arg", "second")]
    _refusals(lib.sfm_match_row_summary, defaults, refused, b"sfm_match_row_summary: ", cases)
    for n_b in (203, 0):
        assert lib.sfm_match_row_summary(None, 0, n_b, None, None, None, None) == 0


def test_hamming_summary_refusals(abi):
    lib, base, refused = abi
    d, off = C.c_void_p(base), C.c_void_p(base + 8)
    ws = lib.sfm_hamming_summary_workspace_bytes
    assert ws(300, 700) == 32 * 300 * 2 and ws(1, 512) == 32 and ws(1, 513) == 64 and ws(20000, 20000) == 32 * 20000 * 40
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == -1 and ws(5, -1) == -1
    defaults = dict(desc_a=d, ok_a=d, n_a=300, desc_b=d, ok_b=d, n_b=700, workspace=d, workspace_bytes=1 << 62, best=d, arg=d,
                    second=d, stream=None)
    cases = [({"n_a": -1}, b"negative size"), ({"n_b": -1}, b"negative size"), ({"n_b": 0}, b"empty rows"),
             ({"n_b": 0, "desc_a": None}, b"empty rows"), ({"n_b": 2**31}, b"rows too long")]
    cases += [({name: None}, b"null pointer")
              for name in ("desc_a", "ok_a", "desc_b", "ok_b", "workspace", "best", "arg", "second")]
    cases += [({"workspace_bytes": ws(300, 700) - 1}, b"workspace smaller than"), ({"workspace_bytes": 0, "desc_a": off}, b"workspace smaller than"),
              ({"workspace": off}, b"workspace and descriptors must be 16-byte aligned"), ({"desc_a": off}, b"workspace and descriptors must be 16-byte aligned"),
              ({"desc_b": off}, b"workspace and descriptors must be 16-byte aligned"), ({"desc_b": C.c_void_p(base + 4)}, b"workspace and descriptors must be 16-byte aligned"),
              ({"n_a": 256 * 65536, "n_b": 512 * 65536}, b"too many tiles"),      # 65536 x 65536 tiles of 256 x 512
              ({"n_a": 256 * 65536, "n_b": 512 * 65536, "desc_a": off}, b"workspace and descriptors must be 16-byte aligned"),
              ({"n_a": 2**32, "n_b": 1}, TOO_LARGE)]
    _refusals(lib.sfm_hamming_summary, defaults, refused, b"sfm_hamming_summary: ", cases)
    for n_b in (700, 0):
        assert lib.sfm_hamming_summary(None, None, 0, None, None, n_b, None, 0, None, None, None, None) == 0
