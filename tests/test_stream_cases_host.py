"""The tables of tests/stream_cases.py against include/sfm_hip.h and ``ops``: every entry point that takes a ``stream`` has a
stream case (tests/test_gpu_streams.py) or a written exemption, the entry points whose header comment says the call
"synchronises `stream`" are exactly ``SYNCHRONISING``, and every torch op family is reached by a case.  No GPU."""
import os
import re

import stream_cases as sc
from structure_from_motion_amd import _native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sfm_hip.h")
SYNC_PHRASE = "synchronises `stream`"


def parse_header(text):
    """name -> (parameter text, the comment block that ends directly before the declaration or "") for every function the
    header declares.  A declaration that follows another one without a comment of its own has no comment."""
    out = {}
    token = re.compile(r"/\*.*?\*/|\b(?:int|int64_t|const char\*)\s+(sfm_\w+)\s*\(([^;{}]*?)\)\s*;", re.S)
    comment, comment_end = "", -1
    for m in token.finditer(text):
        if m.group(1) is None:
            comment = re.sub(r"\s*\n\s*\*\s?", " ", m.group(0))
            comment_end = m.end()
            continue
        own = comment if text[comment_end:m.start()].strip() == "" else ""
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = (" ".join(m.group(2).split()), own)
    return out


def declared():
    with open(HEADER) as f:
        return parse_header(f.read())


def with_stream(functions):
    return {name for name, (params, _) in functions.items() if re.search(r"\bvoid\*\s*stream\b", params)}


def test_the_parser_sees_the_whole_header():
    functions = declared()
    assert set(functions) == set(_native.SIGNATURES) | set(_native.OTHER_SYMBOLS)
    streamed = with_stream(functions)
    assert len(streamed) >= 65 and "sfm_verify_pairs" in streamed and "sfm_score_sed_ex" in streamed
    assert "sfm_fold_select_records_host" not in streamed and "sfm_bundle_workspace_bytes" not in streamed
    # a stream is the last parameter, or the last before the options of an _ex entry point
    for name in streamed:
        assert re.search(r"void\* stream(, const \w+\* options)?$", functions[name][0]), name


def test_every_entry_point_with_a_stream_has_a_case_or_an_exemption():
    streamed = with_stream(declared())
    covered, exempt = sc.covered_entries(), set(sc.EXEMPT)
    assert not covered & exempt
    assert streamed - covered - exempt == set(), "entry points without a stream case (tests/stream_cases.py)"
    assert (covered | exempt) - streamed == set(), "names that the header does not declare with a stream"
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in sc.EXEMPT.values())


def test_removing_any_case_is_noticed(monkeypatch):
    """No case is there for nothing: without any one of them, some entry point or some op family is left uncovered — unless
    the case is a second shape of an entry point (another kernel, another branch of its launcher)."""
    streamed = with_stream(declared())
    families = {o.rstrip("_") for o in ops.FUNCTIONAL_OPS + ops.INPLACE_OPS}
    second_shapes = set()
    for name in list(sc.CASES):
        rest = {k: v for k, v in sc.CASES.items() if k != name}
        monkeypatch.setattr(sc, "CASES", rest)
        lost = (streamed - sc.covered_entries() - set(sc.EXEMPT)) | (families - sc.covered_op_families())
        monkeypatch.undo()
        if not lost:
            second_shapes.add(name)
    assert second_shapes == {"score_sed_valu_filter", "score_sed_exact", "select_best_one_block", "select_best_multi_block",
                             "ransac_pass_batch", "ransac_pass_batch_matrix", "match_summary_ncc", "match_summary_ssd_uint8",
                             "triangulate_tracks", "triangulate_tracks_refined"}


def test_the_host_only_functions_take_no_stream():
    functions = declared()
    streamed = with_stream(functions)
    for name in sc.HOST_ONLY:
        assert name in functions and name not in streamed, name
    # everything without a stream is a size, an option or a host function
    for name in set(functions) - streamed:
        assert name in sc.HOST_ONLY or name.endswith("_workspace_bytes") or name.endswith("_workspace_bytes_ex") \
            or name in ("sfm_last_error", "sfm_abi_version"), name


def test_the_synchronising_entry_points_are_the_ones_the_header_names():
    functions = declared()
    says_so = {name for name, (_, comment) in functions.items() if SYNC_PHRASE in comment}
    assert says_so == set(sc.SYNCHRONISING)
    assert says_so <= with_stream(functions) and says_so <= sc.covered_entries()
    for case in sc.CASES.values():   # a case is either wholly synchronising or not at all: it gets one kind of check
        assert len({e in sc.SYNCHRONISING for e in case.entries}) == 1, case.name
    with open(HEADER) as f:
        text = f.read()
    assert "Calls only enqueue work" in text and "nothing synchronises with the host" in text


def test_every_op_family_is_reached():
    listed = set(ops.FUNCTIONAL_OPS + ops.INPLACE_OPS)
    named = {o for c in sc.CASES.values() for o in c.ops}
    assert named - listed == set(), "a case names an op that ops.py does not list"
    families = {o.rstrip("_") for o in listed}
    assert families - sc.covered_op_families() == set(), "op families no stream case reaches"
