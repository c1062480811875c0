"""The op layer as a caller sees it without a GPU: the registered schemas and what every op gives on Meta tensors, against
the fixtures tests/golden/make_op_fixtures.py recorded (op_schemas.json, op_meta_shapes.json)."""
import json
import os

import pytest

import op_meta_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def op(native_lib):
    from structure_from_motion_amd import ops

    return ops.load()


def test_registered_schemas_equal_the_fixture(op):
    recorded, now = _golden("op_schemas.json"), op_meta_cases.schemas()
    assert sorted(now) == sorted(recorded)
    for name in recorded:
        assert now[name] == recorded[name], name


def test_meta_outcomes_equal_the_fixture(op):
    recorded, now = _golden("op_meta_shapes.json"), op_meta_cases.run(op)
    assert sorted(now) == sorted(recorded)
    for case in recorded:
        assert now[case] == recorded[case], case


def test_inplace_ops_return_none_on_meta_buffers(op):
    for case, name, args in op_meta_cases.inplace_cases():
        assert getattr(op, name)(*args) is None, case


def test_every_op_has_a_case(op):
    """a functional op needs a well-formed call and one whose first tensor has the wrong rank (sample_philox takes no tensor);
    an in-place op one call"""
    functional = {name for _, name, _ in op_meta_cases.functional_cases()}
    ranked = {name for case, name, _ in op_meta_cases.functional_cases() if case.endswith("/rank")}
    inplace = {name for _, name, _ in op_meta_cases.inplace_cases()}
    for schema in _golden("op_schemas.json"):
        name = schema.split("::")[1]
        if name.endswith("_"):
            assert name in inplace, name
        else:
            assert name in functional, name
            assert name in ranked or name == "sample_philox", name
