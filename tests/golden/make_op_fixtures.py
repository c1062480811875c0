"""Record what the op layer shows a caller, on a machine without a GPU:  ``python tests/golden/make_op_fixtures.py``.

Writes ``op_schemas.json`` (every registered ``sfm_hip::`` schema) and ``op_meta_shapes.json`` (the outcome of every call
of tests/op_meta_cases.py on Meta tensors: output shapes and dtypes, or the error text).  Both were recorded on the commit
before the functional and Meta forms of each op were merged into one body, and tests/test_op_meta_fixtures.py holds every
later build to them: regenerate them only for a deliberate change of an op, never to make that test pass.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import op_meta_cases  # noqa: E402
from structure_from_motion_amd import build, ops  # noqa: E402


def main():
    build.build_all()
    op = ops.load()
    for name, content in (("op_schemas.json", op_meta_cases.schemas()), ("op_meta_shapes.json", op_meta_cases.run(op))):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(content, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"{name}: {len(content)} entries")


if __name__ == "__main__":
    main()
