"""Every size export returns what tests/golden/workspace_sizes.json records (no GPU: host arithmetic only).

The file was written by tools/workspace_sizes.py from the library as it stood before the workspaces moved to one layout
function each (csrc/workspace.h); a layout whose total moves -- a region added, an alignment "fixed" -- shows here."""
import importlib.util
import json
import os

import pytest

from qrlsh import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")


def _tool():
    spec = importlib.util.spec_from_file_location("workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_size_export_is_recorded(golden):
    """the table covers every size export the header declares, each over the tool's whole table"""
    tool = _tool()
    recorded = {r["fn"]: r for r in golden}
    exports = tool.size_exports()
    assert len(exports) >= 39 and len(recorded) == len(golden)
    assert sorted(recorded) == sorted(name for name, _ in exports)
    for name, args in exports:
        assert recorded[name]["args"] == [a for _, a in args], name
        assert [case[:-1] for case in recorded[name]["cases"]] == tool.table(args), name


def test_sizes_are_the_recorded_ones(golden):
    lib = _lib.load()
    wrong = []
    cases = [(r["fn"], case[:-1], case[-1]) for r in golden for case in r["cases"]]
    for fn, args, value in cases:
        got = int(getattr(lib, fn)(*args))
        if got != value:
            wrong.append((fn, args, value, got))
    assert len(cases) > 1000 and not wrong, "%d of %d sizes moved, first: %s" % (len(wrong), len(cases), wrong[:5])
