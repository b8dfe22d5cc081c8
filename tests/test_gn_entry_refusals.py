"""The refusals of the GroupNorm stage's 13 launching C entry points and the zero answers of its four workspace queries, pinned whole:
the same return code and the same message, byte for byte, as the build that tests/golden/gn_entry_refusals.json was made from
(tools/make_golden_gn_refusals.py: one argument wrong at a time for every check of every entry point, and pairs of faults that pin the
order of the checks).  No GPU: the device pointers are fake and every call is refused before a launch."""
import importlib.util
import json
import os

import pytest

from inverserenderingofindoorscene_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_gn_refusals", os.path.join(ROOT, "tools", "make_golden_gn_refusals.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

with open(T.OUT) as _f:
    GOLDEN = json.load(_f)
FAULTS = {(entry, T.label(fault)): fault for entry, fault in T.CASES}


def test_the_file_holds_every_case_of_the_tool_and_only_refusals():
    assert [(r["entry"], r["case"]) for r in GOLDEN] == [(entry, T.label(fault)) for entry, fault in T.CASES]
    assert len(FAULTS) == len(T.CASES)
    assert {r["entry"] for r in GOLDEN} == set(T.ENTRIES) | set(T.QUERIES) and len(T.ENTRIES) == 13 and len(T.QUERIES) == 4
    for r in GOLDEN:
        if r["entry"] in T.QUERIES:
            assert r["code"] == 0 and r["message"] == "", r
        else:      # a refused call: an accepted one would launch
            assert r["code"] in (-1, -2) and r["message"].startswith(r["entry"].replace("_bf16", "") + ": "), r


@pytest.mark.parametrize("entry", list(T.ENTRIES) + list(T.QUERIES))
def test_every_refusal_is_the_pinned_one(entry):
    lib = _lib.load()
    rows = [r for r in GOLDEN if r["entry"] == entry]
    assert rows
    for r in rows:
        assert r["code"] != 0 or entry in T.QUERIES, r
        code, message = T.call(lib, entry, FAULTS[(entry, r["case"])])
        assert (code, message) == (r["code"], r["message"]), r
