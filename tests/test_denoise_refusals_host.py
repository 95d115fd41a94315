"""The denoise entry points and rmd_tile_error_dual refuse what they refused, in the order they checked it, before a device is touched.

tests/golden/denoise_refusals.json was recorded by tools/record_denoise_refusals.py from the library as it was before the denoise host code was gathered
in api_denoise.cpp: per entry point every single fault the suite's argument-rule tests try, every ordered pair of two different faults (the caller sees the FIRST failing check's text, and
the families order their checks differently) and the valid variants, which get as far as "null context".  The same list is replayed here against the
library under test, and every case must come out with the recorded status and text."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_denoise_refusals", os.path.join(ROOT, "tools", "record_denoise_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(ROOT, "tests", "golden", "denoise_refusals.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_covers_every_entry_point_and_every_case():
    assert list(GOLDEN["entry_points"]) == list(rec.ENTRY_POINTS) and len(rec.ENTRY_POINTS) == 11
    assert GOLDEN["frame"] == [rec.W, rec.H]
    for name, e in GOLDEN["entry_points"].items():
        faults, valid = rec._faults(name)
        assert list(e["singles"]) == [rec.case_id(a) for a in faults] and list(e["valid"]) == [rec.case_id(v) for v in valid], name
        n = len(faults)
        assert len(e["pairs"]) == n and all(len(row) == n for row in e["pairs"]) and len(e["outcomes"]) <= len(rec.CELLS), name
        assert all((e["pairs"][i][j] == ".") == (i == j) for i in range(n) for j in range(n)), name  # every ordered pair was recorded
        # the list is what it says: every fault alone is refused with the entry point's own text, every valid variant reaches the context
        for o in e["singles"].values():
            status, text = e["outcomes"][o]
            assert status == rec.abi.RMD_ERR_INVALID_ARGUMENT and text.startswith(name + ": "), (name, text)
        assert all(e["outcomes"][o] == [rec.abi.RMD_ERR_INVALID_ARGUMENT, "null context"] for o in e["valid"].values()), name


@pytest.mark.parametrize("name", list(rec.ENTRY_POINTS))
def test_every_case_is_answered_as_recorded(product_lib, name):
    e = GOLDEN["entry_points"][name]
    n = len(e["singles"])
    pair = ((i, j) for i in range(n) for j in range(n) if i != j)
    replayed = 0
    for kind, cid, kw in rec.cases(name):
        if kind == "pairs":
            i, j = next(pair)
            want = e["outcomes"][rec.CELLS.index(e["pairs"][i][j])]
        else:
            want = e["outcomes"][e[kind][cid]]
        assert list(rec.call(product_lib, name, kw)) == want, (name, cid)
        replayed += 1
    assert replayed == n * n + len(e["valid"])  # n singles, n * (n - 1) pairs, the valid ones: none skipped
