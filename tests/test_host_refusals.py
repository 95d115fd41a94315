"""The C++ mirror's render_tiled refuses what it refused, in the order it checked it, before a worker is started.

tests/golden/host_refusals.json was recorded by tools/record_host_refusals.py from raymond_cli as it was before the settings checks were gathered in
check_settings: every fault of the recorder's list alone and every ordered pair of two different faults that can be set together (the caller sees the
FIRST failing check's text, so the pairs pin the order).  The same list is replayed here against the tree's raymond_cli, and every case must come out
with the recorded exit status and the recorded stderr, whole."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_host_refusals", os.path.join(ROOT, "tools", "record_host_refusals.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(ROOT, "tests", "golden", "host_refusals.json")) as _f:
    GOLDEN = json.load(_f)
N = len(rec.FAULTS)


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def test_the_fixture_covers_every_fault_and_every_pair():
    assert list(GOLDEN["singles"]) == [rec.case_id(a) for a in rec.FAULTS] and N >= 31  # (render_tiled has 31 checks)
    assert len(GOLDEN["pairs"]) == N and all(len(row) == N for row in GOLDEN["pairs"])
    for i, a in enumerate(rec.FAULTS):
        for j, b in enumerate(rec.FAULTS):
            cell = GOLDEN["pairs"][i][j]
            assert (cell == ".") == (i == j) and (cell == "-") == (i != j and rec.together(a, b) is None), (a, b)  # every pair that can be set was recorded
    # the list is what it says: every outcome is a refusal of render_tiled, and every check's text is among the single faults' (31 different ones)
    assert all(status == 1 and text.startswith(rec.REFUSAL) and text.endswith("\n") and text.count("\n") == 1 for status, text in GOLDEN["outcomes"])
    assert len({GOLDEN["singles"][rec.case_id(a)] for a in rec.FAULTS}) == 31


@pytest.mark.parametrize("i", range(N), ids=[rec.case_id(a).replace(" ", "_") for a in rec.FAULTS])
def test_every_case_is_answered_as_recorded(cli, tmp_path, i):
    a, row = rec.FAULTS[i], GOLDEN["pairs"][i]
    assert rec.call(cli, a, str(tmp_path)) == GOLDEN["outcomes"][GOLDEN["singles"][rec.case_id(a)]], a
    replayed = 1
    for j, b in enumerate(rec.FAULTS):
        if row[j] in ".-+":  # itself; an option with two values; together no refusal (a render would start)
            continue
        assert rec.call(cli, rec.together(a, b), str(tmp_path)) == GOLDEN["outcomes"][rec.CELLS.index(row[j])], (a, b)
        replayed += 1
    assert replayed == 1 + sum(c in rec.CELLS for c in row)  # none skipped
    assert not (tmp_path / "x.ppm").exists()
