"""Every denoise entry point and rmd_tile_error_dual give, bit for bit, what they gave before their kernels' per-pixel arithmetic moved into
raymond_amd/csrc/denoise_device.hpp.

tests/golden/denoise_bits.json was recorded by tools/record_denoise_bits.py on an MI355X from a build of the commit before that move: the SHA-256 of every
output array of its case list over one 70 x 37 frame with poisoned pixels, uncovered and single-sample rects and unaligned regions (the tool's docstring
has the recipe).  The same list is replayed here against the library under test.  No tolerance: the one-pass kernels (planes, combinations, count images)
are compiled from shared pixel functions now, and the suite's numpy restatements hold to 1e-9 only."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_denoise_bits", os.path.join(ROOT, "tools", "record_denoise_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(ROOT, "tests", "golden", "denoise_bits.json")) as _f:
    GOLDEN = json.load(_f)
RECORDED_WITH = "recorded with %s on %s" % (GOLDEN["hipcc"], GOLDEN["device"])


@pytest.fixture(scope="session")
def inputs():
    """The tool's inputs, held to the recorded hashes before any case makes its first GPU call."""
    x = rec.inputs()
    assert {k: rec.sha(v) for k, v in x.items()} == GOLDEN["inputs"]
    return x


def test_the_fixture_holds_every_case():
    assert GOLDEN["frame"] == [rec.W, rec.H] == [70, 37]
    assert list(GOLDEN["cases"]) == list(rec.CASES) and len(rec.CASES) == 33
    assert all(len(h) == 64 for c in GOLDEN["cases"].values() for h in c.values())
    assert sum("err" in c for c in GOLDEN["cases"].values()) == 19 and set(GOLDEN["cases"]["rmd_denoise_dual_select"]) == {"out", "err", "sure", "win"}


@pytest.mark.parametrize("name", list(rec.CASES))
def test_the_bytes_are_the_recorded_ones(inputs, gpu_ctx, name):
    got = {k: rec.sha(v) for k, v in rec.CASES[name](gpu_ctx, inputs).items()}
    assert got == GOLDEN["cases"][name], (name, RECORDED_WITH)
