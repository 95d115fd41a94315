#!/usr/bin/env python3
"""What the C++ mirror's render_tiled refuses in a Settings, and in which order it checks:

    python tools/record_host_refusals.py --cli <raymond_cli of the commit to record> --recorded-from <that commit> --out tests/golden/host_refusals.json

Every case is one `raymond_cli render spheres 32 32 8 2 OUT <flags>`.  render_tiled refuses before it starts a worker, so no device is touched and
the answer is an exit status and one line on stderr.  The fixed list FAULTS holds one set of flags per check of render_tiled (two where a check has
two arms, and NaN / infinity beside the plain bad value of some "finite and > 0" checks); a case is one fault alone, or an ordered pair (a, b) of two
different faults that can be set together — no option gets two values —, a's flags followed by b's.  The caller sees the FIRST failing check's
text, so the pairs pin the order of the checks.

Two faults together may cancel (`--denoise-dual 1 --spi 2` lacks --denoise, `--denoise 1 --denoise-dual 1` lacks --spi, their union lacks nothing):
such a pair is no refusal, it would start a render, and it is recorded as "+" and not replayed.

The file: "outcomes" is the table of [exit status, stderr] pairs, "singles" {case id: outcome index}, "pairs" a matrix over the faults in their
order, one string per row: character j of pairs[i] is the outcome index (CELLS) of "<fault i> + <fault j>", "." on the diagonal, "-" where the two
cannot be set together, "+" where together they are not refused.  tests/test_host_refusals.py replays every other cell.
"""
import argparse
import json
import os
import subprocess
import tempfile

DUAL = ("--denoise", "1", "--denoise-dual", "1", "--spi", "2")
PREVIEW = ("--preview-every", "2", "--spi", "2")
# one entry per check of render_tiled, in its order (check_preview's six first)
FAULTS = [
    ("--preview-every", "2"),
    ("--preview-exposure", "0"),
    ("--preview-exposure", "inf"),
    ("--preview-gamma", "0"),
    ("--preview-gamma", "nan"),
    ("--preview-denoise", "1"),
    PREVIEW + ("--preview-denoise", "1", "--gpus", "2"),
    PREVIEW + ("--gpus", "2"),
    ("--denoise-radius", "13"),
    ("--denoise-patch", "5"),
    ("--denoise-k", "0"),
    ("--denoise-k", "nan"),
    ("--denoise-alpha", "-1"),
    ("--denoise-alpha", "inf"),
    ("--denoise-feature-k", "0"),
    ("--denoise-feature-tau", "0"),
    ("--denoise-feature-tau", "nan"),
    ("--denoise-features", "1"),
    ("--denoise-atrous-levels", "9"),
    ("--denoise-atrous-k", "0"),
    ("--denoise-atrous-k", "inf"),
    ("--denoise-atrous", "1"),
    DUAL + ("--denoise-atrous", "1"),
    ("--adaptive", "-1"),
    ("--adaptive", "0.1"),
    ("--adaptive-floor", "0"),
    ("--adaptive-floor", "nan"),
    ("--denoise-dual", "1", "--spi", "2"),
    ("--denoise", "1", "--denoise-dual", "1"),
    DUAL + ("--denoise-features", "1"),
    ("--denoise-dual-features", "1"),
    ("--denoise-dual-select", "1"),
    ("--denoise-dual-atrous", "1"),
    DUAL + ("--denoise-dual-atrous", "1", "--denoise-dual-select", "1"),
    ("--denoise-dual-atrous-region", "1"),
    ("--adaptive-denoised", "-1"),
    ("--adaptive-denoised", "0.1"),
    DUAL + ("--adaptive-denoised", "0.1", "--adaptive", "0.1"),
    DUAL + ("--gpus", "2"),
]
CELLS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"  # a pair's outcome, one character: its index in "outcomes"
REFUSAL = "raymond_cli: render_tiled: "


def case_id(flags):
    return " ".join(flags)


def options(flags):
    return dict(zip(flags[0::2], flags[1::2]))


def together(a, b):
    """a's flags followed by those of b that a does not already hold; None where an option would get two values."""
    oa, ob = options(a), options(b)
    if any(k in oa and oa[k] != v for k, v in ob.items()):
        return None
    extra = tuple(x for k, v in ob.items() if k not in oa for x in (k, v))
    return a + extra


def call(cli, flags, tmp):
    """-> [exit status, stderr] of one case."""
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", os.path.join(tmp, "x.ppm"), *flags], capture_output=True, text=True)
    return [r.returncode, r.stderr]


def record(cli, recorded_from):
    about = ("tools/record_host_refusals.py; recorded from: %s.  outcomes = the [exit status, stderr] pairs; singles = {case id: outcome index}; pairs = one "
             "string per fault i, whose character j is the outcome index (in 0-9A-Za-z) of the case '<fault i> + <fault j>' (i's flags, then j's), '.' on "
             "the diagonal, '-' where an option would get two values, '+' where the two together are not refused (a render would start)." % recorded_from)
    n = len(FAULTS)
    outcomes, singles, pairs = [], {}, [["."] * n for _ in range(n)]

    def index(o):
        if o not in outcomes:
            outcomes.append(o)
        return outcomes.index(o)

    with tempfile.TemporaryDirectory() as tmp:
        for a in FAULTS:
            o = call(cli, a, tmp)
            assert o[0] == 1 and o[1].startswith(REFUSAL), (a, o)  # the list is what it says: every fault alone is refused by render_tiled
            singles[case_id(a)] = index(o)
        for i, a in enumerate(FAULTS):
            for j, b in enumerate(FAULTS):
                if i == j:
                    continue
                flags = together(a, b)
                if flags is None:
                    pairs[i][j] = "-"
                    continue
                o = call(cli, flags, tmp)
                refused = o[0] == 1 and o[1].startswith(REFUSAL)
                pairs[i][j] = CELLS[index(o)] if refused else "+"
    assert len(outcomes) <= len(CELLS)
    return {"about": about, "command": "render spheres 32 32 8 2 OUT", "outcomes": outcomes, "singles": singles, "pairs": ["".join(r) for r in pairs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", required=True, help="the raymond_cli to record from")
    ap.add_argument("--out", required=True)
    ap.add_argument("--recorded-from", required=True, help="what --cli was built from, for the file's header (a commit, say)")
    a = ap.parse_args()
    doc = record(a.cli, a.recorded_from)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    cells = "".join(doc["pairs"])
    print("%d faults, %d pairs replayed, %d cannot be set together, %d not refused together, %d outcomes -> %s (%d bytes)"
          % (len(FAULTS), sum(c in CELLS for c in cells), cells.count("-"), cells.count("+"), len(doc["outcomes"]), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
