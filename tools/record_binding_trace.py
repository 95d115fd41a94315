#!/usr/bin/env python3
"""Which C entry points raymond_amd/render.py calls, with which arguments in which order:

    python tools/record_binding_trace.py --recorded-from <the commit recorded> --out tests/golden/binding_trace.json

Runs every scenario of tests/binding_trace.py against its recording stand-in for the library (no .so, no GPU) and writes them: every
distinct line (a C call, a message or a result) once, and per scenario the numbers of its lines.  tests/test_binding_trace.py replays the scenarios
and compares.  The file is recorded once, from the commit before a change of render.py that is meant to keep its calls; a difference afterwards is a bug in that change, not a reason to record again.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT), sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--recorded-from", required=True, help="what was recorded, for the file's header (a commit, say)")
    a = ap.parse_args()
    traces = {name: binding_trace.run(name) for name in binding_trace.SCENARIOS}
    table = sorted({line for lines in traces.values() for line in lines})  # every distinct line once; a scenario is the numbers of its lines
    doc = {"about": "tools/record_binding_trace.py; recorded from: %s.  lines = every distinct line of the traces; scenarios = {name in "
                    "tests/binding_trace.py: the numbers of its lines in `lines`, in order}" % a.recorded_from,
           "lines": table, "scenarios": {name: " ".join(str(table.index(line)) for line in lines) for name, lines in traces.items()}}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("%d scenarios, %d lines -> %s (%d bytes)" % (len(doc["scenarios"]), sum(len(v) for v in traces.values()), a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
