#!/usr/bin/env python3
"""Which C entry points raymond_amd/render.py calls, with which arguments in which order:

    python tools/record_binding_trace.py --recorded-from <the commit recorded> --out tests/golden/binding_trace.json

Runs every scenario of tests/binding_trace.py against its recording stand-in for the library (no .so, no GPU) and writes them: every
distinct line (a C call, a message or a result) once, and per scenario the numbers of its lines.  tests/test_binding_trace.py replays the scenarios
and compares.  The file is recorded once, from the commit before a change of render.py that is meant to keep its calls; a difference afterwards is a bug in that change, not a reason to record again.

When scenarios are ADDED the file has to be made again; what it already holds must not move with that:

    python tools/record_binding_trace.py --keep OLD.json --recorded-from <commit> --out tests/golden/binding_trace.json

refuses to write if any scenario of OLD.json (an earlier file of this tool's) is missing now or has another trace — not one line more or less —, and
prints the differences.  `--keep OLD.json --out /dev/null` only compares.
"""
import argparse
import difflib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT), sys.path.insert(0, os.path.join(ROOT, "tests"))

import binding_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--recorded-from", default="the working tree", help="what was recorded, for the file's header (a commit, say)")
    ap.add_argument("--keep", metavar="OLD.json", help="an earlier recording: refuse to write if one of its scenarios has another trace now")
    a = ap.parse_args()
    traces = {name: binding_trace.run(name) for name in binding_trace.SCENARIOS}
    if a.keep:
        with open(a.keep) as f:
            old = json.load(f)
        moved = 0
        for name, numbers in old["scenarios"].items():
            was = [old["lines"][int(i)] for i in numbers.split()]
            if traces.get(name) != was:
                moved += 1
                print("\n".join(difflib.unified_diff(was, traces.get(name, []), "%s in %s" % (name, a.keep), "%s now" % name, lineterm="", n=1)))
        if moved:
            sys.exit("%d of the %d scenarios of %s changed: nothing written" % (moved, len(old["scenarios"]), a.keep))
        print("the %d scenarios of %s are unchanged; %d new" % (len(old["scenarios"]), a.keep, len(set(traces) - set(old["scenarios"]))))
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
