#!/usr/bin/env python3
"""The worst relative difference per entry point and class from the "FRAMES ..." lines tests/test_gpu_denoise_frames.py prints
(tests/test_denoise_frames_host.py holds this reader to that file's printer):

    python -m pytest -m gpu tests/test_gpu_denoise_frames.py -s > frames.log
    python tools/denoise_frames_table.py frames.log            # one line per entry point and class (profiles/r24_denoise_frames/worst_differences.txt)
    python tools/denoise_frames_table.py frames.log --families # one row per entry point, the classes folded into grid / shape / seam / scale

share: |ref| / scale at the value with the worst relative difference — how far that mean has cancelled against the values it is a mean of.
"""
import collections
import re
import sys

LINE = re.compile(r"FRAMES entry=(\S+) class=(\S+) window=(.*) worst=(\S+) share=(\S+)")


def main(path, families):
    worst = collections.defaultdict(dict)
    for line in open(path):
        m = LINE.search(line)
        if not m:
            continue
        entry, cls, window, value, share = m.group(1), m.group(2), m.group(3), float(m.group(4)), m.group(5)
        key = ("grid" if cls.startswith("grid") else cls.split("_")[0]) if families else cls
        if key not in worst[entry] or value > worst[entry][key][0]:
            worst[entry][key] = (value, cls, window, share)
    for entry in sorted(worst):
        if families:
            cells = ["%.1e (%s at %s, share %s)" % worst[entry][k] if k in worst[entry] else "-" for k in ("grid", "shape", "seam", "scale")]
            print("| `%s` | %s |" % (entry, " | ".join(cells)))
        else:
            for cls in sorted(worst[entry]):
                value, _, window, share = worst[entry][cls]
                print("%-34s %-20s %8.1e  at %s  share %s" % (entry, cls, value, window, share))


if __name__ == "__main__":
    main(sys.argv[1], "--families" in sys.argv[2:])
