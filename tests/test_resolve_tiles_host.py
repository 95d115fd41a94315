"""The host arithmetic of rmd_resolve_tonemap_tiles (raymond_amd/csrc/resolve_tiles_host.hpp) on the CPU.

The header needs only <stdint.h> and the standard library: tests/resolve_tiles_table_main.cpp, a stand-alone program built here with
-fsanitize=address,undefined and run directly, drives it through 1,024 seeded random rect lists — empty rects, single pixels, rows, columns, tiles,
ragged rects, whole frames, and in every 64th list a frame of some 65000 x 55000 with one huge rect that fills what is left of 2^32 - 1 pixels — and stops
at the first list in which
  * a packed pixel is covered by no run of the workgroup table or by two (the runs are not one gapless sequence from 0 to the pixel count),
  * a run spans two rects, is empty, is longer than a workgroup's 1024 pixels or crosses a multiple of 1024,
  * resolve_locate — flagged packed pixel -> (rect, frame position) — does not invert the rect -> packed position of the table.
The run length and the group size are read from the header the kernel is built from."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")


def test_random_rect_lists_keep_the_table_and_its_inverse(tmp_path):
    header = open(os.path.join(CSRC, "resolve_tiles_host.hpp")).read()
    assert re.search(r"constexpr uint32_t kResolveGroup = 4u;", header) and re.search(r"constexpr uint32_t kResolveRun = 1024u;", header)
    includes = re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)
    assert sorted(includes) == ["algorithm", "stdint.h", "vector"], includes  # nothing of the project, nothing of HIP
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "resolve_tiles_table")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "resolve_tiles_table_main.cpp"), "-o", exe], check=True)
    # four runs of 256 lists side by side (a list is seeded by its number: the split changes nothing)
    runs = [subprocess.Popen([exe, str(first), "256"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for first in range(0, 1024, 256)]
    located = 0
    for r in runs:
        out, err = r.communicate(timeout=600)
        print(out, err[-3000:])
        assert r.returncode == 0 and "resolve tiles table ok: 256 lists" in out, (out[-2000:], err[-3000:])
        located += int(re.search(r"(\d+) pixels located", out).group(1))
    assert located > 10**6
