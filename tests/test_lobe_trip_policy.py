"""The trip rule of the role-sorted spheres kernel (raymond_amd/csrc/lobe_trips.hpp) on the CPU.

The header that render_wave_sorted takes its rule from needs only <stdint.h>: tests/lobe_trip_policy_main.cpp, a stand-alone program built here with
-fsanitize=address,undefined and run directly, drives it through 10^5 seeded random park / shade sequences — lobe shares 0, 0.1, 0.5, 0.9 and 1,
items of 1 to 200 generation trips (every size with every share), park probabilities drawn per sequence, every seventh sequence with every path run to the bounce limit — with the
array's entries tracked one by one, and stops at the first sequence in which
  * the two stacks overlap (a push lands on an entry in use, a pop on an entry that is not its lobe's, or the entries disagree with the counters),
  * a generation trip runs without 64 free entries,
  * a trip has no lane,
  * the loop has not ended within kTripBoundPerPair's bound.
The stack size, the bound and the bounce limit are read from the sources the kernel is built from."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")


def constant(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, (path, pattern)
    return int(m.group(1))


def test_random_park_and_shade_sequences_keep_the_rule(tmp_path):
    slots = constant("launch.hpp", r"constexpr uint32_t kSortSlots = (\d+);")
    max_segments = constant("launch.hpp", r"#define RMD_MAX_BOUNCE_LIMIT_DEV (\d+)u")
    per_pair = max_segments + constant("render_kernel.hpp", r"constexpr uint32_t kTripBoundPerPair = RMD_MAX_BOUNCE_LIMIT_DEV \+ (\d+)u;")
    assert slots == 168 and constant("launch.hpp", r"constexpr size_t kSortPoolBytes = (\d+)u \* kSortSlots;") * slots == 10080  # 16 waves a CU, as before
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "lobe_trip_policy")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lobe_trip_policy_main.cpp"), "-o", exe], check=True)
    # 10^5 sequences, in eight runs of 12,500 side by side (a sequence is seeded by its number: the split changes nothing)
    runs = [subprocess.Popen([exe, str(slots), str(per_pair), str(max_segments), str(first), "12500"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for first in range(0, 100000, 12500)]
    trips = [0, 0]
    for r in runs:
        out, err = r.communicate(timeout=600)
        print(out, err[-3000:])
        assert r.returncode == 0 and "lobe trip policy ok: 12500 sequences" in out, (out[-2000:], err[-3000:])
        m = re.search(r"diffuse trips (\d+) .* GGX trips (\d+)", out)
        trips = [trips[0] + int(m.group(1)), trips[1] + int(m.group(2))]
    assert trips[0] > 0 and trips[1] > 0  # both kinds of shading trip ran
    # ... and the rule holds for the smallest stack the kernel's static_assert admits as well
    r = subprocess.run([exe, "72", str(per_pair), str(max_segments), "0", "1000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
