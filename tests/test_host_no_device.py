"""The C++ mirror's owners of device resources on the way out of a failure, under AddressSanitizer and UBSan, on a machine without a GPU.

tests/host_no_device_main.cpp is a program of its own: compiled here together with raymond.cpp and project.cpp with the sanitizers on, linked against
the library as it is built, and run directly.  It calls render_tiled(...).await() — one worker and one pass; two workers with passes of 2; the dual
loop with an adaptive threshold —, denoise_tiles, denoise_dual_tiles and render_features, and wants six raymond::Errors that name
rmd_context_create.

That is each function's FIRST failure and nothing deeper: what is held here is that a worker which never got a context tears down and reports,
that await() rethrows, and that the three callers leave without touching what they never owned.  The paths behind a context that exists are held by
the GPU tests that compare raymond_cli's bytes with the Python path's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "raymond_amd", "host")
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK), reason="a GPU is present")
def test_every_entry_point_fails_cleanly_without_a_device(product_lib, tmp_path):
    exe = str(tmp_path / "host_no_device")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + HOST,
                    os.path.join(ROOT, "tests", "host_no_device_main.cpp"), os.path.join(HOST, "raymond.cpp"), os.path.join(HOST, "project.cpp"), "-L" + CSRC,
                    "-lraymond_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)  # a sanitizer's report ends the program with another status
    assert not r.stderr.strip() and "6 of 6 refused by rmd_context_create" in r.stdout
