"""rmd_luminance_histogram_tiles and rmd_exposure_from_histogram: the parts that need no GPU.

Both entry points are exported and declared as the header states them, the struct has the header's layout, every argument rule of both comes with its
own text (the histogram call's before the context is looked at), rmd_exposure_from_histogram equals its Python restatement (tests/luma_ref.py) bit for
bit on hand-made histograms, the binning header the kernel is built from passes tests/luma_bins_main.cpp under the sanitizers, both host mirrors hold
the settings' rules, and the C++ mirror's host histogram of a small image is the numpy restatement's.
"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import luma_ref
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


# ---------------------------------------------------------------- the boundary
def test_entry_points_are_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert {"rmd_luminance_histogram_tiles", "rmd_exposure_from_histogram"} <= exported
    assert len(lib.SIGNATURES["rmd_luminance_histogram_tiles"][1]) == 9 and len(lib.SIGNATURES["rmd_exposure_from_histogram"][1]) == 4
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_luminance_histogram_tiles(rmd_context *ctx, const double *accum_dev, const double *accum2_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, rmd_luma_histogram *out_host);") in header
    assert "rmd_status rmd_exposure_from_histogram(const rmd_luma_histogram *h, double percentile, double target, double *out_exposure);" in header
    assert "#define RMD_LUMA_BINS 256u" in header and abi.RMD_LUMA_BINS == 256
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # an addition within ABI 6
    fault_list = header[header.index("Reported by the first call that waits"):header.index("rmd_denoise_atrous) */")]
    assert "rmd_luminance_histogram_tiles" in fault_list


def test_struct_layout_matches_the_c_header():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "raymond_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rmd_luma_histogram), offsetof(rmd_luma_histogram, bins), offsetof(rmd_luma_histogram, below),
         offsetof(rmd_luma_histogram, above), offsetof(rmd_luma_histogram, zero), offsetof(rmd_luma_histogram, negative),
         offsetof(rmd_luma_histogram, not_finite), offsetof(rmd_luma_histogram, pixels));
  return 0; }
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [262 * 8, 0, 256 * 8, 257 * 8, 258 * 8, 259 * 8, 260 * 8, 261 * 8]
    H = abi.LumaHistogram
    assert [C.sizeof(H), H.bins.offset, H.below.offset, H.above.offset, H.zero.offset, H.negative.offset, H.not_finite.offset, H.pixels.offset] == got


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_histogram_argument_rules_come_before_the_context(product_lib):
    """rmd_resolve_tonemap_tiles's rules, in its order; every one is reported with a null context, and a call that passes them all reaches it."""
    L = product_lib
    W, H = 8, 8
    span = W * H * 3 * 8
    base = 0x100000
    a, b = C.c_void_p(base), C.c_void_p(base + span)
    full = _rects((0, 0, 8, 8))
    counts = (C.c_uint32 * 2)(4, 4)
    out = abi.LumaHistogram()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))

    def call(A=a, B=None, w=W, h=H, rects=full, cnt=counts, n_rects=1, o=C.byref(out)):
        return L.rmd_luminance_histogram_tiles(None, A, B, w, h, rects, cnt, n_rects, o)

    def refused(text, status=abi.RMD_ERR_INVALID_ARGUMENT, **kw):
        assert call(**kw) == status, kw
        assert _last_error(L) == "rmd_luminance_histogram_tiles: " + text, (kw, _last_error(L))
        assert bytes(out) == b"\xab" * C.sizeof(out)  # the output untouched

    for kw in (dict(A=None), dict(w=0), dict(h=0), dict(rects=None), dict(cnt=None)):
        refused("bad argument", **kw)
    refused("accum2_dev overlaps accum_dev", B=a)
    refused("accum2_dev overlaps accum_dev", B=C.c_void_p(base + span - 8))
    refused("accum2_dev overlaps accum_dev", B=C.c_void_p(base - span + 8))
    refused("tile rectangle outside the framebuffer", rects=_rects((0, 0, 9, 8)))
    refused("tile rectangle outside the framebuffer", rects=_rects((4, 4, 4, 5)))
    refused("tile rectangle outside the framebuffer", rects=_rects((2**32 - 4, 0, 8, 8)))  # left + width wraps
    big = 70000
    refused("more than 2^32-1 packed pixels", status=abi.RMD_ERR_UNSUPPORTED, w=big, h=big, rects=_rects((0, 0, big, big)))
    refused("null out_host", o=None)
    refused("null out_host", o=None, rects=None, cnt=None, n_rects=0)  # even where there is nothing to count
    # the order is the resolve call's: the pointers, then the overlap, then the rects, then the pixel count, then the output
    refused("bad argument", A=None, B=a, rects=_rects((0, 0, 9, 8)), o=None)
    refused("accum2_dev overlaps accum_dev", B=a, rects=_rects((0, 0, 9, 8)), o=None)
    refused("tile rectangle outside the framebuffer", rects=_rects((0, 0, 9, 8)), o=None)
    refused("more than 2^32-1 packed pixels", status=abi.RMD_ERR_UNSUPPORTED, w=big, h=big, rects=_rects((0, 0, big, big)), o=None)
    # what passes reaches the context: a second buffer beside the first, overlapping rects, rects without pixels, counts of 0, no rects
    zero_counts = (C.c_uint32 * 2)(0, 0)
    for kw in ({}, dict(B=b), dict(rects=_rects((0, 0, 4, 4), (3, 3, 2, 2)), n_rects=2), dict(rects=_rects((3, 3, 0, 2))), dict(cnt=zero_counts),
               dict(rects=None, cnt=None, n_rects=0), dict(n_rects=0)):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))
        assert bytes(out) == b"\xab" * C.sizeof(out)


def test_exposure_argument_rules(product_lib):
    L = product_lib
    h, out = abi.LumaHistogram(), C.c_double(-7.0)
    h.bins[128] = 5

    def refused(text, hist=C.byref(h), p=0.99, t=0.8, o=C.byref(out)):
        assert L.rmd_exposure_from_histogram(hist, p, t, o) == abi.RMD_ERR_INVALID_ARGUMENT, (p, t)
        assert _last_error(L) == "rmd_exposure_from_histogram: " + text, _last_error(L)
        assert out.value == -7.0

    refused("null pointer", hist=None)
    refused("null pointer", o=None)
    for bad in (0.0, -0.5, 1.0000000000000002, 2.0, float("nan"), float("inf"), -float("inf")):
        refused("percentile must be finite and in (0, 1]", p=bad)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        refused("target must be finite and in (0, 1)", t=bad)
    refused("percentile must be finite and in (0, 1]", p=0.0, t=1.0)  # the percentile is looked at first
    assert L.rmd_exposure_from_histogram(C.byref(h), 1.0, 0.5, C.byref(out)) == abi.RMD_OK and out.value > 0.0
    assert L.rmd_exposure_from_histogram(C.byref(h), 5e-324, 1.0 - 2.0**-53, C.byref(out)) == abi.RMD_OK  # the ends of both ranges


# ---------------------------------------------------------------- the exposure against its restatement
def _bits(x):
    return struct.pack("<d", x)


def _hist(bins=None, **side):
    h = render.LumaHistogram(**side)
    for i, n in (bins or {}).items():
        h.bins[i] = n
    return h


def test_exposure_is_the_restatement_bit_for_bit(product_lib):
    cases = []
    three = _hist({100: 50, 130: 49, 131: 1})  # N = 100
    # the rank lands exactly on a bin's last pixel (r = 50: bin 100, r = 99: bin 130), and one past it (r = 51: bin 130, r = 100: bin 131)
    for p in (0.5, 0.99, 0.51, 0.505, 1.0, 0.995, 0.01, 1e-9, 5e-324):
        cases.append((three, p, 0.8))
    # the rank counts `below` first and `above` last; zero, negative and not_finite take no part
    sides = _hist({0: 10, 255: 10}, below=10, above=10, zero=1000, negative=1000, not_finite=1000, pixels=3040)
    for p in (0.25, 0.2500001, 0.5, 0.75, 0.7500001, 1.0, 1e-300):
        cases.append((sides, p, 0.8))
    cases += [(_hist(below=7), p, 0.5) for p in (1e-9, 0.5, 1.0)]  # only `below`
    cases += [(_hist(above=7), p, 0.5) for p in (1e-9, 0.5, 1.0)]  # only `above`
    cases += [(_hist(), 0.99, 0.8), (_hist(zero=5, negative=6, not_finite=7, pixels=18), 0.99, 0.8)]  # N = 0
    cases += [(_hist({i: 1}), 1.0, t) for i in (0, 1, 2, 3, 127, 128, 129, 254, 255) for t in (0.8, 0.18, 1e-12, 1.0 - 2.0**-53)]  # every M, both ends
    huge = _hist({7: 2**63, 200: 2**63 - 2, 201: 1})  # N = 2^64 - 1: (double)N rounds up to 2^64
    cases += [(huge, p, 0.8) for p in (1.0, 0.5, 0.5000000000000001, 1.0 - 2.0**-53)]
    rng = np.random.default_rng(12)
    for _ in range(200):
        h = render.LumaHistogram(rng.integers(0, 1000, 256) * (rng.uniform(size=256) < 0.1), below=int(rng.integers(0, 3)), above=int(rng.integers(0, 3)))
        cases.append((h, float(rng.uniform(1e-3, 1.0)), float(rng.uniform(0.01, 0.99))))
    for h, p, t in cases:
        got, want = render.exposure_from_histogram(h, p, t), luma_ref.exposure(h, p, t)
        assert _bits(got) == _bits(want), (h, p, t, got, want)
    # the issue's worked example: the 99th percentile in [1.5, 1.75) -> Y_p = 1.75, exposure 0.92
    assert abs(render.exposure_from_histogram(_hist({130: 1})) - 0.9196788) < 1e-6
    assert render.exposure_from_histogram(_hist()) == 1.0
    assert render.exposure_from_histogram(_hist(below=1), 0.5, 0.5) == -np.log1p(-0.5) * 2.0**32
    assert render.exposure_from_histogram(_hist(above=1), 0.5, 0.5) == -np.log1p(-0.5) / 2.0**32


def test_add_histograms_adds_every_counter():
    rng = np.random.default_rng(3)
    a = render.LumaHistogram(rng.integers(0, 2**40, 256), 1, 2, 3, 4, 5, 6)
    b = render.LumaHistogram(rng.integers(0, 2**40, 256), 10, 20, 30, 40, 50, 60)
    s = render.add_histograms(a, b)
    assert np.array_equal(s.counters(), a.counters() + b.counters()) and s == render.add_histograms(b, a)
    assert (s.below, s.above, s.zero, s.negative, s.not_finite, s.pixels) == (11, 22, 33, 44, 55, 66)
    assert render.LumaHistogram.from_struct(s.to_struct()) == s
    # the restatement over two disjoint rect lists adds up to the one over both
    acc = rng.uniform(0, 4, (9, 11, 3))
    left, right = [(0, 0, 5, 9)], [(5, 0, 6, 9)]
    assert render.add_histograms(luma_ref.histogram(acc, left, [2]), luma_ref.histogram(acc, right, [3])) == luma_ref.histogram(acc, left + right, [2, 3])


# ---------------------------------------------------------------- the binning header, on the CPU under the sanitizers
def test_the_binning_header_agrees_with_frexp_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "luma_bins.hpp")).read()
    includes = re.findall(r"#include [<\"]([^>\"]+)[>\"]", header)
    assert includes == ["stdint.h"], includes  # nothing of the project, nothing of HIP
    assert "__host__ __device__" in header
    kernel = open(os.path.join(CSRC, "luma_histogram.hip")).read()
    assert '#include "luma_bins.hpp"' in kernel and "luma_counter(luma_bits(luma_of(" in kernel  # the kernel reads the same lines
    assert '#include "../csrc/luma_bins.hpp"' in open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "luma_bins")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "luma_bins_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "1", "1000000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"luma bins ok: (\d+) values, (\d+) of 261 counters", r.stdout)
    assert m and int(m.group(1)) >= 10**6 + 3 * 68 * 4 and int(m.group(2)) >= 260  # (a random pattern is never +-0)


def test_the_numpy_restatement_reads_the_same_counters():
    """tests/luma_ref.py's counter_of on the program's values: the edges open their own bins, and the pins of the specials."""
    edges = luma_ref.edge_values()
    got = luma_ref.counter_of(np.array(edges))
    k = 0
    for e in range(-34, 34):
        for m in range(4):
            at, under, over = (int(v) for v in got[k : k + 3])
            k += 3
            if e < -32:
                assert (at, under, over) == (luma_ref.BELOW,) * 3
            elif e >= 32:
                assert at == over == luma_ref.ABOVE and under == (255 if (e, m) == (32, 0) else luma_ref.ABOVE)
            else:
                b = (e + 32) * 4 + m
                assert at == over == b and under == (b - 1 if b else luma_ref.BELOW)
    sp = luma_ref.counter_of(luma_ref.special_values())
    Z, B, N, F, A = luma_ref.ZERO, luma_ref.BELOW, luma_ref.NEGATIVE, luma_ref.NOT_FINITE, luma_ref.ABOVE
    assert list(sp) == [Z, Z, B, B, N, N, F, F, F, F, F, F, F, F, F, F, B, A, N, N, N]
    for v in edges:  # every positive target can be made the luminance of a radiance, exactly
        p = luma_ref.radiance_with_luminance(v)
        assert p is not None and luma_ref.luminance(np.array(p)) == v


# ---------------------------------------------------------------- the host mirrors
def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


def test_settings_defaults_and_rules():
    st = settings()
    assert st.preview_auto_exposure is False and st.auto_exposure_percentile == 0.99 and st.auto_exposure_target == 0.8
    st.check_preview()
    on = settings(samples_per_iteration=2, preview_every=1, preview_auto_exposure=True, auto_exposure_percentile=1.0, auto_exposure_target=0.5)
    on.check_preview(2)  # several devices: their histograms are added
    assert (on.preview_auto_exposure, on.auto_exposure_percentile, on.auto_exposure_target) == (True, 1.0, 0.5)
    with pytest.raises(ValueError, match="preview_auto_exposure needs preview_every > 0"):
        settings(samples_per_iteration=2, preview_auto_exposure=True)
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"auto_exposure_percentile must be finite and in \(0, 1\]"):
            settings(auto_exposure_percentile=bad)  # checked whether or not the setting is on
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"auto_exposure_target must be finite and in \(0, 1\)"):
            settings(auto_exposure_target=bad)
    on.auto_exposure_target = 1.0
    with pytest.raises(ValueError, match="auto_exposure_target"):
        render.render_tiled(scenes.reflective_spheres(), on)  # render_tiled asks again, before it opens a device
    assert render.Message.FramePreview(None, 1, 2).exposure is None and render.Message.FramePreview(None, 1, 2, 0.5).exposure == 0.5


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_parses_the_flags_and_holds_the_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    base = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]
    for extra, word in ((["--auto-exposure", "1", "--auto-exposure-percentile", "0"], "auto_exposure_percentile must be finite and in (0, 1]"),
                        (["--auto-exposure", "1", "--auto-exposure-percentile", "1.5"], "auto_exposure_percentile must be finite and in (0, 1]"),
                        (["--auto-exposure-percentile", "nan"], "auto_exposure_percentile must be finite and in (0, 1]"),
                        (["--auto-exposure", "1", "--auto-exposure-target", "1"], "auto_exposure_target must be finite and in (0, 1)"),
                        (["--auto-exposure-target", "-0.5"], "auto_exposure_target must be finite and in (0, 1)"),
                        (["--auto-exposure", "1", "--preview-every", "2"], "preview_every > 0 needs samples_per_iteration > 0")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    header = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.hpp")).read()
    assert "bool preview_auto_exposure = false;" in header and "double auto_exposure_percentile = 0.99, auto_exposure_target = 0.8;" in header
    assert "std::optional<double> exposure;" in header


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK), reason="a GPU is present")
def test_cli_auto_exposure_without_a_gpu_fails_loudly(cli, tmp_path):
    r = subprocess.run([cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm"), "--spi", "2", "--preview-every", "1", "--auto-exposure", "1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "no HIP device" in r.stderr and not (tmp_path / "x.ppm").exists()


def test_the_cpp_mirrors_host_histogram_is_the_restatements(cli, tmp_path):
    """raymond::luminance_histogram — what raymond_cli --auto-exposure 1 makes the final frame's exposure from — through `raymond_cli lumahist`: a 23 x 17
    image of the program's values (every edge and its neighbours as exact luminances, the specials in all three channels) and random radiances."""
    rng = np.random.default_rng(8)
    W, H = 23, 17
    img = np.exp2(rng.uniform(-40, 40, (H * W, 3)))
    targets = [luma_ref.radiance_with_luminance(v) for v in luma_ref.edge_values()]
    pick = rng.choice(len(targets), 200, replace=False)
    img[:200] = [targets[i] for i in pick]
    sp = luma_ref.special_values()
    img[200 : 200 + len(sp)] = sp[:, None]
    img = img.reshape(H, W, 3)
    path = tmp_path / "frame.f64"
    img.tofile(path)
    want = luma_ref.histogram(img, [(0, 0, W, H)], [1])
    assert want.zero >= 2 and want.negative >= 4 and want.not_finite >= 9 and want.below >= 2 and want.above >= 1 and np.count_nonzero(want.bins) > 100
    for args in ([], ["0.5", "0.18"]):
        r = subprocess.run([cli, "lumahist", str(path)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        counters, exposure = r.stdout.strip().split("\n")
        assert np.array_equal(np.array([int(v) for v in counters.split()], dtype=np.uint64), want.counters())
        p, t = (float(a) for a in args) if args else (0.99, 0.8)
        assert _bits(float(exposure)) == _bits(luma_ref.exposure(want, p, t))
