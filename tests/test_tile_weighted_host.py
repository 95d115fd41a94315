"""rmd_tile_weighted_error and rmd_display_weights: the parts that need no GPU.

tests/tile_weighted_ref.py — the numpy restatement the device is held to (tests/test_gpu_tile_weighted.py) — is held here to the rule header the kernel is
built from, through the C++ mirror's host function (raymond_cli tile-weighted-error), bit for bit in all six fields; the rule header passes
tests/tile_weighted_rule_main.cpp under the host sanitizers; rmd_display_weights follows its formula's numpy restatement; the entry point's refusals come in
the header's order with a NULL context; rmd_tile_weighted has abi.TileWeighted's layout; both mirrors hold the settings' rules in the same words; what the
measure is for is stated as arithmetic; and each frame class of the GPU test is what it names."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tile_weighted_frames as frames
import tile_weighted_ref as ref
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
FRAME_NAMES = ["random", "tiny", "huge", "edges", "zeros", "saturated", "nan_in_S", "inf_in_Q"]


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


# ---------------------------------------------------------------- the boundary
def test_entry_points_are_exported_declared_and_stated(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert {"rmd_tile_weighted_error", "rmd_display_weights"} <= exported
    assert len(lib.SIGNATURES["rmd_tile_weighted_error"][1]) == 10 and len(lib.SIGNATURES["rmd_display_weights"][1]) == 4
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_tile_weighted_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_counts, uint32_t n_rects, const double *weights_host /* RMD_LUMA_WEIGHTS */, "
            "rmd_tile_weighted *out_host);") in header
    assert "rmd_status rmd_display_weights(double exposure, double gamma, double display_floor, double *out_weights /* RMD_LUMA_WEIGHTS */);" in header
    assert "#define RMD_LUMA_WEIGHTS 260u" in header and abi.LUMA_WEIGHTS == 260 == ref.N_WEIGHTS
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # additions within ABI 6
    for meaning in ("E = (w == 0.0) ? 0.0 : w * V", "(w0 + w1) + (w2 + w3)", "rms = sqrt(mean_weighted_variance)", "t(y) = -expm1(-y * e)",
                    "slope(y) = (1/g) * pow(t, 1/g - 1) * e * exp(-y * e)", "y_floor = -log1p(-pow(display_floor, g)) / e", "clamped to the largest finite double"):
        assert meaning in header, meaning


# ---------------------------------------------------------------- (a) the rule header through the C++ mirror is the restatement, bit for bit
def run_cli(cli, tmp_path, S, Q, rects, counts, weights):
    Hf, Wf = S.shape[:2]
    S.tofile(tmp_path / "S.f64"), Q.tofile(tmp_path / "Q.f64"), np.asarray(weights, dtype=np.float64).tofile(tmp_path / "w.f64")
    with open(tmp_path / "rects.txt", "w") as f:
        for (l, t, w, h), c in zip(rects, counts):
            f.write("%d %d %d %d %d\n" % (l, t, w, h, c))
    r = subprocess.run([cli, "tile-weighted-error", str(tmp_path / "S.f64"), str(tmp_path / "Q.f64"), str(Wf), str(Hf), str(tmp_path / "rects.txt"), "--weights",
                        str(tmp_path / "w.f64")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return parse_cli(r.stdout, len(rects))


def parse_cli(stdout, n_rects):
    out = np.zeros(n_rects, dtype=ref.DTYPE)
    lines = stdout.strip().split("\n") if n_rects else []
    assert len(lines) == n_rects
    for j, line in enumerate(lines):
        v = line.split()
        out[j] = tuple(np.array([int(x, 16) for x in v[:4]], dtype=np.uint64).view(np.float64)) + (int(v[4]), int(v[5]))  # the doubles as their bits
    return out


def assert_same_fields(got, want):
    assert list(got["valid"]) == list(want["valid"]) and list(got["invalid"]) == list(want["invalid"])
    for name in ref.FLOAT_FIELDS:
        assert ref.same_bits(got[name], want[name]), (name, got[name], want[name])


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_the_cpp_mirrors_host_function_is_the_restatement(cli, tmp_path, name):
    S, Q = frames.frames()[name]
    rects, counts = frames.rects_and_counts(frames.RECTS)
    for table_name, table in frames.tables().items():
        want = ref.tile_weighted_error(S, Q, rects, counts, table)
        assert_same_fields(run_cli(cli, tmp_path, S, Q, rects, counts, table), want)  # all six fields: both sides are host code, the square root included
        assert not any(np.isnan(want[f]).any() for f in ref.FLOAT_FIELDS), table_name


def test_the_cpp_mirrors_host_function_on_the_wide_frame_on_no_rects_and_with_the_tone_curves_arguments(cli, tmp_path):
    S, Q = frames.random_positive(frames.WIDE, frames.WIDE, seed=3)
    rects, counts = frames.rects_and_counts(frames.WIDE_RECTS)
    table = frames.tables()["random"]
    assert_same_fields(run_cli(cli, tmp_path, S, Q, rects, counts, table), ref.tile_weighted_error(S, Q, rects, counts, table))
    assert len(run_cli(cli, tmp_path, S, Q, [], [], table)) == 0
    # EXPOSURE GAMMA FLOOR in place of --weights: the library's own table
    S.tofile(tmp_path / "S.f64"), Q.tofile(tmp_path / "Q.f64")
    with open(tmp_path / "rects.txt", "w") as f:
        for (l, t, w, h), c in zip(rects, counts):
            f.write("%d %d %d %d %d\n" % (l, t, w, h, c))
    r = subprocess.run([cli, "tile-weighted-error", str(tmp_path / "S.f64"), str(tmp_path / "Q.f64"), str(frames.WIDE), str(frames.WIDE), str(tmp_path / "rects.txt"),
                        "0.92", "2.2", float(1.0 / 255.0).hex()], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert_same_fields(parse_cli(r.stdout, len(rects)), ref.tile_weighted_error(S, Q, rects, counts, render.display_weights(0.92, 2.2, 1.0 / 255.0)))
    # raymond_cli display-weights prints the library's table
    r = subprocess.run([cli, "display-weights", "0.92", "2.2", float(1.0 / 255.0).hex()], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    printed = np.array([int(x, 16) for x in r.stdout.split()], dtype=np.uint64).view(np.float64)
    assert ref.same_bits(printed, render.display_weights(0.92, 2.2, 1.0 / 255.0))


def test_the_rule_header_agrees_with_a_plain_reading_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "tile_weighted_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h", "luma_bins.hpp", "despike_rule.hpp", "tile_reduce.hpp"]  # nothing else of the project, nothing of HIP
    order = open(os.path.join(CSRC, "tile_reduce.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", order) == ["stdint.h"]
    kernel = open(os.path.join(CSRC, "tile_weighted.hip")).read()
    for fn in ("tile_weighted_add(", "tile_weighted_final(", "tile_sums_combine(", "__launch_bounds__(256)", "__shared__ double lds_weights[kLumaWeights]", "__syncthreads()"):
        assert fn in kernel, fn  # the kernel reads the same lines
    for fn in ("__shfl_xor(", "__syncthreads()", "tile_sums_combine(", "tile_rect_sums_host("):
        assert fn in order, fn  # ... and takes the order its sums are added in from where the host emulation takes it
    assert "tile_rect_sums_host(" in header
    assert "asm" not in kernel and "atomic" not in kernel.replace("No atomics", "") and "asm" not in order and "atomic" not in order
    for fn in ("exp(", "pow(", "log(", "expm1("):
        assert fn not in kernel and fn not in header and fn not in order, fn  # no transcendental function on the device
    assert "tile_weighted_pixel(" in header and "despike_pixel(" in header and "luma_counter(luma_bits(Y))" in header
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/tile_weighted_rule.hpp"' in mirror and "rmd::tile_weighted_rect_host(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "tile_weighted_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "tile_weighted_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "1", "10000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"tile weighted rule ok: (\d+) rects, (\d+) empty, (\d+) with an invalid pixel, (\d+) all valid, (\d+) of them with rms 0", r.stdout)
    assert m and int(m.group(1)) == 10000 and all(int(m.group(i)) > 100 for i in range(2, 6))


# ---------------------------------------------------------------- (b) rmd_display_weights
CURVES = [(1.0, 2.2, 1.0 / 255.0), (0.92, 2.2, 1.0 / 255.0), (1000.0, 2.2, 1.0 / 255.0), (0.001, 1.0, 1.0 / 255.0), (1.0, 0.5, 0.1)]


@pytest.mark.parametrize("e,g,floor", CURVES)
def test_display_weights_follow_the_formula(product_lib, e, g, floor):
    got = render.display_weights(e, g, floor)
    want, y_floor = ref.display_weights(e, g, floor)
    assert got.shape == (abi.LUMA_WEIGHTS,) and np.isfinite(got).all() and (got >= 0.0).all()
    zero = want == 0.0
    assert (got[zero] == 0.0).all() and (got[~zero] > 0.0).all()  # zeros exact
    rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
    print((e, g, floor), "largest relative difference from the numpy restatement", rel.max(), "y_floor", y_floor, "zeros", int(zero.sum()))
    assert rel.max() <= 1e-12  # the project's bar for values that pass through a library function
    centres = ref.bin_centres()
    under = centres <= y_floor
    assert ref.same_bits(got[:256][under], np.full(int(under.sum()), got[ref.ZERO]))  # bins under y_floor take the capped slope
    assert got[ref.BELOW] == got[ref.ZERO] == got[ref.NEGATIVE] and got[ref.ZERO] > 0.0
    assert got[ref.ABOVE] == 0.0  # slope(2^32)^2: exp(-2^32 e) is 0 at these exposures
    if g >= 1.0:
        assert (np.diff(got[:256]) <= 0.0).all() and got[ref.ZERO] >= got[0] and got[255] >= got[ref.ABOVE]  # non-increasing in y


def test_display_weights_at_the_starting_values(product_lib):
    got = render.display_weights()  # exposure 1, gamma 2.2, floor 1 / 255
    assert ref.same_bits(got, render.display_weights(1.0, 2.2, 1.0 / 255.0))
    assert int((got[:256] == 0.0).sum()) == 94  # the slope's square underflows from about y = 372 on: the bins from [416, 480) up
    assert got[:256][ref.bin_centres() > 480].max() == 0.0 and got[:256][ref.bin_centres() < 350].min() > 0.0
    # a pixel that displays at the floor: its slope is (1/g) D^(1 - g) (1 - D^g) e with D = 1 / 255
    D, g = 1.0 / 255.0, 2.2
    assert abs(got[ref.ZERO] / ((1.0 / g) * D ** (1.0 - g) * (1.0 - D**g)) ** 2 - 1.0) < 1e-12


def test_display_weights_refusals_and_extremes(product_lib):
    L = product_lib
    out = (C.c_double * abi.LUMA_WEIGHTS)()
    nan, inf = float("nan"), float("inf")
    for args, text in (((1.0, 2.2, 0.1, None), "null pointer"),
                       ((0.0, 2.2, 0.1, out), "exposure must be finite and > 0"), ((-1.0, 2.2, 0.1, out), "exposure must be finite and > 0"),
                       ((nan, 2.2, 0.1, out), "exposure must be finite and > 0"), ((inf, 2.2, 0.1, out), "exposure must be finite and > 0"),
                       ((1.0, 0.0, 0.1, out), "gamma must be finite and > 0"), ((1.0, -2.2, 0.1, out), "gamma must be finite and > 0"),
                       ((1.0, nan, 0.1, out), "gamma must be finite and > 0"), ((1.0, inf, 0.1, out), "gamma must be finite and > 0"),
                       ((1.0, 2.2, 0.0, out), "display_floor must be finite and in (0, 1)"), ((1.0, 2.2, 1.0, out), "display_floor must be finite and in (0, 1)"),
                       ((1.0, 2.2, -0.1, out), "display_floor must be finite and in (0, 1)"), ((1.0, 2.2, nan, out), "display_floor must be finite and in (0, 1)"),
                       ((1.0, 2.2, inf, out), "display_floor must be finite and in (0, 1)")):
        assert L.rmd_display_weights(*args) == abi.RMD_ERR_INVALID_ARGUMENT, args
        assert (L.rmd_last_error(None) or b"").decode() == "rmd_display_weights: " + text, args
    with pytest.raises(Exception):
        render.display_weights(0.0, 2.2, 0.1)
    # every output is finite and >= 0 for every accepted input, the ones where the formula overflows or gives NaN included
    for e in (5e-324, 1e-300, 1e-15, 1.0, 1e15, 1e300, 1.7e308):
        for g in (5e-324, 1e-300, 1e-3, 0.5, 1.0, 2.2, 1e3, 1e300, 1.7e308):
            for f in (5e-324, 1e-300, 1.0 / 255.0, 0.5, 1.0 - 2.0**-53):
                w = render.display_weights(e, g, f)
                assert np.isfinite(w).all() and (w >= 0.0).all(), (e, g, f)


# ---------------------------------------------------------------- (c) the refusals, in order, with a NULL context
RW, RH = 8, 8
SPAN = RW * RH * 3 * 8
BASE = 0x100000
BUFS = [C.c_void_p(BASE + i * SPAN) for i in range(2)]  # two ranges side by side, no allocations: nothing reads them


def rects_of(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def weights_of(index=None, value=None):
    arr = (C.c_double * abi.LUMA_WEIGHTS)(*([1.0] * abi.LUMA_WEIGHTS))
    if index is not None:
        arr[index] = value
    return arr


FULL = rects_of((0, 0, RW, RH))
COUNTS = (C.c_uint32 * 2)(4, 4)
OUT = (abi.TileWeighted * 2)()
GOOD = weights_of()
BAD_WEIGHT = "every weight must be finite and >= 0"


def call(L, S=BUFS[0], Q=BUFS[1], w=RW, h=RH, rects=FULL, cnt=COUNTS, n_rects=1, weights=GOOD, out=OUT):
    return L.rmd_tile_weighted_error(None, S, Q, w, h, rects, cnt, n_rects, weights, out)


def refused(L, text, **kw):
    assert call(L, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
    got = (L.rmd_last_error(None) or b"").decode()
    assert got == ("rmd_tile_weighted_error: " + text if text != "null context" else text), (kw, got)


RULES = [  # in the header's order: (the rule's text, arguments that break it and nothing before it)
    ("bad argument", [dict(S=None), dict(Q=None), dict(w=0), dict(h=0), dict(rects=None), dict(cnt=None), dict(weights=None), dict(out=None)]),
    ("accum_sq_dev must not alias accum_dev", [dict(Q=BUFS[0]), dict(Q=C.c_void_p(BASE + SPAN - 8)), dict(S=C.c_void_p(BASE + 8), Q=BUFS[0])]),
    (BAD_WEIGHT, [dict(weights=weights_of(7, -0.5)), dict(weights=weights_of(130, float("nan"))), dict(weights=weights_of(258, float("-inf"))),
                  dict(weights=weights_of(3, -1e-300), n_rects=0)]),
    ("tile rectangle outside the framebuffer", [dict(rects=rects_of((0, 0, RW + 1, RH))), dict(rects=rects_of((4, 4, 4, 5))), dict(rects=rects_of((2**32 - 4, 0, 8, 8))),
                                                dict(rects=rects_of((0, 0, 4, 4), (RW, RH, 1, 0)), n_rects=2)]),
    ("null context", [dict(), dict(n_rects=0), dict(rects=None, cnt=None, weights=None, out=None, n_rects=0), dict(rects=rects_of((3, 3, 0, 2))),
                      dict(rects=rects_of((RW, RH, 0, 0))), dict(rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2),
                      dict(rects=rects_of((1, 1, 3, 3), (1, 1, 3, 3)), n_rects=2),  # overlapping, repeated
                      dict(cnt=(C.c_uint32 * 2)(0, 0)), dict(weights=weights_of(0, 0.0)), dict(weights=weights_of(259, 1.7e308)), dict(weights=weights_of(5, -0.0))]),
]


@pytest.mark.parametrize("text,breaking", RULES, ids=[r[0].replace(" ", "_")[:40] for r in RULES])
def test_every_refusal_has_its_text_and_comes_before_the_context(product_lib, text, breaking):
    for kw in breaking:
        refused(product_lib, text, **kw)


@pytest.mark.parametrize("index", [0, 259])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -1.0], ids=["nan", "inf", "minus_one"])
def test_a_bad_weight_is_refused_wherever_it_stands(product_lib, index, value):
    refused(product_lib, BAD_WEIGHT, weights=weights_of(index, value))
    refused(product_lib, BAD_WEIGHT, weights=weights_of(index, value), rects=rects_of((0, 0, RW + 1, RH)))  # ... before the rects are looked at
    refused(product_lib, "accum_sq_dev must not alias accum_dev", weights=weights_of(index, value), Q=BUFS[0])  # ... and after the aliasing


def test_the_refusals_come_in_the_stated_order(product_lib):
    """One breaking argument of every rule, accumulated from the last rule to the first: the earliest broken rule is the one reported."""
    broken = {}
    for text, breaking in reversed(RULES):
        broken.update(breaking[0])
        refused(product_lib, text, **broken)
    out = (abi.TileWeighted * 2)()
    C.memset(out, 0xAB, C.sizeof(out))
    for kw in (dict(), dict(weights=weights_of(0, -1.0))):  # out_host is untouched by a refused call
        assert call(product_lib, out=out, **kw) == abi.RMD_ERR_INVALID_ARGUMENT
        assert bytes(out) == b"\xab" * C.sizeof(out)


# ---------------------------------------------------------------- (d) the struct
def test_struct_layout_matches_the_c_header(tmp_path):
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "raymond_hip.h"
#define O(f) printf(#f " %zu\n", offsetof(rmd_tile_weighted, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(rmd_tile_weighted));
  printf("weights %u\n", RMD_LUMA_WEIGHTS);
  O(rms); O(mean_weighted_variance); O(mean_luma); O(mean_variance); O(valid); O(invalid);
  return 0; }
"""
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    layout = dict((l.split()[0], int(l.split()[1])) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l.strip())
    assert layout.pop("sizeof") == C.sizeof(abi.TileWeighted) == 40 == render.TILE_WEIGHTED_DTYPE.itemsize == ref.DTYPE.itemsize
    assert layout.pop("weights") == abi.LUMA_WEIGHTS == 260
    assert [name for name, _ in abi.TileWeighted._fields_] == list(layout) == list(render.TILE_WEIGHTED_DTYPE.names) == list(ref.DTYPE.names)
    for name, offset in layout.items():
        assert getattr(abi.TileWeighted, name).offset == offset == render.TILE_WEIGHTED_DTYPE.fields[name][1], name


# ---------------------------------------------------------------- (e) the settings, in both mirrors
def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


BAD_THRESHOLD = "adaptive_display_threshold must be finite and >= 0 (0 = off)"
NEEDS_SPI = "adaptive_display_threshold > 0 needs samples_per_iteration > 0 (the error is checked between passes)"
WITH_ADAPTIVE = "adaptive_display_threshold and adaptive_threshold are mutually exclusive"
WITH_MEASURE = "adaptive_display_threshold cannot be combined with adaptive_measure: the display rule is a measure of its own"
WITH_DUAL = "adaptive_display_threshold cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual"


def test_settings_defaults_and_rules():
    st = settings()
    assert (st.adaptive_display_threshold, st.adaptive_display_exposure, st.adaptive_display_gamma, st.adaptive_display_floor, st.adaptive_display_auto_exposure) == \
        (0.0, 1.0, 2.2, 1.0 / 255.0, False)
    assert abi.ADAPTIVE_MEASURES == ("channel_max", "luma_tile", "luma_pixel") and st.adaptive_measure == "channel_max"  # no new value there
    settings(adaptive_display_threshold=1.0 / 255.0, samples_per_iteration=2)
    settings(adaptive_display_threshold=1.0 / 255.0, samples_per_iteration=2, despike=True, adaptive_display_auto_exposure=True, adaptive_display_exposure=0.5)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=re.escape(BAD_THRESHOLD)):
            settings(adaptive_display_threshold=bad, samples_per_iteration=2)
    with pytest.raises(ValueError, match=re.escape(NEEDS_SPI)):
        settings(adaptive_display_threshold=0.01)
    with pytest.raises(ValueError, match=re.escape(WITH_ADAPTIVE)):
        settings(adaptive_display_threshold=0.01, adaptive_threshold=0.1, samples_per_iteration=2)
    for measure in ("luma_tile", "luma_pixel"):
        with pytest.raises(ValueError, match=re.escape(WITH_MEASURE)):
            settings(adaptive_display_threshold=0.01, adaptive_measure=measure, samples_per_iteration=2)
        settings(adaptive_measure=measure, samples_per_iteration=2)  # the threshold off: the measure stays legal
    for dual_path in (dict(), dict(adaptive_denoised_threshold=0.1), dict(denoise_dual_atrous=True)):
        with pytest.raises(ValueError, match=re.escape(WITH_DUAL)):
            settings(adaptive_display_threshold=0.01, denoise=True, denoise_dual=True, samples_per_iteration=2, **dual_path)
    for name, text in (("adaptive_display_exposure", "must be finite and > 0"), ("adaptive_display_gamma", "must be finite and > 0")):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=re.escape(name + " " + text)):
                settings(**{name: bad})
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=re.escape("adaptive_display_floor must be finite and in (0, 1)")):
            settings(adaptive_display_floor=bad)
    st = settings(adaptive_display_threshold=0.01, samples_per_iteration=2)
    st.adaptive_threshold = 0.1
    with pytest.raises(ValueError, match=re.escape(WITH_ADAPTIVE)):
        render.render_tiled(scenes.reflective_spheres(), st)  # render_tiled asks, before it opens a device
    st = settings(denoise=True, denoise_dual=True, samples_per_iteration=2)
    st.adaptive_display_threshold = 0.01
    with pytest.raises(ValueError, match=re.escape(WITH_DUAL)):
        render.render_tiled(scenes.reflective_spheres(), st)


def test_cli_parses_the_flags_and_holds_the_rules_in_the_same_words(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    base = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]
    for extra, word in ((["--adaptive-display", "-0.001", "--spi", "2"], BAD_THRESHOLD),
                        (["--adaptive-display", "nan", "--spi", "2"], BAD_THRESHOLD),
                        (["--adaptive-display", "0.01"], NEEDS_SPI),
                        (["--adaptive-display", "0.01", "--adaptive", "0.1", "--spi", "2"], WITH_ADAPTIVE),
                        (["--adaptive-display", "0.01", "--adaptive-measure", "luma_tile", "--spi", "2"], WITH_MEASURE),
                        (["--adaptive-display", "0.01", "--denoise", "1", "--denoise-dual", "1", "--spi", "2"], WITH_DUAL),
                        (["--adaptive-display", "0.01", "--spi", "2", "--adaptive-display-exposure", "0"], "adaptive_display_exposure must be finite and > 0"),
                        (["--adaptive-display", "0.01", "--spi", "2", "--adaptive-display-gamma", "-1"], "adaptive_display_gamma must be finite and > 0"),
                        (["--adaptive-display", "0.01", "--spi", "2", "--adaptive-display-floor", "1"], "adaptive_display_floor must be finite and in (0, 1)")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    source = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read()
    usage = source[: source.index("#include")]
    for flag in ("--adaptive-display T", "--adaptive-display-exposure E", "--adaptive-display-gamma G", "--adaptive-display-floor F", "--adaptive-display-auto-exposure 1",
                 "raymond_cli tile-weighted-error"):
        assert flag in usage, flag
    header = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.hpp")).read()
    assert 'std::string adaptive_measure = "channel_max";' in header  # untouched
    for line in ("double adaptive_display_threshold = 0.0;", "double adaptive_display_exposure = 1.0;", "double adaptive_display_gamma = 2.2;",
                 "double adaptive_display_floor = 1.0 / 255.0;", "bool adaptive_display_auto_exposure = false;"):
        assert line in header, line
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    python = open(os.path.join(ROOT, "raymond_amd", "scene.py")).read()
    for words in (BAD_THRESHOLD, NEEDS_SPI, WITH_ADAPTIVE, WITH_MEASURE, WITH_DUAL):
        assert words in mirror and words in python, words


# ---------------------------------------------------------------- (f) what the measure is for, as arithmetic
def flat_tile(y, rel, n=16, side=32):
    """A tile whose every pixel has the grey mean y and a relative standard error of the mean `rel` in every channel at count n."""
    n = np.float64(n)
    s = np.float64(y) * n
    var_of_mean = (np.float64(rel) * np.float64(y)) ** 2  # = (q - s^2 / n) / (n - 1) / n
    q = var_of_mean * n * (n - 1.0) + s * s / n
    return np.full((side, side, 3), s), np.full((side, side, 3), q)


def test_equal_relative_error_weighs_bright_in_radiance_and_dark_on_the_display():
    """Two tiles at n = 16 with equal relative luminance error, one at Y = 0.01 and one at Y = 4, and saturated ones.
    The issue asked for rms EXACTLY 0 at Y = 40 and, of the same table, for 94 zero bins; the formula cannot give both: the 94 zeros begin where the
    slope's square underflows, at the bin [384, 448), while Y = 40 lies in bin 149, whose weight is (exp(-44) / 2.2)^2 = 1.2e-39.  Measured here: rms
    1.58e-16 at Y = 40 — the displayed value (1 - exp(-40))^(1 / 2.2) is exactly 1.0 in binary64, and the rms is under 2^-52 of the display's scale.  So
    Y = 40 is held to rms < 2^-52 with a positive variance, and exactly 0 is held at Y = 400, inside the zero bins."""
    rect, n = [(0, 0, 32, 32)], [16]
    dark, bright, burnt, white = flat_tile(0.01, 0.05), flat_tile(4.0, 0.05), flat_tile(40.0, 0.05), flat_tile(400.0, 0.05)
    ones = np.ones(ref.N_WEIGHTS)
    a, b = (ref.tile_weighted_error(*t, rect, n, ones)[0] for t in (dark, bright))
    assert a["valid"] == b["valid"] == 1024 and abs(a["mean_luma"] / 0.01 - 1.0) < 1e-12 and abs(b["mean_luma"] / 4.0 - 1.0) < 1e-12
    assert abs(b["rms"] / a["rms"] / 400.0 - 1.0) < 1e-9  # all-ones weights: the absolute error, 400 times larger on the bright tile
    for weights in (ref.display_weights(1.0, 2.2, 1.0 / 255.0)[0],):
        a, b, c = (ref.tile_weighted_error(*t, rect, n, weights)[0] for t in (dark, bright, burnt))
        print("displayed rms: dark", a["rms"], "bright", b["rms"], "ratio", a["rms"] / b["rms"], "burnt", c["rms"])
        assert a["rms"] > b["rms"] > 0.0  # under the tone curve the dark tile's error is the larger one
        assert c["valid"] == 1024 and c["mean_variance"] > 1.0 and c["rms"] < 2.0**-52  # Y = 40 displays white: its noise is not seen
        d = ref.tile_weighted_error(*white, rect, n, weights)[0]
        assert d["valid"] == 1024 and d["mean_variance"] > 100.0 and ref.same_bits(d["rms"], 0.0)  # Y = 400: the weight is exactly 0


def test_the_library_gives_the_restatements_ratio(cli, tmp_path):
    rect, n = [(0, 0, 32, 32)], [16]
    weights = render.display_weights(1.0, 2.2, 1.0 / 255.0)
    got, want = [], []
    for tile in (flat_tile(0.01, 0.05), flat_tile(4.0, 0.05), flat_tile(40.0, 0.05), flat_tile(400.0, 0.05)):
        got.append(run_cli(cli, tmp_path, *tile, rect, n, weights)[0])
        want.append(ref.tile_weighted_error(*tile, rect, n, weights)[0])
        assert got[-1].tobytes() == want[-1].tobytes()
    ratio = got[0]["rms"] / got[1]["rms"]
    print("dark over bright", ratio)
    assert ratio > 1.0 and ratio == want[0]["rms"] / want[1]["rms"] and got[2]["rms"] < 2.0**-52 and ref.same_bits(got[3]["rms"], 0.0)


# ---------------------------------------------------------------- (g) the GPU test's frame classes are what they name
def test_the_frame_classes_are_what_they_name():
    fr = frames.frames()
    tables = frames.tables()
    rects, counts = frames.rects_and_counts(frames.RECTS)
    assert all(l + w <= frames.W and t + h <= frames.H for (l, t, w, h) in rects)
    shapes = sorted((w, h) for (_, _, w, h) in rects)
    for want in ((1, 1), (16, 16), (17, 15), (32, 32), (33, 31)):
        assert want in shapes
    assert len(rects) == 16 and sorted(w * h for (_, _, w, h) in rects)[4:7] == [63, 64, 65] and (frames.W, frames.H) == (67, 45) and {1, 2, 3, 17, 2**32 - 1} == set(counts)
    assert sorted((w, h) for (_, _, w, h), _ in frames.WIDE_RECTS)[1:] == [(1, 257), (255, 1)] and frames.WIDE == 300
    lit = [j for j, ((_, _, w, h), c) in enumerate(zip(rects, counts)) if w * h and c >= 2]

    def counters(name, j):
        (l, t, w, h), c = rects[j], counts[j]
        S, Q = fr[name]
        valid, Y, V, _ = ref.pixels(S[t : t + h, l : l + w], Q[t : t + h, l : l + w], c, tables["ones"])
        return valid, ref.counter(Y), Y, V

    S, Q = fr["random"]
    assert (S > 0).all() and np.isfinite(S).all() and np.isfinite(Q).all()
    base = ref.tile_weighted_error(S, Q, rects, counts, tables["ones"])
    for j, ((l, t, w, h), c) in enumerate(zip(rects, counts)):
        if w * h == 0:
            assert tuple(base[j]) == (0.0, 0.0, 0.0, 0.0, 0, 0)
        elif c == 1:
            assert base[j]["valid"] == 0 and base[j]["invalid"] == w * h and base[j]["rms"] == np.inf and base[j]["mean_luma"] == 0.0
        else:
            assert base[j]["valid"] == w * h and 0 < base[j]["rms"] < np.inf and ref.same_bits(base[j]["mean_weighted_variance"], base[j]["mean_variance"])
    for j in lit:
        valid, k, _, _ = counters("random", j)
        assert valid.all() and (k < 256).all()
        for name, side in (("tiny", ref.BELOW), ("huge", ref.ABOVE), ("saturated", ref.ABOVE)):
            valid, k, _, _ = counters(name, j)
            assert valid.all() and (k == side).all(), (name, j)  # every pixel falls in `below` / `above`

    # the one-bin table proves the lookup index: the bin is reached in some rects and not by every pixel, and a table shifted by one bin gives other sums
    one = ref.tile_weighted_error(S, Q, rects, counts, tables["one_bin"])
    valid, k, _, _ = counters("random", frames.BAD_RECT)
    assert 0 < (k == frames.ONE_BIN).sum() < len(k) and 0 < one[frames.BAD_RECT]["rms"] < base[frames.BAD_RECT]["rms"] * np.sqrt(3.0)
    shifted = np.roll(tables["one_bin"], 1)
    assert not ref.same_bits(ref.tile_weighted_error(S, Q, rects, counts, shifted)["mean_weighted_variance"], one["mean_weighted_variance"])

    # edges: in the 16 x 16 rect at count 2 every luminance is exactly a bin's lower edge or the double under it, and each lands in its own bin
    targets = frames.edge_targets()
    print("edge targets", len(targets), "of", 2 * 257)
    assert len(targets) >= 480 and {i for i, _, _, _ in targets} == set(range(257))
    both = {i for i, u, _, _ in targets if u == 0} & {i for i, u, _, _ in targets if u == 1}
    assert len(both) >= 220  # a seam: two pixels one ulp apart across a bin edge
    for i, under, target, (c, u) in targets:
        assert frames.WEIGHTS[c] * u == target
        k = int(ref.counter(np.array([target]))[0])
        assert k == ((i if i < 256 else ref.ABOVE) if not under else (i - 1 if i > 0 else ref.BELOW)), (i, under)
    assert counts[frames.SEAM_RECT] == 2 and rects[frames.SEAM_RECT][2:] == (16, 16)
    valid, k, Y, V = counters("edges", frames.SEAM_RECT)
    planted = {float(t) for _, _, t, _ in targets}
    assert valid.all() and (V > 0).all() and all(float(y) in planted for y in Y)
    by_bits = {float(y): int(kk) for y, kk in zip(Y, k)}
    seams = [(y, np.nextafter(y, 0.0)) for y in by_bits if float(np.nextafter(y, 0.0)) in by_bits]
    assert len(seams) >= 20 and all(by_bits[float(a)] != by_bits[float(b)] for a, b in seams)  # one ulp apart, different bins
    assert ref.BELOW in by_bits.values() or ref.ABOVE in set(ref.counter(np.array([t for _, _, t, _ in targets])))

    # zeros: zeros of both signs land in `zero`, negative sums in `negative`, all valid
    s, q = fr["zeros"]
    assert (s == 0).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all() and (s < 0).any()
    valid, k, Y, _ = counters("zeros", frames.BAD_RECT)
    assert valid.all() and (k == ref.ZERO).sum() == 512 and np.signbit(Y[k == ref.ZERO]).any() and (k == ref.NEGATIVE).sum() == 256 and (k < 256).sum() == 256
    z = np.zeros(ref.N_WEIGHTS)
    z[ref.ZERO] = 1.0
    assert ref.tile_weighted_error(s, q, rects, counts, z)[frames.BAD_RECT]["rms"] == 0.0  # (a pixel of zeros has no variance either)
    z[ref.NEGATIVE] = 1.0
    assert ref.tile_weighted_error(s, q, rects, counts, z)[frames.BAD_RECT]["rms"] > 0.0

    # saturated: valid pixels with the largest V finite sums give, under a zero weight -> exactly 0; under 1e30 the product overflows -> +inf, not NaN
    s, q = fr["saturated"]
    valid, k, _, V = counters("saturated", frames.BAD_RECT)
    assert valid.all() and (V > 1e305).all() and np.isfinite(V).all()  # (count 17)
    valid, k, _, V = counters("saturated", frames.SEAM_RECT)
    assert valid.all() and (V > 4e307).all() and np.isfinite(V).all()  # (count 2: 0.56 q / 2, the largest there is)
    for table in ("display_1", "zero", "one_bin"):
        assert tables[table][ref.ABOVE] == 0.0
        got = ref.tile_weighted_error(s, q, rects, counts, tables[table])
        assert ref.same_bits(got["rms"][lit], np.zeros(len(lit))) and (got["mean_variance"][lit] > 1e280).all() and (got["valid"][lit] > 0).all()
    got = ref.tile_weighted_error(s, q, rects, counts, tables["big"])
    assert (got["rms"][lit] == np.inf).all() and (got["mean_weighted_variance"][lit] == np.inf).all() and (got["invalid"][lit] == 0).all()

    bx, by = frames.BAD_PIXEL
    for name, which in (("nan_in_S", 0), ("inf_in_Q", 1)):
        pair = fr[name]
        bad = ~np.isfinite(pair[which])
        assert bad.sum() == 1 and bad[by, bx].any() and np.isfinite(pair[1 - which]).all()
        got = ref.tile_weighted_error(*pair, rects, counts, tables["ones"])
        one_rect = got[frames.BAD_RECT]
        assert one_rect["invalid"] == 1 and one_rect["valid"] == 1023 and one_rect["rms"] == np.inf and 0 < one_rect["mean_luma"] < np.inf and 0 < one_rect["mean_variance"] < np.inf
        others = [j for j in range(len(rects)) if j != frames.BAD_RECT]
        assert np.array_equal(got[others], base[others])

    # the tables: a fifth of the random one is 0, the tone curve's has its 94 zeros, every entry is one the entry point accepts
    assert (tables["random"] == 0).sum() > 20 and (tables["display_1"][:256] == 0).sum() == 94 and (tables["display_0.001"][:256] == 0).sum() < 94
    for name, table in tables.items():
        assert table.shape == (260,) and np.isfinite(table).all() and (table >= 0).all(), name

    # the order matters: the same pixels permuted inside the 32 x 32 tile give other bits
    S2, Q2 = frames.permuted_tile(S, Q, rects[frames.BAD_RECT], seed=frames.ORDER_SEED)
    for table in ("ones", "random"):
        moved = ref.tile_weighted_error(S2, Q2, [rects[frames.BAD_RECT]], [17], tables[table])[0]
        there = ref.tile_weighted_error(S, Q, [rects[frames.BAD_RECT]], [17], tables[table])[0]
        assert not ref.same_bits(moved["mean_weighted_variance"], there["mean_weighted_variance"]), table
        assert abs(moved["mean_weighted_variance"] / there["mean_weighted_variance"] - 1.0) < 1e-13
