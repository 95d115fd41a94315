"""rmd_tile_luma_error: the parts that need no GPU.

tests/tile_luma_ref.py — the numpy restatement the device is held to (tests/test_gpu_tile_luma.py) — is held here to the rule header the kernel is built from,
through the C++ mirror's host function (raymond_cli tile-luma-error), bit for bit in all seven fields; the rule header passes tests/tile_luma_rule_main.cpp
under the host sanitizers; the entry point's refusals come in the header's order with a NULL context; rmd_tile_luma has abi.TileLuma's layout; both mirrors
hold the settings' rules; the case the measure exists for is stated as arithmetic; and each frame class of the GPU test is what it names."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tile_luma_frames as frames
import tile_luma_ref as ref
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


# ---------------------------------------------------------------- the boundary
def test_entry_point_is_exported_declared_and_clear_of_the_traced_prefixes(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "rmd_tile_luma_error" in set(re.findall(r" T (\w+)", out))
    assert len(lib.SIGNATURES["rmd_tile_luma_error"][1]) == 10
    assert not "rmd_tile_luma_error".startswith(("rmd_tile_error", "rmd_denoise", "rmd_despike", "rmd_resolve", "rmd_luminance", "rmd_exposure"))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_tile_luma_error(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_counts, uint32_t n_rects, double floor, rmd_tile_luma *out_host);") in header
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # an addition within ABI 6
    for meaning in ("tile_rms is the RMS standard error of the tile's luminance over the tile's own mean luminance",
                    "pixel_rms is the RMS over the tile of each pixel's relative luminance error", "R = (V / d) / d", "(w0 + w1) + (w2 + w3)"):
        assert meaning in header, meaning


# ---------------------------------------------------------------- (a) the rule header through the C++ mirror is the restatement, bit for bit
def run_cli(cli, tmp_path, S, Q, rects, counts, floor):
    Hf, Wf = S.shape[:2]
    S.tofile(tmp_path / "S.f64"), Q.tofile(tmp_path / "Q.f64")
    with open(tmp_path / "rects.txt", "w") as f:
        for (l, t, w, h), c in zip(rects, counts):
            f.write("%d %d %d %d %d\n" % (l, t, w, h, c))
    r = subprocess.run([cli, "tile-luma-error", str(tmp_path / "S.f64"), str(tmp_path / "Q.f64"), str(Wf), str(Hf), str(tmp_path / "rects.txt"), float(floor).hex()],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.zeros(len(rects), dtype=ref.DTYPE)
    lines = r.stdout.strip().split("\n") if rects else []
    assert len(lines) == len(rects)
    for j, line in enumerate(lines):
        v = line.split()
        out[j] = tuple(float(x) for x in v[:5]) + (int(v[5]), int(v[6]))  # (%.17g round-trips a binary64; inf and nan parse)
    return out


def assert_same_fields(got, want, exact=ref.FLOAT_FIELDS):
    assert list(got["valid"]) == list(want["valid"]) and list(got["invalid"]) == list(want["invalid"])
    for name in exact:
        assert ref.same_bits(got[name], want[name]), (name, got[name], want[name])


@pytest.mark.parametrize("name", ["random", "tiny", "huge", "clamped", "negative", "nan_in_S", "inf_in_Q"])
def test_the_cpp_mirrors_host_function_is_the_restatement(cli, tmp_path, name):
    S, Q = frames.frames()[name]
    rects, counts = frames.rects_and_counts(frames.RECTS)
    for floor in (frames.FLOOR, 0.75):
        want = ref.tile_luma_error(S, Q, rects, counts, floor)
        assert_same_fields(run_cli(cli, tmp_path, S, Q, rects, counts, floor), want)  # all seven fields: both sides are host code, the square root included
    assert not any(np.isnan(want[f]).any() for f in ref.FLOAT_FIELDS)


def test_the_cpp_mirrors_host_function_on_the_wide_frame_and_on_no_rects(cli, tmp_path):
    S, Q = frames.random_positive(frames.WIDE, frames.WIDE, seed=3)
    rects, counts = frames.rects_and_counts(frames.WIDE_RECTS)
    assert_same_fields(run_cli(cli, tmp_path, S, Q, rects, counts, frames.FLOOR), ref.tile_luma_error(S, Q, rects, counts, frames.FLOOR))
    assert len(run_cli(cli, tmp_path, S, Q, [], [], frames.FLOOR)) == 0


def test_the_rule_header_agrees_with_a_plain_reading_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "tile_luma_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h", "despike_rule.hpp", "tile_reduce.hpp"]  # nothing else of the project, nothing of HIP
    order = open(os.path.join(CSRC, "tile_reduce.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", order) == ["stdint.h"]
    kernel = open(os.path.join(CSRC, "tile_luma.hip")).read()
    for fn in ("tile_luma_add(", "tile_luma_final(", "tile_sums_combine(", "__launch_bounds__(256)"):
        assert fn in kernel, fn  # the kernel reads the same lines
    for fn in ("__shfl_xor(", "__syncthreads()", "tile_sums_combine(", "tile_rect_sums_host("):
        assert fn in order, fn  # ... and takes the order its sums are added in from where the host emulation takes it
    assert "tile_rect_sums_host(" in header
    assert "asm" not in kernel and "atomic" not in kernel.replace("No atomics", "") and "asm" not in order and "atomic" not in order
    assert "tile_luma_pixel(" in header and "despike_pixel(" in header
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/tile_luma_rule.hpp"' in mirror and "rmd::tile_luma_rect_host(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "tile_luma_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "tile_luma_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "1", "10000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"tile luma rule ok: (\d+) rects, (\d+) empty, (\d+) with an invalid pixel, (\d+) all valid, (\d+) of them with every variance clamped", r.stdout)
    assert m and int(m.group(1)) == 10000 and all(int(m.group(i)) > 100 for i in range(2, 6))


# ---------------------------------------------------------------- (b) the refusals, in order, with a NULL context
RW, RH = 8, 8
SPAN = RW * RH * 3 * 8
BASE = 0x100000
BUFS = [C.c_void_p(BASE + i * SPAN) for i in range(2)]  # two ranges side by side, no allocations: nothing reads them


def rects_of(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


FULL = rects_of((0, 0, RW, RH))
COUNTS = (C.c_uint32 * 2)(4, 4)
OUT = (abi.TileLuma * 2)()


def call(L, S=BUFS[0], Q=BUFS[1], w=RW, h=RH, rects=FULL, cnt=COUNTS, n_rects=1, floor=1e-3, out=OUT):
    return L.rmd_tile_luma_error(None, S, Q, w, h, rects, cnt, n_rects, floor, out)


def refused(L, text, **kw):
    assert call(L, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
    got = (L.rmd_last_error(None) or b"").decode()
    assert got == ("rmd_tile_luma_error: " + text if text != "null context" else text), (kw, got)


RULES = [  # in the header's order: (the rule's text, arguments that break it and nothing before it)
    ("bad argument", [dict(S=None), dict(Q=None), dict(w=0), dict(h=0), dict(rects=None), dict(cnt=None), dict(out=None)]),
    ("accum_sq_dev must not alias accum_dev", [dict(Q=BUFS[0]), dict(Q=C.c_void_p(BASE + SPAN - 8)), dict(S=C.c_void_p(BASE + 8), Q=BUFS[0])]),
    ("floor must be finite and > 0", [dict(floor=0.0), dict(floor=-1e-3), dict(floor=float("nan")), dict(floor=float("inf"))]),
    ("tile rectangle outside the framebuffer", [dict(rects=rects_of((0, 0, RW + 1, RH))), dict(rects=rects_of((4, 4, 4, 5))), dict(rects=rects_of((2**32 - 4, 0, 8, 8))),
                                                dict(rects=rects_of((0, 0, 4, 4), (RW, RH, 1, 0)), n_rects=2)]),
    ("null context", [dict(), dict(n_rects=0), dict(rects=None, cnt=None, out=None, n_rects=0), dict(rects=rects_of((3, 3, 0, 2))), dict(rects=rects_of((RW, RH, 0, 0))),
                      dict(rects=rects_of((0, 0, 5, 5), (4, 4, 4, 4)), n_rects=2), dict(rects=rects_of((1, 1, 3, 3), (1, 1, 3, 3)), n_rects=2),  # overlapping, repeated
                      dict(cnt=(C.c_uint32 * 2)(0, 0)), dict(floor=5e-324)]),
]


@pytest.mark.parametrize("text,breaking", RULES, ids=[r[0].replace(" ", "_")[:40] for r in RULES])
def test_every_refusal_has_its_text_and_comes_before_the_context(product_lib, text, breaking):
    for kw in breaking:
        refused(product_lib, text, **kw)


def test_the_refusals_come_in_the_stated_order(product_lib):
    """One breaking argument of every rule, accumulated from the last rule to the first: the earliest broken rule is the one reported."""
    broken = {}
    for text, breaking in reversed(RULES):
        broken.update(breaking[0])
        refused(product_lib, text, **broken)
    out = (abi.TileLuma * 2)()
    C.memset(out, 0xAB, C.sizeof(out))
    for kw in (dict(), dict(floor=0.0)):  # out_host is untouched by a refused call
        assert call(product_lib, out=out, **kw) == abi.RMD_ERR_INVALID_ARGUMENT
        assert bytes(out) == b"\xab" * C.sizeof(out)


# ---------------------------------------------------------------- (c) the struct
def test_struct_layout_matches_the_c_header(tmp_path):
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "raymond_hip.h"
#define O(f) printf(#f " %zu\n", offsetof(rmd_tile_luma, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(rmd_tile_luma));
  O(tile_rms); O(pixel_rms); O(mean_luma); O(mean_variance); O(mean_rel_variance); O(valid); O(invalid);
  return 0; }
"""
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    layout = dict((l.split()[0], int(l.split()[1])) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l.strip())
    assert layout.pop("sizeof") == C.sizeof(abi.TileLuma) == 48 == render.TILE_LUMA_DTYPE.itemsize == ref.DTYPE.itemsize
    assert [name for name, _ in abi.TileLuma._fields_] == list(layout) == list(render.TILE_LUMA_DTYPE.names) == list(ref.DTYPE.names)
    for name, offset in layout.items():
        assert getattr(abi.TileLuma, name).offset == offset == render.TILE_LUMA_DTYPE.fields[name][1], name


# ---------------------------------------------------------------- (d) the settings, in both mirrors
def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


BAD_MEASURE = 'adaptive_measure must be "channel_max", "luma_tile" or "luma_pixel"'
WITH_DUAL = "adaptive_measure cannot be combined with denoise_dual: the dual loop's check is rmd_tile_error_dual"


def test_settings_defaults_and_rules():
    assert settings().adaptive_measure == "channel_max" and abi.ADAPTIVE_MEASURES == ("channel_max", "luma_tile", "luma_pixel")
    for name in abi.ADAPTIVE_MEASURES:
        assert settings(adaptive_measure=name).adaptive_measure == name  # (checked and kept whether or not adaptive sampling is on)
        settings(adaptive_measure=name, adaptive_threshold=0.1, samples_per_iteration=2)
        settings(adaptive_measure=name, adaptive_threshold=0.1, samples_per_iteration=2, despike=True)
    for bad in ("luma", "", "LUMA_TILE", None, 1, b"luma_tile"):
        with pytest.raises(ValueError, match=re.escape(BAD_MEASURE)):
            settings(adaptive_measure=bad)
    for measure in ("luma_tile", "luma_pixel"):
        for dual_path in (dict(), dict(adaptive_denoised_threshold=0.1), dict(denoise_dual_atrous=True)):
            with pytest.raises(ValueError, match=re.escape(WITH_DUAL)):
                settings(adaptive_measure=measure, denoise=True, denoise_dual=True, samples_per_iteration=2, **dual_path)
    settings(denoise=True, denoise_dual=True, samples_per_iteration=2)  # the default measure stays legal there
    st = settings(adaptive_threshold=0.1, samples_per_iteration=2)
    st.adaptive_measure = "worst"
    with pytest.raises(ValueError, match=re.escape(BAD_MEASURE)):
        render.render_tiled(scenes.reflective_spheres(), st)  # render_tiled asks, before it opens a device
    st = settings(denoise=True, denoise_dual=True, samples_per_iteration=2)
    st.adaptive_measure = "luma_pixel"
    with pytest.raises(ValueError, match=re.escape(WITH_DUAL)):
        render.render_tiled(scenes.reflective_spheres(), st)


def test_cli_parses_the_flag_and_holds_the_rules_in_the_same_words(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    base = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]
    for extra, word in ((["--adaptive-measure", "luma"], BAD_MEASURE),
                        (["--adaptive-measure", ""], BAD_MEASURE),
                        (["--adaptive", "0.1", "--spi", "2", "--adaptive-measure", "LUMA_TILE"], BAD_MEASURE),
                        (["--adaptive-measure", "luma_tile", "--denoise", "1", "--denoise-dual", "1", "--spi", "2"], WITH_DUAL),
                        (["--adaptive-measure", "luma_pixel", "--denoise", "1", "--denoise-dual", "1", "--spi", "2", "--adaptive-denoised", "0.1"], WITH_DUAL)):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    header = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.hpp")).read()
    assert 'std::string adaptive_measure = "channel_max";' in header


# ---------------------------------------------------------------- (e) the case the feature exists for, as arithmetic
@pytest.mark.parametrize("x", [1e-12, 1e-6, 1e-3, 0.25, 1.0])
def test_a_dim_channel_lit_by_one_sample_holds_the_worst_channel_rule_and_not_the_luminance(x):
    """A 32 x 32 tile at n = 16 whose every pixel has S = (8, 8, x) and Q = (4.2, 4.2, x^2): red and green are well sampled, blue has x in exactly one
    sample.  The worst-channel relative error is 1 whatever x > 0 is — the tile never finishes at a threshold below 1 — while both luminance measures sit
    below 0.1: blue carries 0.0722 x of a luminance near 0.43."""
    n = np.float64(16.0)
    S = np.tile(np.array([8.0, 8.0, x]), (32, 32, 1))
    Q = np.tile(np.array([4.2, 4.2, x * x]), (32, 32, 1))
    # the three lines: mean, variance of the mean, relative standard error per channel (rmd_tile_error's floor under |mean| would only lower it for x < 0.016)
    mean = S / n
    var_of_mean = np.maximum(0.0, (Q - S * mean) / (n - 1.0)) / n
    rel = np.sqrt(var_of_mean) / np.abs(mean)
    assert abs(rel[..., 2].max() - 1.0) < 1e-12 and rel[..., :2].max() < 0.06  # sqrt((x^2 - x^2 / 16) / 15 / 16) / (x / 16) = 1
    got = ref.tile_luma_error(S, Q, [(0, 0, 32, 32)], [16], 1e-3)[0]
    assert got["valid"] == 1024 and got["invalid"] == 0
    assert 0.0 < got["tile_rms"] < 0.1 and 0.0 < got["pixel_rms"] < 0.1, (got["tile_rms"], got["pixel_rms"])
    assert abs(got["tile_rms"] / got["pixel_rms"] - 1.0) < 1e-12  # (every pixel alike: the two normalisations coincide, up to the sums' rounding)


# ---------------------------------------------------------------- (f) the GPU test's frame classes are what they name
def test_the_frame_classes_are_what_they_name():
    fr = frames.frames()
    rects, counts = frames.rects_and_counts(frames.RECTS)
    assert all(l + w <= frames.W and t + h <= frames.H for (l, t, w, h) in rects)
    assert all(l + w <= frames.WIDE and t + h <= frames.WIDE for (l, t, w, h), _ in frames.WIDE_RECTS)
    shapes = sorted((w, h) for (_, _, w, h) in rects)
    for want in ((1, 1), (16, 16), (17, 15), (32, 32), (33, 31)):
        assert want in shapes
    assert sorted((w, h) for (_, _, w, h), _ in frames.WIDE_RECTS)[1:] == [(1, 257), (255, 1)]
    assert any(w * h == 0 for (_, _, w, h) in rects) and any(l + w == frames.W and t + h == frames.H and w * h for (l, t, w, h) in rects)
    assert rects.count((40, 36, 9, 9)) == 2 and {2, 3, 17, frames.NMAX, 1} == set(counts)
    (a, b) = ((8, 8, 20, 12), (18, 14, 20, 12))
    assert a in rects and b in rects and a[0] < b[0] < a[0] + a[2] and a[1] < b[1] < a[1] + a[3]  # they overlap
    bx, by = frames.BAD_PIXEL
    holds = [j for j, (l, t, w, h) in enumerate(rects) if l <= bx < l + w and t <= by < t + h]
    assert holds == [frames.BAD_RECT] and rects[frames.BAD_RECT][2:] == (32, 32)

    S, Q = fr["random"]
    assert (S > 0).all() and (Q > S * S / 2.0).all() and np.isfinite(S).all() and np.isfinite(Q).all()
    base = ref.tile_luma_error(S, Q, rects, counts, frames.FLOOR)
    for j, ((l, t, w, h), c) in enumerate(zip(rects, counts)):
        if w * h == 0:
            assert tuple(base[j]) == (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
        elif c == 1:  # the count of 1: every pixel invalid, the errors +inf, the means 0
            assert base[j]["valid"] == 0 and base[j]["invalid"] == w * h and base[j]["tile_rms"] == np.inf == base[j]["pixel_rms"] and base[j]["mean_luma"] == 0.0
        else:
            assert base[j]["valid"] == w * h and base[j]["invalid"] == 0 and base[j]["mean_variance"] > 0 and 0 < base[j]["tile_rms"] < np.inf and base[j]["mean_luma"] > 0
    assert tuple(base[10]) == tuple(base[11])  # the rect given twice
    lit = [j for j, ((_, _, w, h), c) in enumerate(zip(rects, counts)) if w * h and c >= 2]

    for name, scale in (("tiny", -500), ("huge", 500)):
        s, q = fr[name]
        assert ref.same_bits(s, np.ldexp(S, scale)) and ref.same_bits(q, np.ldexp(Q, 2 * scale)) and np.isfinite(q).all() and (q > 0).all()
        got = ref.tile_luma_error(s, q, rects, counts, frames.FLOOR)
        assert (np.abs(got["mean_luma"][lit]) < 2.0**-490).all() if scale < 0 else (got["mean_luma"][lit] > 2.0**460).all()  # (at the count 2^32 - 1 a mean is 2^-28 of its sum)
        if scale > 0:  # the relative measures do not see a scale that is a power of two, above the floor
            above = [j for j in lit if counts[j] <= 17]  # (at 2^32 - 1 the unscaled frame's means lie below the floor)
            assert ref.same_bits(got["tile_rms"][above], base["tile_rms"][above]) and ref.same_bits(got["pixel_rms"][above], base["pixel_rms"][above])
        else:  # below the floor the floor divides
            assert (got["tile_rms"][lit] < 2.0**-480).all()

    s, q = fr["clamped"]
    assert (q < s * s / np.float64(frames.NMAX)).all()
    got = ref.tile_luma_error(s, q, rects, counts, frames.FLOOR)
    assert (got["mean_variance"][lit] == 0).all() and (got["tile_rms"][lit] == 0).all() and (got["pixel_rms"][lit] == 0).all() and (got["invalid"][lit] == 0).all()

    s, q = fr["negative"]
    assert (s < 0).all()
    got = ref.tile_luma_error(s, q, rects, counts, frames.FLOOR)
    assert (got["mean_luma"][lit] < 0).all() and ref.same_bits(got["tile_rms"][lit], base["tile_rms"][lit]) and ref.same_bits(got["mean_variance"][lit], base["mean_variance"][lit])

    for name, which in (("nan_in_S", 0), ("inf_in_Q", 1)):
        pair = fr[name]
        bad = ~np.isfinite(pair[which])
        assert bad.sum() == 1 and bad[by, bx].any() and np.isfinite(pair[1 - which]).all()
        assert np.isnan(pair[0][by, bx, 1]) if which == 0 else pair[1][by, bx, 2] == np.inf
        got = ref.tile_luma_error(*pair, rects, counts, frames.FLOOR)
        one = got[frames.BAD_RECT]
        assert one["invalid"] == 1 and one["valid"] == 1023 and one["tile_rms"] == np.inf == one["pixel_rms"] and 0 < one["mean_luma"] < np.inf and 0 < one["mean_variance"] < np.inf
        others = [j for j in range(len(rects)) if j != frames.BAD_RECT]
        assert np.array_equal(got[others], base[others])

    # the order matters: the same pixels permuted inside the 32 x 32 tile give other bits
    S2, Q2 = frames.permuted_tile(S, Q, rects[frames.BAD_RECT])
    moved = ref.tile_luma_error(S2, Q2, [rects[frames.BAD_RECT]], [17], frames.FLOOR)[0]
    assert not ref.same_bits(moved["mean_variance"], base[frames.BAD_RECT]["mean_variance"])
    assert abs(moved["mean_variance"] / base[frames.BAD_RECT]["mean_variance"] - 1.0) < 1e-13
