"""rmd_despike: the parts that need no GPU.

tests/despike_ref.py — the numpy restatement the device is held to byte for byte (tests/test_gpu_despike.py) — is held here to what it names, on
noise-free frames where every outcome is derivable by hand (tests/despike_frames.py; radius 2, rank 2, k 6, ratio 2, floor 0 unless stated; every pixel
carries a small per-sample variance, so V > 0).  The rule header the kernel is built from passes tests/despike_rule_main.cpp under the host sanitizers and,
through the C++ mirror's host despike (raymond_cli despike), gives the restatement's bytes on random frames.  Both mirrors hold the settings' rules.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import despike_frames as frames
import despike_ref as ref
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
W = H = 12


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def unchanged_except(S, Q, oS, oQ, pixels):
    """Every pixel but `pixels` (x, y) is a bit copy of its input."""
    keep = np.ones(S.shape[:2], dtype=bool)
    for x, y in pixels:
        keep[y, x] = False
    return np.array_equal(bits(S)[keep], bits(oS)[keep]) and np.array_equal(bits(Q)[keep], bits(oQ)[keep])


# ---------------------------------------------------------------- the boundary
def test_entry_point_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "rmd_despike" in set(re.findall(r" T (\w+)", out))
    assert len(lib.SIGNATURES["rmd_despike"][1]) == 16
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    assert ("rmd_status rmd_despike(rmd_context *ctx, const double *accum_dev, const double *accum_sq_dev, uint32_t width, uint32_t height, "
            "const rmd_tile_rect *rects, const uint32_t *rect_sample_counts, uint32_t n_rects, uint32_t radius, uint32_t rank, double k, double ratio, "
            "double floor, double *out_accum_dev, double *out_accum_sq_dev, uint32_t *replaced_host /* n_rects, may be NULL */);") in header
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # an addition within ABI 6
    for consequence in ("is how many brighter others a pixel may have and still be a spike", "survives only if rank < m - 1", "removes energy, so it is BIASED"):
        assert consequence in header


# ---------------------------------------------------------------- the restatement, on frames whose outcome is derivable by hand
def test_constant_frame_has_no_spike():
    """Every Y is the same: e = Y - 1 * Y - 0 = 0, and e > 0 fails on equality — at ratio 1, k 0, floor 0, where anything above it would pass."""
    S, Q, rects, counts = frames.flat(W, H)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, k=0.0, ratio=1.0, floor=0.0)
    assert spikes == [] and list(replaced) == [0] and ref.same_bits(S, oS) and ref.same_bits(Q, oQ)


def test_linear_ramp_has_no_spike():
    """mean = 1 + x / 8: in the interior the two columns to the right hold 10 of the 24 others, all brighter, so the donor (index 2) is brighter and
    e < 0, even at ratio 1 and k 0, where anything above equality passes.  In the last column the others of the same column tie with p and stand first — four
    of them, three in the second row — and e = 0; only its two CORNER pixels have two such others, take a donor from the column before (the first of it in
    raster order) and are spikes at ratio 1, by one step of the ramp.  At ratio 2 nothing is."""
    S, Q, rects, counts = frames.flat(W, H)
    S, Q = frames.sums_of(1.0 + np.arange(W)[None, :] / 8.0 + np.zeros((H, 1)), 16)
    plan = ref.Plan(S, Q, rects, counts, 2, 2)
    for y in range(2, H - 2):
        for x in range(2, W - 2):
            brighter = sum(1 for dy in range(-2, 3) for dx in range(-2, 3) if plan.Y[y + dy, x + dx] > plan.Y[y, x])
            assert brighter == 10
    oS, oQ, replaced, spikes = plan.decide(k=0.0, ratio=1.0, floor=0.0)
    assert spikes == [(W - 1, 0, W - 2, 0), (W - 1, H - 1, W - 2, H - 3)]
    assert unchanged_except(S, Q, oS, oQ, [(W - 1, 0), (W - 1, H - 1)])
    oS, oQ, replaced, spikes = plan.decide()
    assert spikes == [] and ref.same_bits(S, oS) and ref.same_bits(Q, oQ)


def test_an_isolated_spike_takes_its_donors_bits_and_is_counted_in_its_rect():
    """One pixel at 50 among 1s: e = 50 - 2 = 48 > 0 and 48^2 is far above 36 V.  All its others tie at Y = 1, so the order is the raster order of d and the
    donor, index 2, is d = (0, -2).  Its neighbours see one brighter other, have a donor at their own Y, and e = 1 - 2 < 0."""
    S, Q, _, _ = frames.flat(W, H)
    rects, counts = [(0, 0, 6, H), (6, 0, 6, H)], [16, 16]
    frames.plant(S, Q, 7, 5, 50.0)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts)
    assert spikes == [(7, 5, 7, 3)] and list(replaced) == [0, 1]
    assert np.array_equal(bits(oS)[5, 7], bits(S)[3, 7]) and np.array_equal(bits(oQ)[5, 7], bits(Q)[3, 7])
    assert not np.array_equal(bits(Q)[3, 7], bits(Q)[3, 6])  # (the donor's Q is its own: the copy shows which pixel it was)
    assert unchanged_except(S, Q, oS, oQ, [(7, 5)])


def test_adjacent_pairs_stand_at_rank_0_and_fall_at_rank_1():
    """Two pixels at 50 side by side.  rank 0: each one's donor is the other, e = 50 - 100 < 0, both stand.  rank 1: the donor is the first 1 in raster
    order, d = (-2, -2), and both are replaced — each by a pixel of the INPUT: (5, 5) by (3, 3), (6, 5) by (4, 3), whatever became of the other."""
    S, Q, rects, counts = frames.flat(W, H)
    frames.plant(S, Q, 5, 5, 50.0), frames.plant(S, Q, 6, 5, 50.0)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, rank=0)
    assert spikes == [] and ref.same_bits(S, oS) and ref.same_bits(Q, oQ)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, rank=1)
    assert spikes == [(5, 5, 3, 3), (6, 5, 4, 3)] and list(replaced) == [2]
    for (x, y, qx, qy) in spikes:
        assert np.array_equal(bits(oS)[y, x], bits(S)[qy, qx]) and np.array_equal(bits(oQ)[y, x], bits(Q)[qy, qx])
    assert unchanged_except(S, Q, oS, oQ, [(5, 5), (6, 5)])
    # had (6, 5) been decided on a frame in which (5, 5) was already replaced, all its others would tie and its donor would be index 1 of the raster
    # order, (5, 3): it is (4, 3), so the decision saw (5, 5) as the input has it
    assert not np.array_equal(bits(oQ)[5, 6], bits(Q)[3, 5])


def test_a_one_pixel_line_survives_radius_2_and_is_erased_at_radius_1():
    """The documented cost of the rank.  A bright column over the whole height, rank 2.  radius 2: a line pixel sees the line's pixels at dy = -2 .. 2, four
    others as bright as itself — three at least from the second row on —, so its donor is on the line and e = 50 - 100 < 0: it survives; the two END
    pixels see only two and are replaced.  radius 1: two others on the line, the donor is a 1, and the whole line is erased."""
    S, Q, rects, counts = frames.flat(W, H)
    for y in range(H):
        frames.plant(S, Q, 6, y, 50.0)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, radius=2, rank=2)
    assert sorted((x, y) for x, y, _, _ in spikes) == [(6, 0), (6, H - 1)] and list(replaced) == [2]
    for y in range(1, H - 1):
        assert np.array_equal(bits(oS)[y, 6], bits(S)[y, 6]) and np.array_equal(bits(oQ)[y, 6], bits(Q)[y, 6])
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, radius=1, rank=2)
    assert sorted((x, y) for x, y, _, _ in spikes) == [(6, y) for y in range(H)] and list(replaced) == [H]
    assert (oS[:, 6] == 16.0).all()  # every line pixel now holds a background pixel's sums


def test_a_corner_with_too_few_others_is_unchanged():
    """radius 1: the corner pixel has 3 others.  At rank 2 the third is its donor and a 50 there is replaced; at rank 3 it has no donor and stays."""
    S, Q, rects, counts = frames.flat(W, H)
    frames.plant(S, Q, 0, 0, 50.0)
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, radius=1, rank=2)
    assert spikes == [(0, 0, 1, 1)] and np.array_equal(bits(oS)[0, 0], bits(S)[1, 1])
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts, radius=1, rank=3)
    assert spikes == [] and ref.same_bits(S, oS) and ref.same_bits(Q, oQ)


def test_pixels_that_are_not_valid_are_copied_and_never_donors():
    """The spike at (5, 5) would take d = (0, -2), the third other in raster order.  With (3, 3) a NaN pixel and (4, 3) an inf pixel the others start at
    (5, 3) and the donor is (7, 3).  With row 3 under a rect at count 1, or under no rect, the others start in row 4: the donor is (5, 4)."""
    S, Q, rects, counts = frames.flat(W, H)
    frames.plant(S, Q, 5, 5, 50.0)
    S[3, 3, 1] = np.uint64(0x7FF8000000000123).view(np.float64)  # a NaN with a payload
    Q[3, 4, 2] = np.inf
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts)
    assert spikes == [(5, 5, 7, 3)] and np.array_equal(bits(oS)[5, 5], bits(S)[3, 7]) and np.array_equal(bits(oQ)[5, 5], bits(Q)[3, 7])
    assert unchanged_except(S, Q, oS, oQ, [(5, 5)])  # the NaN's payload and the inf included
    S, Q, _, _ = frames.flat(W, H)
    frames.plant(S, Q, 5, 5, 50.0)
    for rects, counts in (([(0, 0, W, 4), (0, 4, W, H - 4)], [1, 16]), ([(0, 4, W, H - 4)], [16]), ([(0, 0, W, 3), (0, 4, W, H - 4)], [16, 16])):
        oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts)
        assert spikes == [(5, 5, 5, 4)] and int(replaced[-1]) == 1 and int(replaced.sum()) == 1
        assert np.array_equal(bits(oS)[5, 5], bits(S)[4, 5]) and unchanged_except(S, Q, oS, oQ, [(5, 5)])


def test_a_donor_at_another_count_gives_its_per_sample_moments_at_the_pixels_count():
    """Rows 0 .. 3 hold 5 samples, the rest 16, every mean 1: all Y tie, the spike at (5, 5) takes d = (0, -2) = (5, 3), a pixel of the other rect."""
    n = np.full((H, W), 16.0)
    n[:4] = 5.0
    s2 = frames.S2 * (1.0 + 1e-3 * np.arange(W * H, dtype=np.float64).reshape(H, W))
    S, Q = frames.sums_of(np.ones((H, W)), n, s2)
    frames.plant(S, Q, 5, 5, 50.0)
    rects, counts = [(0, 0, W, 4), (0, 4, W, H - 4)], [5, 16]
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts)
    assert spikes == [(5, 5, 5, 3)] and list(replaced) == [0, 1]
    for c in range(3):
        assert oS[5, 5, c] == (S[3, 5, c] / np.float64(5.0)) * np.float64(16.0) == 16.0
        assert bits(oQ)[5, 5, c] == bits(np.array((Q[3, 5, c] / np.float64(5.0)) * np.float64(16.0)))
        assert oQ[5, 5, c] != Q[3, 5, c]
    assert unchanged_except(S, Q, oS, oQ, [(5, 5)])


def test_a_negative_donor_luminance_is_where_counting_alone_would_be_wrong():
    """Every mean is -1 but p = (5, 5) at -1.5: all 24 others of p are ABOVE it — counting them, 24 > rank, says "settled" — yet with the donor at -1,
    e = -1.5 - 2 * (-1) = 0.5 > 0 and p is a spike at ratio 2.  (So is every other pixel of this frame, e = -1 + 2 = 1: a negative frame at ratio 2.)"""
    S, Q, rects, counts = frames.flat(W, H, value=-1.0)
    frames.plant(S, Q, 5, 5, -1.5)
    plan = ref.Plan(S, Q, rects, counts, 2, 2)
    assert sum(1 for dy in range(-2, 3) for dx in range(-2, 3) if (dx or dy) and plan.Y[5 + dy, 5 + dx] >= plan.Y[5, 5]) == 24
    oS, oQ, replaced, spikes = plan.decide()
    assert (5, 5, 5, 3) in spikes and np.array_equal(bits(oS)[5, 5], bits(S)[3, 5])
    assert len(spikes) == W * H and list(replaced) == [W * H]
    oS, oQ, replaced, spikes = plan.decide(ratio=1.0)  # at ratio 1 only e = 0 and e = -0.5 are left
    assert spikes == []


def test_the_motivating_tile_converges_once_its_firefly_is_gone():
    """A tile that has converged (relative standard error 2.5e-3) but for one pixel where one of the 16 samples came back as 800: rmd_tile_error is
    held near 1 by that pixel alone, and is back under the threshold on the despiked sums."""
    S, Q, rects, counts = frames.flat(W, H)
    S[6, 4] = 15.0 + 800.0
    Q[6, 4] = 15.0 * (1.0 + frames.S2) + 800.0 * 800.0
    threshold, floor = 0.05, 1e-3
    before = ref.tile_error(S, Q, 16, floor, rects)[0]
    oS, oQ, replaced, spikes = ref.despike(S, Q, rects, counts)
    after = ref.tile_error(oS, oQ, 16, floor, rects)[0]
    assert [(x, y) for x, y, _, _ in spikes] == [(4, 6)] and list(replaced) == [1]
    # (the per-sample variance runs from 1e-4 to 1.143e-4 over the frame: sqrt(s2 / 16) / 1 from 2.5e-3 to 2.673e-3)
    assert before > 0.9 > threshold >= after and 2.5e-3 <= after < 2.7e-3, (before, after)


# ---------------------------------------------------------------- the rule header, on the CPU under the sanitizers
def test_the_rule_header_agrees_with_sorting_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "despike_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h", "luma_bins.hpp"]  # nothing else of the project, nothing of HIP
    kernel = open(os.path.join(CSRC, "despike.hip")).read()
    for fn in ("despike_pixel(", "despike_settled(despike_at_or_above(", "despike_donor(", "despike_is_spike(", "despike_scaled("):
        assert fn in kernel, fn  # the kernel reads the same lines
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/despike_rule.hpp"' in mirror and "rmd::despike_donor(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "despike_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "despike_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "1", "100000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"despike rule ok: (\d+) windows, (\d+) with ties, (\d+) without a donor, (\d+) settled by the count, (\d+) spikes, (\d+) of them under a negative", r.stdout)
    assert m and int(m.group(1)) == 100000 and all(int(m.group(i)) > 1000 for i in range(2, 7))


# ---------------------------------------------------------------- the host mirrors
def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


def test_settings_defaults_and_rules():
    st = settings()
    assert st.despike is False
    assert st.despike_keywords() == dict(radius=2, rank=2, k=6.0, ratio=2.0, floor=0.0)
    on = settings(despike=True, despike_radius=3, despike_rank=47, despike_k=0.0, despike_ratio=1.0, despike_floor=0.5)
    on.check_despike(4)  # several devices are fine without the adaptive check
    assert on.despike_keywords() == dict(radius=3, rank=47, k=0.0, ratio=1.0, floor=0.5)
    for bad in (0, 4, -1, 2.0, True):
        with pytest.raises(ValueError, match=r"despike_radius must be an integer in \[1, 3\]"):
            settings(despike_radius=bad)  # checked whether or not the setting is on
    for radius, bad in ((1, 8), (2, 24), (3, 48), (2, -1), (2, 1.0)):
        with pytest.raises(ValueError, match="despike_rank must be an integer in"):
            settings(despike_radius=radius, despike_rank=bad)
    settings(despike_radius=1, despike_rank=7), settings(despike_radius=3, despike_rank=47)
    for name, bads in (("despike_k", (-1.0, float("nan"), float("inf"))), ("despike_ratio", (0.5, float("nan"), float("inf"))),
                       ("despike_floor", (-1e-9, float("nan"), float("inf")))):
        for bad in bads:
            with pytest.raises(ValueError, match=name + " must be finite and >="):
                settings(**{name: bad})
    with pytest.raises(ValueError, match="despike cannot be combined with denoise_dual: the halves are not yet despiked"):
        settings(despike=True, denoise=True, denoise_dual=True, samples_per_iteration=2)
    for dual_path in (dict(denoise_dual_features=True), dict(denoise_dual_select=True), dict(denoise_dual_atrous=True), dict(adaptive_denoised_threshold=0.1)):
        with pytest.raises(ValueError, match="the halves are not yet despiked"):
            settings(despike=True, denoise=True, denoise_dual=True, samples_per_iteration=2, **dual_path)
    adaptive = settings(despike=True, adaptive_threshold=0.1, samples_per_iteration=2)
    adaptive.check_despike(1)
    with pytest.raises(ValueError, match="despike with adaptive_threshold renders on one device"):
        adaptive.check_despike(2)
    with pytest.raises(ValueError, match="despike with adaptive_threshold renders on one device"):
        render.render_tiled(scenes.reflective_spheres(), adaptive, devices=(0, 1))  # render_tiled asks, before it opens a device
    on.despike_ratio = 0.5
    with pytest.raises(ValueError, match="despike_ratio"):
        render.render_tiled(scenes.reflective_spheres(), on)


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_parses_the_flags_and_holds_the_rules(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    base = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]
    for extra, word in ((["--despike-radius", "0"], "despike_radius must be in [1, 3]"),
                        (["--despike", "1", "--despike-radius", "4"], "despike_radius must be in [1, 3]"),
                        (["--despike-radius", "1", "--despike-rank", "8"], "despike_rank must be in [0, (2 * despike_radius + 1)^2 - 2]"),
                        (["--despike-rank", "24"], "despike_rank must be in [0, (2 * despike_radius + 1)^2 - 2]"),
                        (["--despike-k", "-1"], "despike_k must be finite and >= 0"),
                        (["--despike-k", "nan"], "despike_k must be finite and >= 0"),
                        (["--despike-ratio", "0.5"], "despike_ratio must be finite and >= 1"),
                        (["--despike-ratio", "inf"], "despike_ratio must be finite and >= 1"),
                        (["--despike-floor", "-0.1"], "despike_floor must be finite and >= 0"),
                        (["--despike", "1", "--denoise", "1", "--denoise-dual", "1", "--spi", "2"], "despike cannot be combined with denoise_dual: the halves are not yet despiked"),
                        (["--despike", "1", "--denoise", "1", "--denoise-dual", "1", "--denoise-dual-atrous", "1", "--spi", "2"], "the halves are not yet despiked"),
                        (["--despike", "1", "--adaptive", "0.1", "--spi", "2", "--gpus", "2"], "despike with adaptive_threshold renders on one device")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    header = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.hpp")).read()
    assert "bool despike = false;" in header and "uint32_t despike_radius = 2, despike_rank = 2;" in header
    assert "double despike_k = 6.0, despike_ratio = 2.0, despike_floor = 0.0;" in header


@pytest.mark.parametrize("size,radius,rank", [((37, 21), 2, 2), ((37, 21), 1, 0), ((37, 21), 3, 47), ((3, 2), 1, 2), ((1, 1), 2, 2)])
def test_the_cpp_mirrors_host_despike_is_the_restatements(cli, tmp_path, size, radius, rank):
    """raymond::despike_host — the rule header driven the way the kernel drives it, on the CPU — through `raymond_cli despike`, on the random frames the
    device test uses: the restatement's bytes and counts."""
    Wd, Hd = size
    S, Q, rects, counts = frames.random_frame(Wd, Hd, seed=7)
    S.tofile(tmp_path / "S.f64"), Q.tofile(tmp_path / "Q.f64")
    with open(tmp_path / "rects.txt", "w") as f:
        for (l, t, w, h), c in zip(rects, counts):
            f.write("%d %d %d %d %d\n" % (l, t, w, h, c))
    plan = ref.Plan(S, Q, rects, counts, radius, rank)
    total = 0
    for k, ratio, floor in ((6.0, 2.0, 0.0), (0.0, 1.0, 0.0), (6.0, 1.0, 0.25), (0.0, 2.0, 1e300)):
        r = subprocess.run([cli, "despike", str(tmp_path / "S.f64"), str(tmp_path / "Q.f64"), str(Wd), str(Hd), str(tmp_path / "rects.txt"), str(radius), str(rank),
                            float(k).hex(), float(ratio).hex(), float(floor).hex(), str(tmp_path / "oS.f64"), str(tmp_path / "oQ.f64")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        oS, oQ, replaced, spikes = plan.decide(k, ratio, floor)
        assert [int(v) for v in r.stdout.split()] == [int(v) for v in replaced]
        assert ref.same_bits(np.fromfile(tmp_path / "oS.f64").reshape(Hd, Wd, 3), oS) and ref.same_bits(np.fromfile(tmp_path / "oQ.f64").reshape(Hd, Wd, 3), oQ)
        if floor == 1e300:
            assert spikes == [] and ref.same_bits(oS, S) and ref.same_bits(oQ, Q)
        total += len(spikes)
    assert total > 0 or Wd * Hd < 9  # (the planted spikes are found)
