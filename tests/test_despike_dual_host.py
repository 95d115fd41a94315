"""rmd_despike_dual without a GPU: the export, the C++ mirror (raymond_cli despike-dual: the rule headers driven the way the kernel drives them) against the
numpy restatement tests/despike_dual_ref.py byte for byte, the hand-derived classes, the restatement told from four wrong readings of the definition, the
two statements the definition makes true against tests/despike_ref.py, the rule header under the host sanitizers, and the settings rule in both mirrors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import binding_trace as bt
import despike_dual_frames as frames
import despike_dual_ref as ref
import despike_ref
from raymond_amd import lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")


def test_entry_point_is_exported_and_declared(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT rmd_despike_dual\b", out)
    assert "rmd_despike_dual" in lib.SIGNATURES and callable(render.despike_dual) and callable(render.despike_dual_arrays)
    header = open(os.path.join(ROOT, "include", "raymond_hip.h")).read()
    assert "#define RMD_ABI_VERSION 6" in header and "rmd_status rmd_despike_dual(rmd_context *ctx," in header
    assert re.search(r"rmd_despike, rmd_despike_dual, rmd_tile_luma_error", header)  # in the list of calls that report RMD_ERR_DEVICE_FAULT


@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def run_cli(cli, tmp_path, SA, QA, SB, QB, rects, ca, cb, radius, rank, k=6.0, ratio=2.0, floor=0.0):
    """raymond_cli despike-dual on a frame: (S'_A, Q'_A, S'_B, Q'_B, replaced)."""
    H, W = SA.shape[0], SA.shape[1]
    names = [str(tmp_path / n) for n in ("SA.f64", "QA.f64", "SB.f64", "QB.f64")]
    outs = [str(tmp_path / n) for n in ("oSA.f64", "oQA.f64", "oSB.f64", "oQB.f64")]
    for a, n in zip((SA, QA, SB, QB), names):
        np.ascontiguousarray(a).tofile(n)
    with open(tmp_path / "rects.txt", "w") as f:
        for (l, t, w, h), a, b in zip(rects, ca, cb):
            f.write("%d %d %d %d %d %d\n" % (l, t, w, h, a, b))
    r = subprocess.run([cli, "despike-dual", *names, str(W), str(H), str(tmp_path / "rects.txt"), str(radius), str(rank), float(k).hex(), float(ratio).hex(), float(floor).hex(),
                        *outs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return tuple(np.fromfile(n).reshape(H, W, 3) for n in outs) + (np.array([int(v) for v in r.stdout.split()], dtype=np.uint32),)


def same_result(got, want):
    return all(ref.same_bits(g, w) for g, w in zip(got[:4], want[:4])) and [int(v) for v in got[4]] == [int(v) for v in want[4]]


# ---------------------------------------------------------------- the C++ mirror is the restatement
@pytest.mark.parametrize("size", frames.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("radius", frames.RADII)
def test_the_cpp_mirror_is_the_restatement_on_random_frames(cli, tmp_path, size, radius):
    SA, QA, SB, QB, rects, ca, cb = frames.frame(size)
    total = 0
    for rank in frames.ranks(radius):
        want = frames.reference(size, radius, rank)
        assert same_result(run_cli(cli, tmp_path, SA, QA, SB, QB, rects, ca, cb, radius, rank), want), (size, radius, rank)
        total += len(want[5])
    assert total > 0 or size[0] * size[1] < 9  # (the planted spikes are found)


def test_the_random_frames_hold_what_they_are_said_to_hold():
    SA, QA, SB, QB, rects, ca, cb = frames.frame((37, 21))
    assert sorted(zip(ca, cb)) == [(0, 8), (1, 1), (8, 8), (8, 8), (8, 16)] and sum(w * h for _, _, w, h in rects) < 37 * 21  # the four pairs, an uncovered strip
    finite_a, finite_b = np.isfinite(SA) & np.isfinite(QA), np.isfinite(SB) & np.isfinite(QB)
    assert (finite_a & ~finite_b).any() and (~finite_a & finite_b).any()  # NaN and infinities in one half only
    with np.errstate(all="ignore"):
        assert (finite_a & finite_b & ~np.isfinite(SA + SB)).any() and (finite_a & finite_b & ~np.isfinite(QA + QB)).any()  # finite halves whose sum overflows
    assert (SA < 0).any() and ((SA == 0) & np.signbit(SA)).any() and ((SA == 0) & ~np.signbit(SA)).any()  # negatives, zeros of both signs
    S, Q = ref.merge(SA, QA, SB, QB)
    na, _ = despike_ref.count_image(37, 21, rects, ca)
    nb, _ = despike_ref.count_image(37, 21, rects, cb)
    valid, Y, _ = ref.dual_planes(S, Q, na, nb)
    ys = Y[valid]
    assert len(ys) - len(np.unique(ys)) > 10  # exact ties
    spikes = frames.reference((37, 21), 2, 2)[5]
    assert any(frames.rect_of(rects, x, y) != frames.rect_of(rects, qx, qy) for x, y, qx, qy in spikes)  # a donor across a rect edge


# ---------------------------------------------------------------- the hand-derived classes
HAND = frames.HAND


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived_classes(cli, tmp_path, name):
    planes, expected = HAND[name]
    want = ref.despike_dual(*planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B)
    assert sorted(want[5]) == sorted(expected)  # the class is what it names
    frames.check_hand(name, planes, want)
    got = run_cli(cli, tmp_path, *planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B, 2, 2)
    assert same_result(got, want)
    frames.check_hand(name, planes, got)


# ---------------------------------------------------------------- the restatement against four wrong readings of the definition
WRONG_ON = {"per_half": "half_a_alone", "split_merged": "donor_in_8_16", "merged_counts": "donor_in_8_16", "merged_n_ge_2": "next_to_0_8"}


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_restatement_is_told_from_a_wrong_reading(variant):
    """Each wrong reading gives other bytes on the hand-made class that exists to catch it, and on the random frame."""
    planes, expected = HAND[WRONG_ON[variant]]
    right = ref.despike_dual(*planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B)
    wrong = ref.despike_dual(*planes, frames.HAND_RECTS, frames.HAND_A, frames.HAND_B, variant=variant)
    assert not all(ref.same_bits(a, b) for a, b in zip(right[:4], wrong[:4])), variant
    if variant == "per_half":  # half B sees no firefly: it keeps its pixel, and the halves are no longer the same pixels' samples
        assert ref.same_bits(wrong[3], planes[3]) and not ref.same_bits(right[3], planes[3])
    if variant == "split_merged":  # each half would hold half of BOTH halves' samples: the halves are no longer independent
        assert ref.same_bits(wrong[1][10, 19], wrong[3][10, 19]) and not ref.same_bits(right[1][10, 19], right[3][10, 19])
    if variant == "merged_counts":  # 16 against 24 merged samples scales half A too, which holds 8 against 8
        assert not ref.same_bits(wrong[0][10, 19], planes[0][10, 20]) and ref.same_bits(right[0][10, 19], planes[0][10, 20])
    if variant == "merged_n_ge_2":  # the (0, 8) pixels become others: another donor
        assert sorted(wrong[5]) != sorted(expected)
    SA, QA, SB, QB, rects, ca, cb = frames.frame((37, 21))
    wrong = ref.despike_dual(SA, QA, SB, QB, rects, ca, cb, 2, 2, variant=variant)
    assert not all(ref.same_bits(a, b) for a, b in zip(frames.reference((37, 21), 2, 2)[:4], wrong[:4])), variant


# ---------------------------------------------------------------- the two statements the definition makes true
@pytest.mark.parametrize("radius,rank", [(1, 0), (2, 2), (3, 47)])
def test_statement_a_the_spikes_are_those_of_despike_on_all_the_samples(radius, rank):
    """Every rect with both counts >= 1: the spike set, the donors and replaced equal rmd_despike's on S_A + S_B, Q_A + Q_B at n_A + n_B."""
    ca, cb = [8, 8, 1, 8, 3], [8, 16, 1, 8, 8]
    SA, QA, SB, QB, rects, _, _ = frames.random_frame(37, 21, seed=11, counts=(ca, cb))
    dual = ref.despike_dual(SA, QA, SB, QB, rects, ca, cb, radius, rank)
    S, Q = ref.merge(SA, QA, SB, QB)
    single = despike_ref.despike(S, Q, rects, [a + b for a, b in zip(ca, cb)], radius, rank)
    assert sorted(dual[5]) == sorted(single[3]) and len(single[3]) > 0
    assert [int(v) for v in dual[4]] == [int(v) for v in single[2]]


@pytest.mark.parametrize("radius,rank", [(1, 0), (2, 2), (3, 47)])
def test_statement_b_the_halves_add_to_despikes_outputs(radius, rank):
    """In addition every spike's counts agree with its donor's half by half (here: one pair of counts for the frame): S'_A + S'_B and Q'_A + Q'_B, one
    rounded addition, are rmd_despike's outputs bit for bit."""
    ca, cb = [8] * 5, [16] * 5
    SA, QA, SB, QB, rects, _, _ = frames.random_frame(37, 21, seed=12, counts=(ca, cb))
    dual = ref.despike_dual(SA, QA, SB, QB, rects, ca, cb, radius, rank)
    S, Q = ref.merge(SA, QA, SB, QB)
    single = despike_ref.despike(S, Q, rects, [24] * 5, radius, rank)
    assert sorted(dual[5]) == sorted(single[3]) and len(single[3]) > 0
    oS, oQ = ref.merge(dual[0], dual[1], dual[2], dual[3])
    assert ref.same_bits(oS, single[0]) and ref.same_bits(oQ, single[1])


# ---------------------------------------------------------------- the rule header, on the CPU under the sanitizers
def test_the_rule_header_agrees_with_a_plain_reading_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "despike_dual_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h", "despike_rule.hpp"]  # nothing else of the project, nothing of HIP
    kernel = open(os.path.join(CSRC, "despike_dual.hip")).read()
    for fn in ("despike_dual_pixel(", "despike_settled(despike_at_or_above(", "despike_donor(", "despike_is_spike(", "despike_dual_take("):
        assert fn in kernel, fn  # the kernel reads the same lines
    assert "asm" not in kernel
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/despike_dual_rule.hpp"' in mirror and "rmd::despike_dual_pixel(" in mirror and "rmd::despike_dual_take(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "despike_dual_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "despike_dual_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "1", "100000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"despike dual rule ok: (\d+) windows, (\d+) with a centre that is not valid, (\d+) without a donor, (\d+) spikes, (\d+) copied in both halves, "
                  r"(\d+) scaled in one, (\d+) scaled in both, (\d+) others with one empty half", r.stdout)
    assert m and int(m.group(1)) == 100000 and all(int(m.group(i)) > 1000 for i in range(2, 9))


# ---------------------------------------------------------------- the setting, in both mirrors
NEEDS = "despike_dual needs denoise_dual: it despikes the two halves"


def settings(**kw):
    return Settings(scenes.camera(96, 64), 8, **kw)


def test_settings_default_and_rule():
    assert settings().despike_dual is False
    on = settings(despike_dual=True, denoise=True, denoise_dual=True, samples_per_iteration=2, despike_radius=3, despike_rank=47)
    assert on.despike_dual is True and on.despike is False
    assert on.despike_keywords() == dict(radius=3, rank=47, k=6.0, ratio=2.0, floor=0.0)  # it reads the existing five
    for dual_path in (dict(denoise_dual_features=True), dict(denoise_dual_select=True), dict(denoise_dual_atrous=True), dict(adaptive_denoised_threshold=0.1),
                      dict(denoise_dual_atrous=True, denoise_dual_atrous_region=True, adaptive_denoised_threshold=0.1)):
        settings(despike_dual=True, denoise=True, denoise_dual=True, samples_per_iteration=2, **dual_path)
    for without in (dict(), dict(denoise=True), dict(despike=True), dict(denoise=True, denoise_atrous=True)):
        with pytest.raises(ValueError, match=re.escape(NEEDS)):
            settings(despike_dual=True, **without)
    with pytest.raises(ValueError, match=re.escape(NEEDS)):
        render.render_tiled(scenes.reflective_spheres(), _switched_on_later())  # render_tiled asks, before it opens a device


def _switched_on_later():
    st = settings()
    st.despike_dual = True
    return st


def test_every_older_refusal_is_still_raised_first_with_the_setting_on():
    """tests/test_despike_host.py's refusal texts, each with despike_dual on as well (and, where the case allows it, without denoise_dual, so that the new
    rule is broken too): the older text is the one raised."""
    for bad in (0, 4, -1, 2.0, True):
        with pytest.raises(ValueError, match=r"despike_radius must be an integer in \[1, 3\]"):
            settings(despike_dual=True, despike_radius=bad)
    for radius, bad in ((1, 8), (2, 24), (3, 48), (2, -1), (2, 1.0)):
        with pytest.raises(ValueError, match="despike_rank must be an integer in"):
            settings(despike_dual=True, despike_radius=radius, despike_rank=bad)
    for name, bads in (("despike_k", (-1.0, float("nan"), float("inf"))), ("despike_ratio", (0.5, float("nan"), float("inf"))),
                       ("despike_floor", (-1e-9, float("nan"), float("inf")))):
        for bad in bads:
            with pytest.raises(ValueError, match=name + " must be finite and >="):
                settings(despike_dual=True, **{name: bad})
    with pytest.raises(ValueError, match="despike cannot be combined with denoise_dual: the halves are not yet despiked"):
        settings(despike=True, despike_dual=True, denoise=True, denoise_dual=True, samples_per_iteration=2)
    for dual_path in (dict(denoise_dual_features=True), dict(denoise_dual_select=True), dict(denoise_dual_atrous=True), dict(adaptive_denoised_threshold=0.1)):
        with pytest.raises(ValueError, match="the halves are not yet despiked"):
            settings(despike=True, despike_dual=True, denoise=True, denoise_dual=True, samples_per_iteration=2, **dual_path)
    adaptive = settings(despike=True, adaptive_threshold=0.1, samples_per_iteration=2)
    adaptive.despike_dual = True
    with pytest.raises(ValueError, match="despike with adaptive_threshold renders on one device"):
        adaptive.check_despike(2)
    with pytest.raises(ValueError, match=re.escape(NEEDS)):
        adaptive.check_despike(1)


def test_cli_parses_the_flag_and_holds_the_rule_in_the_same_words(cli, tmp_path):
    """render_tiled (C++) throws raymond::Error before it starts a worker: no device is needed to see it."""
    base = [cli, "render", "spheres", "32", "32", "8", "2", str(tmp_path / "x.ppm")]
    for extra, word in ((["--despike-dual", "1"], NEEDS),
                        (["--despike-dual", "1", "--denoise", "1"], NEEDS),
                        (["--despike-dual", "1", "--despike", "1"], NEEDS),
                        (["--despike-dual", "1", "--despike-radius", "0"], "despike_radius must be in [1, 3]"),
                        (["--despike-dual", "1", "--despike-radius", "1", "--despike-rank", "8"], "despike_rank must be in [0, (2 * despike_radius + 1)^2 - 2]"),
                        (["--despike-dual", "1", "--despike-k", "-1"], "despike_k must be finite and >= 0"),
                        (["--despike-dual", "1", "--despike-ratio", "0.5"], "despike_ratio must be finite and >= 1"),
                        (["--despike-dual", "1", "--despike-floor", "-0.1"], "despike_floor must be finite and >= 0"),
                        (["--despike-dual", "1", "--despike", "1", "--denoise", "1", "--denoise-dual", "1", "--spi", "2"],
                         "despike cannot be combined with denoise_dual: the halves are not yet despiked"),
                        (["--despike-dual", "1", "--despike", "1", "--adaptive", "0.1", "--spi", "2", "--gpus", "2"], "despike with adaptive_threshold renders on one device")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
    header = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.hpp")).read()
    assert "bool despike_dual = false;" in header
    for path in (os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp"), os.path.join(ROOT, "raymond_amd", "scene.py")):
        assert '"' + NEEDS + '"' in open(path).read()  # the same words in both mirrors


# ---------------------------------------------------------------- the binding's C calls, on tests/binding_trace.py's recording stand-in (bt.installed())
def test_the_loader_declares_the_entry_point(product_lib):
    fn = product_lib.rmd_despike_dual
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 21 and list(fn.argtypes) == lib.SIGNATURES["rmd_despike_dual"][1]
    assert "rmd_despike_dual" in lib.SIGNATURES and len(lib.SIGNATURES["rmd_despike_dual"][1]) == 21


def test_the_wrappers_make_the_call_with_the_arguments_in_the_headers_order():
    with bt.installed() as fake:
        b = bt.Bench()
        try:
            outs = ((b.fbs[4], b.fbs[5]), (b.fbs[0], b.fbs[1]))  # (the stand-in checks no aliasing)
            a, bb, replaced = render.despike_dual(b.ctx, b.half_a, b.half_b, bt.RECTS, bt.COUNTS, bt.COUNTS_B, radius=1, rank=3, k=5.0, ratio=1.5, floor=0.25, out=outs)
            assert (a, bb) == outs and list(replaced) == [1, 2, 3, 4]  # (what the stand-in writes: the array that comes back is the one the call was given)
            rects = "[" + ",".join("[%d,%d,%d,%d]" % r for r in bt.RECTS) + "]"
            assert fake.lines[-1] == "rmd_despike_dual(ctx0,fb0,fb1,fb2,fb3,8,6,%s,[2,2,3,3],[1,2,3,4],4,1,3,5.0,1.5,0.25,fb4,fb5,fb0,fb1,out)" % rects
            made = render.despike_dual(b.ctx, b.half_a, b.half_b, bt.RECTS, bt.COUNTS, bt.COUNTS_B, want_replaced=False)  # four new buffers, NULL for the counts
            new = [fake._label(fb.ptr.value) for fb in made[0] + made[1]]
            assert made[2] is None and len(set(new)) == 4 and fake.lines[-1].endswith(",4,2,2,6.0,2.0,0.0,%s,0)" % ",".join(new))  # (NULL is shown as 0)
            for fb in made[0] + made[1]:
                fb.close()
            with pytest.raises(ValueError, match="one sample count per rect and half"):
                render.despike_dual(b.ctx, b.half_a, b.half_b, bt.RECTS, bt.COUNTS, bt.COUNTS_B[:3])
            fake.fail = ("rmd_despike_dual",)  # a refused call leaves no buffer behind
            live = list(fake.live)
            with pytest.raises(lib.RaymondError):
                render.despike_dual(b.ctx, b.half_a, b.half_b, bt.RECTS, bt.COUNTS, bt.COUNTS_B)
            assert fake.live == live
            fake.fail = ()
            got = render.despike_dual_arrays(b.ctx, bt.S3, bt.S3, bt.S3, bt.S3, bt.RECTS, bt.COUNTS, bt.COUNTS_B)
            assert [g.shape for g in got[:4]] == [(bt.H, bt.W, 3)] * 4 and len(got[4]) == 4 and fake.live == live
        finally:
            b.close()
        assert fake.live == []


@pytest.mark.parametrize("extra,filter_call", [(dict(), "rmd_denoise_dual_region("), (dict(denoise_dual_atrous=True, denoise_dual_atrous_region=True), "rmd_denoise_atrous_dual_region("),
                                               (dict(denoise_dual_atrous=True), "rmd_denoise_atrous_dual(")], ids=["default", "atrous_region", "atrous"])
def test_the_dual_loop_and_await_despike_before_every_filter_call(extra, filter_call):
    """The dual loop on the stand-in: one rmd_despike_dual call in front of each of the two checks' filter calls and one in front of await_()'s, each filter
    call on that call's four outputs — and with the setting off the same run makes none and allocates four buffers fewer."""
    def run(**kw):
        with bt.installed() as fake:
            fake.tile_errors = bt.first_converges
            handle = render.render_tiled(scenes.reflective_spheres(), bt._settings(**dict(bt.DUAL, adaptive_denoised_threshold=0.5, adaptive_min_samples=2, sample_count=6), **extra, **kw))
            assert fake.live == []
            handle.async_await()
            handle.await_()
            assert fake.live == []
            return list(fake.lines)

    off, on = run(), run(despike_dual=True, despike_radius=1, despike_rank=1, despike_k=5.0)
    assert not any(line.startswith("rmd_despike") for line in off)
    calls = [i for i, line in enumerate(on) if line.startswith("rmd_despike_dual(")]
    assert len(calls) == 3 and all(",1,1,5.0,2.0,0.0," in on[i] and on[i].endswith(",0)") for i in calls)
    for i in calls[:2]:  # the loop's: raw halves in, the spare buffers out, and the check's filter reads the spare buffers
        args = on[i].split("(", 1)[1]
        assert args.startswith("ctx0,fb0,fb1,fb2,fb3,8,6,")
        spare = args.rsplit(",0.0,", 1)[1].rsplit(",0)", 1)[0]
        assert len(set(spare.split(","))) == 4 and not set(spare.split(",")) & {"fb0", "fb1", "fb2", "fb3"}
        assert on[i + 1].startswith(filter_call + "ctx0," + spare + ","), on[i + 1]
    spares = {on[i].rsplit(",0.0,", 1)[1] for i in calls[:2]}
    assert len(spares) == 1  # the same four buffers in both passes
    outs = on[calls[2]].rsplit(",0.0,", 1)[1].rsplit(",0)", 1)[0].split(",")  # await_()'s: its four outputs come down, and then the filter is called
    assert [line.split(",")[1] for line in on[calls[2] + 1 : calls[2] + 5]] == outs and all(line.startswith("rmd_framebuffer_download(") for line in on[calls[2] + 1 : calls[2] + 5])
    assert next(line for line in on[calls[2] + 5 :] if line.startswith("rmd_denoise")).startswith(("rmd_denoise_dual(", "rmd_denoise_atrous_dual("))
    allocs = lambda lines: sum(1 for line in lines if line.startswith("rmd_framebuffer_alloc("))  # noqa: E731
    assert allocs(on) == allocs(off) + 4 + 8  # the loop's four spare buffers, and await_()'s despike_dual_arrays: four halves in, four out
